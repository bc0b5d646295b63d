"""KV-cached generation (DESIGN.md sections 12 to 15): the cache, the ``Generation`` mixin that gives ``Transformer`` its ``prefill /
decode_step / new_cache / extend / generate / generate_speculative / generate_lookup``, and the host logic under them.

The mixin alone takes a model, through the seam its docstring states (transformer.py imports this module, never the other way round);
``guard`` holds the refusals its methods share.  Everything else is plain functions over tensors on any device - the length checks, the
choice of the row a padded prompt is continued from, the token loop with its EOS freezing - so that tests/test_decode_host.py runs them
on the CPU with a fake step function.  The kernels are reached through two ops per cached step:
ops.kv_append_rope / ops.attn_decode for one token per sequence, ops.kv_append_rope_rows / ops.attn_extend for a chunk.  On-device
sampling adds the argument rules (check_sampling), the one draw of uniforms per call (draw_uniforms) and the
per-step pick (sampling_pick over ops.sample_logits).  Speculative decoding adds its refusals (check_speculative),
greedy acceptance (greedy_accept), the bookkeeping of a round (commit_round), the round loop over callables (speculative_loop), the one draw
of all its uniforms (speculative_uniforms) and ``_SpecSession``, the state of one call and the four callables the loop drives.  Draft-free
speculative decoding reuses that loop with ``_LookupSession``: the draft is ops.lookup_draft over the sequence's own
token history (check_lookup, lookup_uniforms, lookup_round_uniforms).  The fused decode step is a keyword of
decode_step, ``fused=True``, which runs every layer as one ops.decode_layer call, and generate_fused is generate over it (check_fused holds
its refusals).  The fused extend is the same keyword of extend, one ops.extend_layer call per layer, and
generate_lookup_fused is generate_lookup over it (check_fused_rows).  Both walk the layers with the host's one ``fused_layers``: a decode
step is the chunk of one row per sequence, told apart by its ``chunk`` argument alone.  The FP8 KV cache is a
format of ``KVCache`` (``kv_dtype='fp8'``, chosen by cfg.kv_cache or by prefill / new_cache's ``kv_dtype``): decode_step, extend and
fused_layers dispatch on the cache to the ops.*_kv8 twins of the same calls, and nothing else here knows about it.  Parallel sampling from
one prompt is ``SharedPrefixCache`` - a prefilled KVCache held once per prompt plus one suffix cache per sample -
made by ``fork``; decode_step dispatches on it to ops.kv_append_rope_at / ops.attn_decode_shared (fused: ops.decode_layer_shared), and
``generate_samples`` is generate over it (check_fork holds its refusals).  Beam search rides the same cache: ``fork_beam``
attaches ops.BeamBuffers to a fork (``cache.beam``), decode_step then attends the suffix through the buffers' ancestor table
(ops.attn_decode_beam, fused: ops.decode_layer_beam) and no cache row is copied when beams are re-parented; ``beam_loop`` is the host loop over
ops.beam_select / ops.beam_advance / ops.beam_finalize, ``generate_beam`` the public call (check_beam holds its refusals).  The paged KV
cache is ``PagePool`` - per-layer pages of ops.KV_PAGE_ROWS token rows and a host free list - and ``PagedKVCache`` - a
device block table with a host mirror, host upper bounds of the lengths, release / adopt; ``prefill_paged`` / ``new_cache_paged`` make one,
decode_step and extend dispatch on it to ops.kv_paged_append_rope_rows / ops.attn_decode_paged / ops.attn_extend_paged, and ``serve`` is
continuous batching over it (refuse_paged and refuse_paged_model hold its refusals); fused=True runs ops.decode_layer_paged /
ops.extend_layer_paged per layer.  Shared-prefix pages: ``PagePool`` counts a page's holders, ``prefill_prefix``
keeps a prompt prefix's whole pages once (``PagedPrefix``), ``PagedKVCache.admit_prefix`` starts sequences on them, ``step_ragged``
dispatches on such a cache to ops.attn_ragged_paged_cascade, and ``serve_shared`` is the chunked-prefill serving loop over it.
"""

import itertools
import math

import torch

from . import ops

KV_DTYPES = ('bf16', 'fp8')  # ModelConfig.kv_cache / KVCache.kv_dtype


def check_kv_dtype(kv_dtype):
  if kv_dtype not in KV_DTYPES:
    raise ValueError(f'kv_cache: {kv_dtype!r} is not one of {KV_DTYPES}')
  return kv_dtype


FINISH_CHECK_EVERY = 16  # generate: the one device-to-host read of the loop (have all sequences emitted eos_id?) at most this often


class KVCache:
  """Per-layer ``kv`` bf16 [B, Tmax, 2*dim] (row (b, j): the k | v columns of token j's rotated qkv row), ``lens`` int32 [B] on the
  device, and the status flag of the append kernel (checked by ``check``).  It owns no workspace: ops.attn_decode / ops.attn_extend take
  theirs from the workspace arena of the current stream.  kv_dtype 'fp8' (DESIGN.md section 20): ``kv`` is uint8 [B, Tmax, row_bytes]
  per layer, every row k codes | v codes | k scales | v scales (e4m3fn under one E8M0 scale per 16 elements of a head), 0.53 of the
  bf16 bytes; ``to_bf16(layer)`` is its exact bf16 image."""

  def __init__(self, n_layers, B, Tmax, n_heads, head_dim, device, kv_dtype='bf16'):
    dim = n_heads * head_dim
    self.B, self.Tmax, self.n_heads, self.head_dim = B, Tmax, n_heads, head_dim
    self.kv_dtype = check_kv_dtype(kv_dtype)
    self.row_bytes = ops.kv8_row_bytes(dim) if kv_dtype == 'fp8' else 4 * dim  # bytes per token and layer
    shape, dtype = ((B, Tmax, self.row_bytes), torch.uint8) if kv_dtype == 'fp8' else ((B, Tmax, 2 * dim), torch.bfloat16)
    self.kv = [torch.empty(shape, dtype=dtype, device=device) for _ in range(n_layers)]  # rows >= lens are never read
    # [pos | lens] = [lens - 1 | lens] during a decode step: one in-place add per step moves both, every layer reads the same pair
    self._pl = torch.zeros((2, B), dtype=torch.int32, device=device)
    self._pl[0] -= 1
    self.status = torch.zeros((1,), dtype=torch.int32, device=device)

  @property
  def lens(self):
    return self._pl[1]

  @property
  def pos(self):
    """Position of the token appended by the current decode step (lens - 1)."""
    return self._pl[0]

  def set_lens(self, lens):
    self._pl[1].copy_(lens)
    self._pl[0].copy_(lens - 1)

  def advance(self):
    self._pl += 1

  def advance_by(self, n_new):
    """Move [pos | lens] by n_new - an int32 [B] device tensor, or an int - with one in-place add (Transformer.extend, after its chunk)."""
    self._pl += n_new

  def commit_tree(self, path, n_accept):
    """After Transformer.extend_tree: keep the accepted root-to-leaf path (ops.tree_accept's path int32 [B, n] and n_accept int32 [B]) -
    every layer's rows lens + path[d] move to lens + d in one ops.kv_tree_commit launch - and move the lengths by n_accept + 1, the root
    included, on the device.  bf16 caches only."""
    if self.kv_dtype != 'bf16':
      raise ValueError(f"KVCache.commit_tree: a {self.kv_dtype!r} cache has no tree path (bf16 caches only)")
    ops.kv_tree_commit(self.kv, self.lens, path, n_accept, self.n_heads)
    self.advance_by(n_accept + 1)

  def to_bf16(self, layer):
    """Layer ``layer``'s cache as bf16 [B, Tmax, 2*dim]: the buffer itself, or the exact dequantised image of an fp8 cache (rows at and
    beyond lens hold whatever the buffer holds there)."""
    if self.kv_dtype == 'fp8':
      return ops.kv8_dequant_rows(self.kv[layer], self.n_heads, self.head_dim)
    return self.kv[layer]

  def check(self):
    """Raises if a decode step tried to append past the cache (or past the RoPE table); reads the device flag, so it waits for the GPU."""
    if int(self.status.item()) != 0:
      raise RuntimeError(f'KVCache: a decode step appended at a position outside [0, {self.Tmax}): that token was not stored '
                         '(prefill with a larger max_len)')


class SharedPrefixCache:
  """G continuations per prompt on top of ONE copy of the prompts' cache.  ``prefix``: the prefilled bf16 KVCache
  of the P prompts, read-only from here on; ``kv``: per layer the suffix buffer bf16 [P*G, Ts_max, 2*dim], sequence p*G + g = sample g of
  prompt p, row j = the sample's j-th own token; ``[pos | lens]`` of the suffix as KVCache keeps them (one in-place add per step);
  ``rot0`` int32 [P*G] = the prompts' lengths repeated G times, on the device: suffix row j of sample i is rotated at rot0[i] + j.
  ``status`` / ``check()`` as KVCache's: a step past Ts_max (or past the RoPE table) stores nothing and raises the flag.  ``beam``: None, or
  the ops.BeamBuffers of a beam search (``fork_beam``): suffix slot g then holds the rows beam g WROTE, and a beam attends the rows its
  ancestor table names."""
  kv_dtype = 'bf16'
  beam = None

  def __init__(self, prefix, n_samples, max_new_tokens):
    G, Ts = check_fork(prefix, n_samples, max_new_tokens)
    self.prefix, self.G, self.P, self.B, self.Tmax = prefix, G, prefix.B, prefix.B * G, Ts
    self.n_heads, self.head_dim = prefix.n_heads, prefix.head_dim
    dev = prefix.status.device
    self.kv = [torch.empty((self.B, Ts, 2 * self.n_heads * self.head_dim), dtype=torch.bfloat16, device=dev) for _ in prefix.kv]
    self._pl = torch.zeros((2, self.B), dtype=torch.int32, device=dev)
    self._pl[0] -= 1
    self.rot0 = prefix.lens.repeat_interleave(G).contiguous()
    self.status = torch.zeros((1,), dtype=torch.int32, device=dev)

  lens = KVCache.lens
  pos = KVCache.pos
  advance = KVCache.advance

  def cache_bytes(self):
    """Bytes of cache held for all layers: the prefix once, (Tp_max + G * Ts_max) rows per prompt."""
    return sum(t.numel() * t.element_size() for t in self.prefix.kv + self.kv)

  def check(self):
    if int(self.status.item()) != 0:
      raise RuntimeError(f'SharedPrefixCache: a decode step appended at a row outside [0, {self.Tmax}) or past the RoPE table: that token was '
                         'not stored (fork with a larger max_new_tokens)')


class PagePool:
  """The pages of a paged KV cache: per layer ``kv`` bf16 [n_pages, ops.KV_PAGE_ROWS, 2*dim] in KVCache's row
  layout, and a host free list.  One page id means the same page in every layer.  ``alloc(k)`` hands out k page ids and raises
  RuntimeError when fewer are free - on the host, before anything is launched; ``free(ids)`` takes them back.  Pages are counted by
  their holders: ``share(ids)`` adds one, ``free`` drops one, and a page is free again when none is left; ``n_free`` and
  ``bytes_in_use`` count a shared page once.  bf16 pages only."""

  def __init__(self, n_layers, n_pages, n_heads, head_dim, device, kv_dtype='bf16'):
    if check_kv_dtype(kv_dtype) != 'bf16':
      raise ValueError(f'PagePool: {kv_dtype!r} pages are not served (the paged kernels read bf16 pages)')
    if int(n_pages) < 1:
      raise ValueError(f'PagePool: n_pages must be at least 1, got {n_pages}')
    self.n_pages, self.n_heads, self.head_dim = int(n_pages), n_heads, head_dim
    shape = (self.n_pages, ops.KV_PAGE_ROWS, 2 * n_heads * head_dim)
    self.kv = [torch.empty(shape, dtype=torch.bfloat16, device=device) for _ in range(n_layers)]  # rows >= a sequence's length are never read
    self._free = list(range(self.n_pages - 1, -1, -1))  # a stack: page 0 goes out first, a freed page is reused first
    self._used = [0] * self.n_pages  # holders of every page: alloc makes one, share adds one, free drops one

  @property
  def n_free(self):
    return len(self._free)

  def alloc(self, k):
    if k > len(self._free):
      raise RuntimeError(f'PagePool: {k} pages asked for, {len(self._free)} of {self.n_pages} free (nothing was launched): release sequences or '
                         'make a larger pool')
    ids = [self._free.pop() for _ in range(k)]
    for p in ids:
      self._used[p] = 1
    return ids

  def _held(self, what, ids):
    ids = list(ids)
    if any(not 0 <= p < self.n_pages or not self._used[p] for p in ids) or len(set(ids)) != len(ids):
      raise ValueError(f'PagePool.{what}: {ids} are not all pages in use')
    return ids

  def share(self, ids):
    """One more holder of pages in use: they return to the free list when every holder has freed them."""
    for p in self._held('share', ids):
      self._used[p] += 1

  def free(self, ids):
    ids = self._held('free', ids)
    for p in ids:
      self._used[p] -= 1
    self._free.extend(p for p in reversed(ids) if not self._used[p])

  def bytes_in_use(self):
    """Bytes of the pages handed out, all layers."""
    return (self.n_pages - len(self._free)) * sum(t[0].numel() * t.element_size() for t in self.kv)


class PagedPrefix:
  """A prompt prefix kept once in a PagePool: ``pages``, the ids of its whole pages, held by this object;
  ``n_tokens`` = 64 * len(pages), the tokens they hold; ``rest``, the tokens past the last whole page, which every member sequence
  feeds itself.  ``PagedKVCache.admit_prefix`` starts sequences on the pages; ``release()`` drops this object's hold (the pages are
  free again once the last member has left).  Made by ``Transformer.prefill_prefix``."""
  _ids = itertools.count()

  def __init__(self, pool, pages, rest):
    self.pool, self.pages, self.rest = pool, list(pages), rest
    self.n_tokens = ops.KV_PAGE_ROWS * len(self.pages)
    self.group = next(PagedPrefix._ids)  # what cascade_plan groups the members by

  def release(self):
    self.pool.free(self.pages)
    self.pages, self.n_tokens = [], 0


class PagedKVCache:
  """B sequences over a PagePool: ``table`` int32 [B, max_pages] on the device (entry (b, i): the page of tokens
  64*i .. 64*i + 63 of sequence b, -1 for none) with a host mirror, ``[pos | lens]`` and ``status`` as KVCache keeps them, ``live`` int32
  [B] (1: the slot holds a sequence, 0: idle - an idle slot keeps pos = lens = 0, appends nothing and attends nothing), and per sequence
  a HOST upper bound of its length.  Pages are taken on the host, before a step, whenever a bound crosses a page boundary (``reserve``);
  the changed table rows go to the device as one copy when ``table`` is next read, and nothing is ever read back from the device."""
  kv_dtype = 'bf16'

  def __init__(self, pool, B, max_len):
    if not isinstance(pool, PagePool):
      raise TypeError(f'PagedKVCache: pool must be a PagePool, got {type(pool).__name__}')
    if int(B) < 1 or int(max_len) < 1:
      raise ValueError(f'PagedKVCache: need B >= 1 and max_len >= 1, got B={B} max_len={max_len}')
    self.pool, self.B, self.Tmax = pool, int(B), int(max_len)
    self.n_heads, self.head_dim = pool.n_heads, pool.head_dim
    self.max_pages = -(-self.Tmax // ops.KV_PAGE_ROWS)
    dev = pool.kv[0].device
    self._table = torch.full((self.B, self.max_pages), -1, dtype=torch.int32, device=dev)
    self._mirror = torch.full((self.B, self.max_pages), -1, dtype=torch.int32)
    self._dirty = None  # (first, last) changed row of the mirror
    self.pages = [[] for _ in range(self.B)]
    self.bound = [0] * self.B
    self._live = [False] * self.B
    self.key_lo = [0] * self.B     # the keys slot b shares with its group (whole pages; 0: none) ...
    self.group = [None] * self.B   # ... and the group: the PagedPrefix's id
    self._pl = torch.zeros((2, self.B), dtype=torch.int32, device=dev)
    self.live = torch.zeros((self.B,), dtype=torch.int32, device=dev)
    self.status = torch.zeros((1,), dtype=torch.int32, device=dev)

  lens = KVCache.lens
  pos = KVCache.pos

  @property
  def kv(self):
    return self.pool.kv

  @property
  def table(self):
    if self._dirty is not None:
      lo, hi = self._dirty
      src = self._mirror[lo:hi + 1].clone()  # a snapshot: the mirror may change again before the copy has run
      self._table[lo:hi + 1].copy_(src.pin_memory() if self._table.is_cuda else src, non_blocking=True)
      self._dirty = None
    return self._table

  def _touch(self, b):
    self._dirty = (b, b) if self._dirty is None else (min(b, self._dirty[0]), max(b, self._dirty[1]))

  def lcap(self):
    """The keys of the table worth walking: the largest host bound, rounded up to whole chunks of ops.KV_PAGED_CHUNK."""
    c = ops.KV_PAGED_CHUNK
    return min(self.max_pages * ops.KV_PAGE_ROWS, max(1, -(-max(self.bound) // c)) * c)

  def reserve(self, extra):
    """Move the host bounds by ``extra`` (an int for every live sequence, or B ints) and take the pages the new bounds need - all of
    them or, when the pool is short, none (RuntimeError).  A bound beyond max_len takes no page: the append refuses that sequence."""
    extra = [int(extra) if live else 0 for live in self._live] if isinstance(extra, int) else [int(v) for v in extra]
    want = [min(-(-(self.bound[b] + extra[b]) // ops.KV_PAGE_ROWS), self.max_pages) - len(self.pages[b]) if extra[b] > 0 else 0
            for b in range(self.B)]
    want = [max(w, 0) for w in want]
    ids = self.pool.alloc(sum(want))
    for b, w in enumerate(want):
      for _ in range(w):
        self._mirror[b, len(self.pages[b])] = ids[0]
        self.pages[b].append(ids.pop(0))
      if w:
        self._touch(b)
      self.bound[b] += extra[b]

  def set_lens(self, lens):
    """Host integers (B ints or a CPU tensor): every sequence becomes live with that length; pages are taken or returned to match."""
    if isinstance(lens, torch.Tensor) and lens.is_cuda:
      raise TypeError('PagedKVCache.set_lens: pass host integers (they size the page lists before anything is launched)')
    vals = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
    if len(vals) != self.B or any(v < 0 or v > self.Tmax for v in vals):
      raise ValueError(f'PagedKVCache.set_lens: need {self.B} lengths in [0, {self.Tmax}], got {vals}')
    if any(v < k for v, k in zip(vals, self.key_lo)):
      raise ValueError(f'PagedKVCache.set_lens: {vals} cut into the shared prefixes {self.key_lo} (release the slot instead)')
    for b, v in enumerate(vals):
      keep = -(-v // ops.KV_PAGE_ROWS)
      if len(self.pages[b]) > keep:
        self.pool.free(self.pages[b][keep:])
        del self.pages[b][keep:]
        self._mirror[b, keep:] = -1
        self._touch(b)
      self.bound[b] = min(self.bound[b], v)
    self._live = [True] * self.B
    self.reserve([v - self.bound[b] for b, v in enumerate(vals)])
    t = torch.tensor([[v - 1 for v in vals], vals], dtype=torch.int32)
    self._pl.copy_(t.to(self._pl.device))
    self.live.fill_(1)

  def advance(self):
    """One token per live sequence: its page when the bound crosses a page edge, then one in-place add of ``live``."""
    self.reserve(1)
    self._pl += self.live

  def advance_by(self, n_new, bound=None):
    """Move [pos | lens] by n_new (an int, or an int32 [B] device tensor) after ``reserve`` has moved the host bounds; or pass
    ``bound`` (host ints) to do both here."""
    if bound is not None:
      self.reserve(bound)
    self._pl += n_new * self.live if isinstance(n_new, int) else n_new

  def admit(self, b):
    """The idle slot b becomes a live sequence of length 0 that holds no page yet: the start of a prompt fed through ragged steps
    (DESIGN.md section 26)."""
    if self._live[b] or self.pages[b]:
      raise ValueError(f'PagedKVCache.admit: slot {b} holds a sequence (release it first)')
    self._live[b] = True
    self._pl[0, b] = -1  # pos = lens - 1, as set_lens keeps it
    self.live[b] = 1

  def admit_prefix(self, b, prefix):
    """The idle slot b becomes a live sequence of length prefix.n_tokens on the prefix's pages: its first
    table entries are the prefix's page ids, of which it is one more holder; its key_lo and group say so to ``step_ragged``.  Its
    appends take fresh pages - the length starts at a page edge - so a shared page is never written.  A prefix without a whole
    page is ``admit``."""
    if not isinstance(prefix, PagedPrefix) or prefix.pool is not self.pool:
      raise ValueError('PagedKVCache.admit_prefix: the prefix must be a PagedPrefix on the same pool')
    if self._live[b] or self.pages[b]:
      raise ValueError(f'PagedKVCache.admit_prefix: slot {b} holds a sequence (release it first)')
    n = prefix.n_tokens
    if n >= self.Tmax:
      raise ValueError(f'PagedKVCache.admit_prefix: the prefix holds {n} tokens, this cache {self.Tmax} per sequence')
    if not n:
      return self.admit(b)
    self.pool.share(prefix.pages)
    self.pages[b] = list(prefix.pages)
    self._mirror[b, :len(self.pages[b])] = torch.tensor(self.pages[b], dtype=torch.int32)
    self._touch(b)
    self.bound[b], self._live[b], self.key_lo[b], self.group[b] = n, True, n, prefix.group
    self._pl[:, b] = torch.tensor([n - 1, n], dtype=torch.int32)
    self.live[b] = 1

  def ship(self, *words):
    """Host int32 tensors -> their device copies, as ONE non-blocking copy from a pinned snapshot (the way ``table`` ships its rows)."""
    src = torch.cat([w.reshape(-1) for w in words])
    dev = torch.empty(src.shape, dtype=torch.int32, device=self._table.device)
    dev.copy_(src.pin_memory() if dev.is_cuda else src, non_blocking=True)
    return dev.split([w.numel() for w in words])

  def release(self, b):
    """Sequence b leaves: its pages go back to the pool (a shared page loses one holder), its table row to -1, its length to 0; the
    slot is idle."""
    self.pool.free(self.pages[b])
    self.pages[b], self.key_lo[b], self.group[b] = [], 0, None
    self._mirror[b] = -1
    self._touch(b)
    self.bound[b], self._live[b] = 0, False
    self._pl[:, b] = 0
    self.live[b] = 0

  def adopt(self, b, other, j):
    """Sequence j of ``other`` (a cache on the same pool) moves into the idle slot b: page ids move, no row is copied."""
    if not isinstance(other, PagedKVCache) or other.pool is not self.pool:
      raise ValueError('PagedKVCache.adopt: the other cache must be a PagedKVCache on the same pool')
    if self._live[b] or self.pages[b]:
      raise ValueError(f'PagedKVCache.adopt: slot {b} holds a sequence (release it first)')
    if len(other.pages[j]) > self.max_pages or other.bound[j] > self.Tmax:
      raise ValueError(f'PagedKVCache.adopt: the sequence holds {other.bound[j]} tokens, this cache {self.Tmax} per sequence')
    self.pages[b], other.pages[j] = other.pages[j], []
    self.key_lo[b], self.group[b], other.key_lo[j], other.group[j] = other.key_lo[j], other.group[j], 0, None
    self._mirror[b, :len(self.pages[b])] = torch.tensor(self.pages[b], dtype=torch.int32)
    other._mirror[j] = -1
    self._touch(b)
    other._touch(j)
    self.bound[b], self._live[b] = other.bound[j], True
    other.bound[j], other._live[j] = 0, False
    self._pl[:, b].copy_(other._pl[:, j])
    self.live[b] = 1
    other._pl[:, j] = 0
    other.live[j] = 0

  def prefill_sink(self, layer):
    """What the trunk hands layer ``layer``'s rotated k | v rows [B, T, 2*dim] to: one ops.kv_paged_store_rows launch."""
    return lambda rows: ops.kv_paged_store_rows(rows, self.lens, self.pool.kv[layer], self.table, self.n_heads, status=self.status)

  def gather(self, layer):
    """Layer ``layer`` as the contiguous image bf16 [B, max_pages * 64, 2*dim], by torch indexing (rows of missing pages and rows at and
    beyond lens hold whatever page 0 / the page holds).  For tests and debugging only."""
    t = self.table.clamp(min=0).long()
    return self.pool.kv[layer][t].reshape(self.B, self.max_pages * ops.KV_PAGE_ROWS, -1)

  def check(self):
    if int(self.status.item()) != 0:
      raise RuntimeError(f'PagedKVCache: a step appended past max_len {self.Tmax} (or the RoPE table) or into a missing page: those tokens '
                         'were not stored')


def refuse_paged(what, cache):
  if isinstance(cache, PagedKVCache):
    raise TypeError(f'Transformer.{what}: a PagedKVCache takes prefill_paged, decode_step, extend and serve only (no fork, no tree rows, no '
                    'speculative or lookup rounds)')


def refuse_paged_model(what, model):
  if model.cfg.linear_precision == 'mxfp8':
    raise ValueError(f'Transformer.{what}: linear_precision: mxfp8 has no paged cache path (the cached step runs the bf16 shadows)')
  if model.cfg.kv_cache != 'bf16':
    raise ValueError(f"Transformer.{what}: cfg.kv_cache = {model.cfg.kv_cache!r}: FP8 pages are not served (the paged kernels read bf16 pages)")


def check_fork(cache, n_samples, max_new_tokens):
  """The refusals of Transformer.fork that need no GPU; returns (G, suffix rows per sample)."""
  refuse_paged('fork', cache)
  if isinstance(cache, SharedPrefixCache):
    raise TypeError('fork: the cache is already a fork (a SharedPrefixCache cannot be forked again: fork its prefix)')
  if not isinstance(cache, KVCache):
    raise TypeError(f'fork: cache must be a prefilled KVCache, got {type(cache).__name__}')
  if cache.kv_dtype != 'bf16':
    raise ValueError(f"fork: a {cache.kv_dtype!r} cache cannot be shared (the shared-prefix kernels read bf16 prefix and suffix rows): prefill "
                     "with kv_dtype='bf16'")
  if isinstance(n_samples, bool) or not isinstance(n_samples, int) or n_samples < 1:
    raise ValueError(f'fork: n_samples must be an int >= 1, got {n_samples!r}')
  if int(max_new_tokens) < 1:
    raise ValueError(f'fork: max_new_tokens must be at least 1, got {max_new_tokens}')
  return n_samples, int(max_new_tokens)


def refuse_shared(what, cache):
  if isinstance(cache, SharedPrefixCache):
    raise TypeError(f'Transformer.{what}: a SharedPrefixCache takes decode steps only (decode_step, generate_samples): no chunks, no '
                    'speculative or lookup rounds')


def refuse_shared_mxfp8(what, model):
  if model.cfg.linear_precision == 'mxfp8':
    raise ValueError(f'Transformer.{what}: linear_precision: mxfp8 has no shared-prefix decode path (the decode step runs the bf16 shadows)')


def refuse_cpu(tokens):
  if isinstance(tokens, torch.Tensor) and not tokens.is_cuda:
    raise RuntimeError('plainlm_amd.Transformer runs on MI355X only (inputs are on CPU; there is no CPU fallback)')


def refuse_mxfp8(what, model):
  if model.cfg.linear_precision == 'mxfp8':
    raise NotImplementedError(f"Transformer.{what}: linear_precision: mxfp8 has no cached decode path (the decode step runs the bf16 shadows)")


def guard(what, tokens, model, *drafts, forward_only=False, rank2=False):
  """The refusals the generation methods share.  Their order decides which one an input that is bad in two ways gets; it is pinned by
  tests/test_generate_trace_host.py and tests/test_generate_trace_gpu.py.  A forward-only method (generate, generate_speculative) first
  refuses CPU tokens, a draft that is no Generation, and grad mode while any of the models has a trainable parameter.  Then every method
  refuses an mxfp8 model, tokens that are no int64 tensor, CPU tokens, an mxfp8 draft and, with ``rank2``, tokens that are not [B, T]."""
  if forward_only:
    refuse_cpu(tokens)
    for d in drafts:
      if not isinstance(d, Generation):
        raise TypeError(f'{what}: draft must be a plainlm_amd.Transformer, got {type(d).__name__}')
    if torch.is_grad_enabled() and any(p.requires_grad for m in (model,) + drafts for p in m.parameters()):
      raise RuntimeError(f'Transformer.{what} is forward-only (no backward): call it under torch.no_grad(), or use loss() to train')
  refuse_mxfp8(what, model)
  if not isinstance(tokens, torch.Tensor) or tokens.dtype != torch.int64:
    raise TypeError(f'Transformer.{what}: tokens must be an int64 tensor')
  refuse_cpu(tokens)
  for d in drafts:
    refuse_mxfp8(what, d)
  if rank2 and tokens.dim() != 2:
    raise TypeError('inputs must be an int64 [B, T] tensor')


def check_cache(who, cache, model):
  """A cache made for another model shape is refused before any library call (its format is its own: every method dispatches on
  cache.kv_dtype)."""
  if len(cache.kv) != model.n_layers or cache.n_heads != model.cfg.n_heads or cache.head_dim != model.head_dim or \
     getattr(cache, 'kv_dtype', None) not in KV_DTYPES:
    raise ValueError(f'{who}: the cache was made for another model shape (layers, heads or head_dim differ)')


def chunk_lens(token_lens, B, n, device):
  """token_lens of Transformer.extend as (what advance_by takes, the int32 [B] device tensor the kernels take or None for "n
  everywhere").  None: every sequence appends all n tokens.  Host integers (a sequence of B ints in [0, n], or a CPU tensor) are checked
  here and copied to the device; an int32 [B] device tensor is never read back: it is clamped to [0, n] on the device (as the kernels
  clamp it), so that the lengths move by what was appended and the gather of the last rows stays inside the chunk."""
  if token_lens is None:
    return int(n), None
  if isinstance(token_lens, torch.Tensor) and token_lens.device.type != 'cpu':
    if token_lens.dtype != torch.int32 or tuple(token_lens.shape) != (B,):
      raise TypeError(f'extend: a device token_lens must be an int32 [{B}] tensor, got {token_lens.dtype} {tuple(token_lens.shape)}')
    t = token_lens.clamp(0, int(n))
    return t, t
  vals = token_lens.tolist() if isinstance(token_lens, torch.Tensor) else list(token_lens)
  vals = [int(v) for v in vals]
  if len(vals) != B:
    raise ValueError(f'extend: {len(vals)} token_lens for a batch of {B}')
  if any(v < 0 or v > n for v in vals):
    raise ValueError(f'extend: every token_lens must be in [0, {n}] (the token tensor\'s width), got {vals}')
  t = torch.tensor(vals, dtype=torch.int32).to(device)
  return t, t


def check_fused_dim(who, dim):
  if dim % 32 != 0:
    raise ValueError(f'{who}: fused=True needs cfg.dim % 32 == 0, got {dim}: leave fused off')


def check_fused(who, B, dim):
  """The refusals of fused=True that need no GPU: the skinny-M kernels take at most ops.FUSED_DECODE_MAX_ROWS rows and dim % 32 == 0."""
  if B > ops.FUSED_DECODE_MAX_ROWS:
    raise ValueError(f'{who}: fused=True serves at most {ops.FUSED_DECODE_MAX_ROWS} sequences, got {B}: leave fused off')
  check_fused_dim(who, dim)


def check_fused_rows(who, B, n, dim):
  """check_fused for a chunk of n rows per sequence: the skinny-M kernels take at most ops.FUSED_EXTEND_MAX_ROWS rows, B * n of them."""
  if B * n > ops.FUSED_EXTEND_MAX_ROWS:
    raise ValueError(f'{who}: fused=True serves at most {ops.FUSED_EXTEND_MAX_ROWS} chunk rows, got {B} sequences x {n} rows = {B * n}: leave fused off')
  check_fused_dim(who, dim)


def check_ragged(tokens, counts, cache, fused, dim):
  """The refusals of Transformer.step_ragged that need no GPU; returns (R, the counts as a list of cache.B ints)."""
  who = 'step_ragged'
  if not isinstance(tokens, torch.Tensor) or tokens.dtype != torch.int64 or tokens.dim() != 1 or tokens.numel() < 1:
    raise TypeError(f'Transformer.{who}: tokens must be a non-empty int64 [R] tensor, packed in slot order')
  counts = [int(c) for c in (counts.tolist() if isinstance(counts, torch.Tensor) else counts)]
  R = tokens.numel()
  if len(counts) != cache.B or any(c < 0 for c in counts):
    raise ValueError(f'{who}: need {cache.B} counts (one per slot, none negative), got {counts}')
  if sum(counts) != R:
    raise ValueError(f'{who}: the counts {counts} sum to {sum(counts)}, the step has {R} rows')
  for b, c in enumerate(counts):
    if c and not cache._live[b]:
      raise ValueError(f'{who}: slot {b} is idle and must have count 0, got {c}')
    if cache.bound[b] + c > cache.Tmax:
      raise ValueError(f'{who}: slot {b} holds {cache.bound[b]} tokens, {c} more do not fit max_len {cache.Tmax}')
  check_fused_kind(who, fused)
  if fused is True and any(cache.key_lo):
    raise ValueError(f'{who}: fused=True has no cascade variant and the cache holds sequences on shared prefix pages: pass fused=\'wide\' or '
                     'leave fused off')
  if fused == 'wide':
    if R > ops.FUSED_WIDE_MAX_ROWS:
      raise ValueError(f'{who}: fused=\'wide\' serves at most {ops.FUSED_WIDE_MAX_ROWS} packed rows, got {R}: leave fused off')
    check_wide_dim(who, dim)
  elif fused:
    if R > ops.FUSED_EXTEND_MAX_ROWS:
      raise ValueError(f'{who}: fused=True serves at most {ops.FUSED_EXTEND_MAX_ROWS} packed rows, got {R}: leave fused off')
    check_fused_dim(who, dim)
  return R, counts


def check_fused_kind(who, fused):
  """fused of step_ragged and serve: False, True (the skinny-M kernels) or 'wide' (the wide kernels, section 27)."""
  if not isinstance(fused, bool) and fused != 'wide':
    raise ValueError(f'{who}: fused must be False, True or \'wide\', got {fused!r}')


def check_wide_dim(who, dim):
  if dim % 32 != 0:
    raise ValueError(f'{who}: fused=\'wide\' needs cfg.dim % 32 == 0, got {dim}: leave fused off')


def check_prefill_chunk(who, prefill_chunk, max_batch, fused):
  """serve's prefill_chunk as an int >= 1; with fused, a step's max_batch decode rows + prefill_chunk prompt rows must fit the skinny-M
  kernels (True) or the wide ones ('wide')."""
  if isinstance(prefill_chunk, bool) or not isinstance(prefill_chunk, int) or prefill_chunk < 1:
    raise ValueError(f'{who}: prefill_chunk must be None or an int >= 1, got {prefill_chunk!r}')
  if fused == 'wide':
    if int(max_batch) + prefill_chunk > ops.FUSED_WIDE_MAX_ROWS:
      raise ValueError(f'{who}: fused=\'wide\' serves at most {ops.FUSED_WIDE_MAX_ROWS} rows a step, got max_batch {max_batch} + prefill_chunk '
                       f'{prefill_chunk}: feed smaller chunks')
  elif fused and int(max_batch) + prefill_chunk > ops.FUSED_EXTEND_MAX_ROWS:
    raise ValueError(f'{who}: fused=True serves at most {ops.FUSED_EXTEND_MAX_ROWS} rows a step, got max_batch {max_batch} + prefill_chunk '
                     f'{prefill_chunk}: leave fused off or feed smaller chunks')
  return prefill_chunk


def pad4(n):
  return (int(n) + 3) // 4 * 4


def prompt_lens_list(prompt_lens, B, T):
  """prompt_lens (None | a sequence of ints | an integer tensor on the host) as a list of B ints in [1, T]."""
  if prompt_lens is None:
    return [int(T)] * B
  if isinstance(prompt_lens, torch.Tensor):
    if prompt_lens.is_cuda:
      raise TypeError('prompt_lens: pass host integers (a list, a tuple or a CPU tensor): they size the cache before anything is launched')
    prompt_lens = prompt_lens.tolist()
  lens = [int(v) for v in prompt_lens]
  if len(lens) != B:
    raise ValueError(f'prompt_lens: {len(lens)} lengths for a batch of {B}')
  if any(v < 1 or v > T for v in lens):
    raise ValueError(f'prompt_lens: every length must be in [1, {T}] (the prompt tensor\'s width), got {lens}')
  return lens


def _check_new_tokens(who, T, max_new_tokens, extra, extra_text, limits):
  """The length refusals of ``who``: returns T + max_new_tokens + extra (spelled extra_text), which must fit every (owner, seq_len)."""
  if int(max_new_tokens) < 1:
    raise ValueError(f'{who}: max_new_tokens must be at least 1, got {max_new_tokens}')
  if T < 1:
    raise ValueError(f'{who}: empty prompt')
  need = T + int(max_new_tokens) + extra
  for owner, seq_len in limits:
    if need > seq_len:
      raise ValueError(f'{who}: prompt length {T} + max_new_tokens {max_new_tokens}{extra_text} exceeds {owner}cfg.seq_len {seq_len}')
  return need


def check_lengths(T, max_new_tokens, seq_len):
  """The refusals of generate that need no GPU; returns the cache length (the padded prompt must fit it too)."""
  return max(pad4(T), _check_new_tokens('generate', T, max_new_tokens, 0, '', [('', seq_len)]))


def cache_rows(max_len, seq_len, least=1):
  """max_len of prefill / new_cache as (cache rows per sequence, default cfg.seq_len; do they hold ``least`` rows and fit cfg.seq_len?)."""
  rows = seq_len if max_len is None else int(max_len)
  return rows, least <= rows <= seq_len


def last_rows(y, B, T, lens):
  """Rows lens[b] - 1 of every sequence of y [B*T, d] -> [B, d]: what a right-padded prompt is continued from (NOT the padded last row)."""
  idx = torch.arange(B, device=y.device) * T + (lens.to(device=y.device, dtype=torch.int64) - 1)
  return y.index_select(0, idx)


def generate_loop(first, step, max_new_tokens, eos_id=None, all_done=None, check_every=FINISH_CHECK_EVERY):
  """The token loop.  ``first`` = (tokens int64 [B], logprob fp32 [B]) from the prefill; ``step(tokens) -> (tokens, logprob)`` is one
  decode step.  Returns (tokens [B, N], logprobs [B, N]).  After a sequence has emitted eos_id its later tokens are eos_id with
  log-probability 0 (its steps still run: the batch stays rectangular).  Nothing is read back per token; ``all_done(done)`` - the one
  device-to-host read - runs at most once every ``check_every`` steps and ends the loop early."""
  tok, lp = first
  toks, lps = [tok], [lp]
  done = (tok == eos_id) if eos_id is not None else None
  if all_done is None:
    all_done = lambda d: bool(d.all())  # noqa: E731
  for i in range(1, int(max_new_tokens)):
    if done is not None and i % check_every == 0 and all_done(done):
      rest = int(max_new_tokens) - i
      toks += [torch.full_like(tok, eos_id)] * rest
      lps += [torch.zeros_like(lp)] * rest
      break
    tok, lp = step(tok)
    if done is not None:
      tok = torch.where(done, torch.full_like(tok, eos_id), tok)
      lp = torch.where(done, torch.zeros_like(lp), lp)
      done = done | (tok == eos_id)
    toks.append(tok)
    lps.append(lp)
  return torch.stack(toks, dim=1), torch.stack(lps, dim=1)


def sampled(sample, logits):
  """(tokens int64 [B], log p(tokens) fp32 [B]) from the caller's sampler on fp32 logits [B, V]."""
  lf = logits.float()
  tok = sample(lf)
  if not isinstance(tok, torch.Tensor) or tok.dtype != torch.int64 or tuple(tok.shape) != (lf.shape[0],):
    raise TypeError('generate: sample(logits fp32 [B, V]) must return an int64 [B] tensor')
  tok = tok.to(lf.device)
  return tok, torch.log_softmax(lf, dim=-1).gather(1, tok[:, None])[:, 0]


def check_sampling(temperature=None, top_k=None, top_p=None, sample=None, seed=None):
  """The sampling arguments of generate, normalised: None when the call is greedy or goes through the caller's ``sample``, else
  (temperature, top_k, top_p) for ops.sample_logits.  top_k None is 0 (off), top_p None is 1 (off); temperature None or 0 with neither
  filter is greedy, temperature None with a filter is 1.  Refused with ValueError: ``sample`` together with any of the other four, a
  negative or non-finite temperature, temperature 0 together with a filter (that is greedy: say so by leaving the filters out), top_k < 0,
  top_p outside (0, 1]."""
  if sample is not None:
    given = [n for n, v in (('temperature', temperature), ('top_k', top_k), ('top_p', top_p), ('seed', seed)) if v is not None]
    if given:
      raise ValueError(f'generate: sample= is the caller\'s own sampler; it cannot be combined with {", ".join(given)}')
    return None
  k = 0 if top_k is None else int(top_k)
  p = 1.0 if top_p is None else float(top_p)
  if k < 0:
    raise ValueError(f'generate: top_k must be >= 0 (0 or None = off), got {top_k}')
  if not (0.0 < p <= 1.0):
    raise ValueError(f'generate: top_p must be in (0, 1] (1 or None = off), got {top_p}')
  t = None if temperature is None else float(temperature)
  if t is not None and (not math.isfinite(t) or t < 0.0):
    raise ValueError(f'generate: temperature must be finite and >= 0, got {temperature}')
  filtered = k > 0 or p < 1.0
  if t is None or t == 0.0:
    if not filtered:
      return None  # greedy: the fused prediction head, no logits
    if t is not None:
      raise ValueError('generate: temperature 0 is greedy decoding, which top_k / top_p cannot change: leave them out, or give a positive temperature')
    t = 1.0
  return t, k, p


def draw_uniforms(max_new_tokens, B, device, seed=None):
  """u fp32 [max_new_tokens, B] on ``device``, drawn once per generate call: step n uses row n.  ``seed`` seeds a torch.Generator of
  that device (the same seed gives the same bits); None draws from torch's default generator."""
  gen = None
  if seed is not None:
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
  return torch.rand((int(max_new_tokens), int(B)), generator=gen, dtype=torch.float32, device=device)


def sampling_pick(u, temperature, top_k, top_p, sampler=None):
  """pick(logits bf16 [B, V]) -> (tokens, logprob) for generate_loop: its n-th call samples with row n of u, through ops.sample_logits
  (``sampler`` stands in for it in the host tests)."""
  sampler = ops.sample_logits if sampler is None else sampler
  rows = iter(u)

  def pick(logits):
    r = sampler(logits, next(rows), temperature, top_k, top_p)
    return r[0], r[1]
  return pick


# ---- speculative decoding ---------------------------------------------------------------------------------------
MAX_DRAFT = 31  # a chunk of n_draft + 1 <= 32 rows is one wave's queries in attn_extend_kernel; plm_spec_verify_bf16 holds the same limit


def check_speculative(T, max_new_tokens, n_draft, cfg, draft_cfg, device=None, draft_device=None, temperature=None, top_k=None, top_p=None,
                      seed=None, sample=None):
  """The refusals of generate_speculative that need no GPU.  cfg / draft_cfg: the two models' ModelConfig.  Returns (cache rows per
  sequence - the same for both models -, check_sampling's normalised (temperature, top_k, top_p) or None for greedy).  A round may write
  n_draft + 1 rows past the last token a sequence keeps, hence the longer cache."""
  if sample is not None:
    raise ValueError('generate_speculative: sample= callables are not supported (the acceptance rule needs both models\' distributions on the '
                     'device): use temperature / top_k / top_p, or generate()')
  if isinstance(n_draft, bool) or not isinstance(n_draft, int):
    raise TypeError(f'generate_speculative: n_draft must be an int, got {type(n_draft).__name__}')
  if n_draft < 1 or n_draft > MAX_DRAFT:
    raise ValueError(f'generate_speculative: n_draft must be in [1, {MAX_DRAFT}], got {n_draft}')
  if draft_cfg.vocab_size != cfg.vocab_size:
    raise ValueError(f'generate_speculative: the draft\'s vocab_size {draft_cfg.vocab_size} is not the target\'s {cfg.vocab_size}')
  if device is not None and draft_device is not None and torch.device(device) != torch.device(draft_device):
    raise ValueError(f'generate_speculative: the draft is on {draft_device}, the target on {device}')
  need = _check_new_tokens('generate_speculative', T, max_new_tokens, n_draft + 1, f' + n_draft {n_draft} + 1',
                           [("the target's ", cfg.seq_len), ("the draft's ", draft_cfg.seq_len)])
  return need, check_sampling(temperature, top_k, top_p, None, seed)


def greedy_accept(draft_tok, target_pred, n_prop=None):
  """Greedy acceptance: draft_tok int64 [B, k], target_pred int64 [B, k + 1] (row r: the target's prediction after the round's first r + 1
  tokens).  Returns (n_accept int32 [B] = the number of leading draft tokens the target predicts too, next_token int64 [B] = the target's
  prediction at the first mismatch, or at row k).  n_prop int [B]: only the first n_prop[b] columns of sequence b hold a proposal - a
  column at or beyond it never counts as a match, whatever it holds (None: all k do).  Integer ops only, any device."""
  k = draft_tok.shape[1]
  match = draft_tok == target_pred[:, :k]
  if n_prop is not None:
    match = match & (torch.arange(k, device=draft_tok.device)[None, :] < n_prop[:, None])
  n = match.to(torch.int32).cumprod(dim=1).sum(dim=1)
  return n.to(torch.int32), target_pred.gather(1, n.to(torch.int64)[:, None])[:, 0]


def commit_round(out_tok, out_lp, count, done, draft_tok, n_accept, next_tok, logp, eos_id=None):
  """The bookkeeping of one round, plain tensor ops on any device.  out_tok int64 [B, N] / out_lp fp32 [B, N] are updated in place;
  count int [B] (tokens emitted so far) and done bool [B] are not.  The round offers sequence b the tokens draft_tok[b, :n_accept[b]]
  followed by next_tok[b], with log-probabilities logp[b, :n_accept[b] + 1]; a live sequence takes them at columns count[b] .., cut at N
  and after the first eos_id, a finished one takes nothing.  A sequence that has emitted eos_id holds eos_id with log-probability 0 from
  there on, as generate_loop leaves it.  Returns (count, done, moved): the new counts and flags, and moved int32 [B] = the number of tokens
  each sequence took - how far its caches move."""
  B, N = out_tok.shape
  k = draft_tok.shape[1]
  dev = out_tok.device
  j = torch.arange(k + 1, device=dev)[None, :]
  na = n_accept.to(torch.int64)[:, None]
  cand = torch.where(j < na, torch.nn.functional.pad(draft_tok, (0, 1)), next_tok[:, None])
  m = torch.minimum(na[:, 0] + 1, N - count.to(torch.int64))
  m = torch.where(done, torch.zeros_like(m), m)
  if eos_id is not None:  # cut after the first eos_id among the tokens taken
    is_eos = (cand == eos_id) & (j < m[:, None])
    hit = is_eos.any(dim=1)
    m = torch.where(hit, is_eos.to(torch.int32).argmax(dim=1) + 1, m)
  pos = torch.arange(N, device=dev)[None, :] - count.to(torch.int64)[:, None]  # column n of the outputs is round entry pos[b, n]
  take = (pos >= 0) & (pos < m[:, None])
  src = pos.clamp(0, k)
  out_tok.copy_(torch.where(take, cand.gather(1, src), out_tok))
  out_lp.copy_(torch.where(take, logp.gather(1, src), out_lp))
  new_count = count + m.to(count.dtype)
  new_done = done | (new_count >= N)
  if eos_id is not None:
    new_done = new_done | hit
    tail = new_done[:, None] & (pos >= m[:, None])  # nothing for a sequence that filled up: it has no column left
    out_tok.masked_fill_(tail, eos_id)
    out_lp.masked_fill_(tail, 0.0)
  return new_count, new_done, m.to(torch.int32)


def speculative_loop(first, draft_round, target_round, accept, max_new_tokens, n_draft, eos_id=None, advance=None, all_done=None,
                     drafted_in_round=None):
  """The round loop of speculative decoding over callables (tests/test_spec_host.py runs it on the CPU with fake models).
    first                                       (tokens int64 [B], logprob fp32 [B]) of the target's prefill
    draft_round(last, carry_tok, carry, live)   -> (draft_tok int64 [B, k], whatever accept needs of the draft).  last [B]: every
                                                sequence's newest token; carry bool [B]: the draft has not seen carry_tok [B] yet (the
                                                last draft token of a round that accepted all k), which then precedes ``last``
    target_round(last, draft_tok, live)         -> whatever accept needs of the target's k + 1 chunk rows
    accept(draft_tok, draft_out, target_out)    -> (n_accept [B], next_token [B], logprob [B, k + 1])
    advance(moved, live)                        moves the caches: moved int32 [B] from commit_round (0 for a finished sequence); a live
                                                sequence's draft cache keeps min(moved, k) of the round's rows
    drafted_in_round()                          -> int [B]: the proposals the round just run made per sequence, for a draft that does not
                                                always make k of them (called after accept; None: k for every live sequence)
  Returns (tokens [B, N], logprobs [B, N], stats) with stats = dict(rounds, drafted int64 [B], accepted int64 [B]) over the rounds a
  sequence was live in.  A round emits at least one token per live sequence, so there are at most N - 1 rounds.  ``all_done(done)`` - the
  one device-to-host read, one int32 per round - ends the loop."""
  tok, lp = first
  N, k = int(max_new_tokens), int(n_draft)
  B, dev = tok.shape[0], tok.device
  out_tok = torch.zeros((B, N), dtype=torch.int64, device=dev)
  out_lp = torch.zeros((B, N), dtype=torch.float32, device=dev)
  out_tok[:, 0] = tok
  out_lp[:, 0] = lp
  count = torch.ones((B,), dtype=torch.int32, device=dev)
  done = torch.full((B,), N <= 1, dtype=torch.bool, device=dev)
  if eos_id is not None:
    done = done | (tok == eos_id)
    out_tok[:, 1:] = torch.where(done[:, None], torch.full_like(out_tok[:, 1:], eos_id), out_tok[:, 1:])
  if all_done is None:
    all_done = lambda d: bool(d.all())  # noqa: E731
  last, carry_tok = tok, tok
  carry = torch.zeros((B,), dtype=torch.bool, device=dev)
  drafted = torch.zeros((B,), dtype=torch.int64, device=dev)
  accepted = torch.zeros((B,), dtype=torch.int64, device=dev)
  rounds = 0
  while rounds < N - 1 and not all_done(done):
    live = ~done
    draft_tok, draft_out = draft_round(last, carry_tok, carry, live)
    n_accept, next_tok, logp = accept(draft_tok, draft_out, target_round(last, draft_tok, live))
    count, done, moved = commit_round(out_tok, out_lp, count, done, draft_tok, n_accept, next_tok, logp, eos_id)
    if advance is not None:
      advance(moved, live)
    carry = live & (moved == k + 1)
    carry_tok = draft_tok[:, k - 1]
    last = torch.where(live, next_tok, last)
    drafted += live.to(torch.int64) * (k if drafted_in_round is None else drafted_in_round().to(torch.int64))
    accepted += torch.where(live, n_accept.to(torch.int64), torch.zeros_like(accepted))
    rounds += 1
  return out_tok, out_lp, dict(rounds=rounds, drafted=drafted, accepted=accepted)


def uniforms_per_round(k):
  """Uniforms a round uses per sequence: k draft draws, k + 1 draws of the target's sampler, k acceptance tests, one residual draw."""
  return 3 * k + 2


def speculative_uniforms(max_new_tokens, n_draft, B, device, seed=None):
  """All uniforms of one generate_speculative call, drawn once through draw_uniforms: fp32 [1 + (N - 1) * (3k + 2), B].  Row 0 draws the
  first token; round i owns the next 3k + 2 rows (``round_uniforms``).  Every entry is used at most once, so the four roles are
  independent of one another."""
  return draw_uniforms(1 + (int(max_new_tokens) - 1) * uniforms_per_round(int(n_draft)), B, device, seed)


def round_uniforms(u, i, n_draft):
  """Round i's rows of ``speculative_uniforms``: (draft draws [k, B], target sampler's [k + 1, B], acceptance [k, B], residual [B])."""
  k = int(n_draft)
  r = u[1 + i * uniforms_per_round(k):1 + (i + 1) * uniforms_per_round(k)]
  return r[:k], r[k:2 * k + 1], r[2 * k + 1:3 * k + 1], r[3 * k + 1]


class _SpecSession:
  """One generate_speculative call between its rounds: the two models and their caches, the lengths the caches are set to after every
  round, the round counter and - when the call samples (``sampling`` = check_sampling's triple, else None) - its uniforms ``u`` and the
  draft's logits of the current round.  The four methods are the callables ``speculative_loop`` documents."""

  def __init__(self, target, draft, tcache, dcache, k, sampling, u):
    self.target, self.draft, self.tcache, self.dcache = target, draft, tcache, dcache
    self.k, self.sampling, self.sampled, self.u, self.round = k, sampling, sampling is not None, u, 0
    # the lengths the caches are set to after every round: both hold the sequence up to, not including, its newest token - the draft one
    # row less while it has not seen the last draft token of a fully accepted round
    self.tlen, self.dlen = tcache.lens.clone(), dcache.lens.clone()
    self.qbuf = torch.empty((k, tcache.B, target.cfg.vocab_size), dtype=torch.bfloat16, device=u.device) if self.sampled else None

  def draft_round(self, last, carry_tok, carry, live):
    sampled = self.sampled
    ur = round_uniforms(self.u, self.round, self.k)[0] if sampled else None
    toks, cuts = [], []
    for i in range(self.k):
      if i == 0:  # [carry_tok, last] where the draft still lacks carry_tok, else [last, -]; a finished sequence appends nothing
        pair = torch.stack([torch.where(carry, carry_tok, last), last], dim=1)
        out = self.draft.extend(pair, self.dcache, token_lens=(live.to(torch.int32) * (1 + carry.to(torch.int32))), logits=sampled)
      else:
        out = self.draft.decode_step(toks[-1], self.dcache, logits=sampled)
      if sampled:
        self.qbuf[i].copy_(out)
        sq = ops.sample_logits(self.qbuf[i], ur[i], *self.sampling, want_stats=True)
        toks.append(sq.tokens)
        cuts.append(sq.cutoff)
      else:
        toks.append(out.tokens)
    return torch.stack(toks, dim=1), (torch.stack(toks, dim=0), torch.stack(cuts, dim=0)) if sampled else None

  def target_round(self, last, draft_tok, live):
    chunk = torch.cat([last[:, None], draft_tok], dim=1)
    return self.target.extend(chunk, self.tcache, token_lens=live.to(torch.int32) * (self.k + 1), logits=self.sampled, all_rows=True)

  def accept(self, draft_tok, draft_out, out):
    if not self.sampled:
      return greedy_accept(draft_tok, out.tokens) + (out.logprob,)
    _, ut, ua, ures = round_uniforms(self.u, self.round, self.k)
    V = out.shape[-1]
    rows = out.view(-1, V)  # [B * (k + 1), V]
    st = ops.sample_logits(rows, ut.t().reshape(-1), *self.sampling, want_stats=True)  # row b * (k + 1) + r draws with ut[r, b]
    return tuple(ops.spec_verify(rows, self.qbuf.view(-1, V), draft_out[0], st.cutoff, draft_out[1].reshape(-1), st.tokens, ua, ures,
                                 self.sampling[0]))

  def advance(self, moved, live):
    self.dlen.copy_(torch.where(live, self.tlen + moved.clamp(max=self.k), self.dlen))
    self.tlen.add_(moved)
    self.tcache.set_lens(self.tlen)
    self.dcache.set_lens(self.dlen)
    self.round += 1


# ---- draft-free speculative decoding: n-gram lookup drafts -----------------------------------------------------------
MAX_NGRAM = 16  # plm_lookup_draft_i64 compares at most this many tokens of a match


def check_lookup(T, max_new_tokens, n_draft, ngram, cfg, temperature=None, top_k=None, top_p=None, seed=None):
  """The refusals of generate_lookup that need no GPU.  Returns (cache rows per sequence, check_sampling's normalised (temperature, top_k,
  top_p) or None for greedy).  A round may write n_draft + 1 rows past the last token a sequence keeps, hence the longer cache."""
  if isinstance(n_draft, bool) or not isinstance(n_draft, int):
    raise TypeError(f'generate_lookup: n_draft must be an int, got {type(n_draft).__name__}')
  if n_draft < 1 or n_draft > MAX_DRAFT:
    raise ValueError(f'generate_lookup: n_draft must be in [1, {MAX_DRAFT}], got {n_draft}')
  if not isinstance(ngram, (tuple, list)) or len(ngram) != 2 or any(isinstance(g, bool) or not isinstance(g, int) for g in ngram):
    raise TypeError(f'generate_lookup: ngram must be two ints (g_min, g_max), got {ngram!r}')
  if not 1 <= ngram[0] <= ngram[1] <= MAX_NGRAM:
    raise ValueError(f'generate_lookup: ngram must satisfy 1 <= g_min <= g_max <= {MAX_NGRAM}, got {tuple(ngram)}')
  need = _check_new_tokens('generate_lookup', T, max_new_tokens, n_draft + 1, f' + n_draft {n_draft} + 1', [('', cfg.seq_len)])
  return need, check_sampling(temperature, top_k, top_p, None, seed)


def lookup_uniforms_per_round(k):
  """Uniforms a lookup round uses per sequence: k + 1 draws of the sampler, k acceptance tests, one residual draw (the draft draws none)."""
  return 2 * k + 2


def lookup_uniforms(max_new_tokens, n_draft, B, device, seed=None):
  """All uniforms of one sampled generate_lookup call, drawn once through draw_uniforms: fp32 [1 + (N - 1) * (2k + 2), B].  Row 0 draws
  the first token; round i owns the next 2k + 2 rows (``lookup_round_uniforms``).  Every entry is used at most once."""
  return draw_uniforms(1 + (int(max_new_tokens) - 1) * lookup_uniforms_per_round(int(n_draft)), B, device, seed)


def lookup_round_uniforms(u, i, n_draft):
  """Round i's rows of ``lookup_uniforms``: (the sampler's [k + 1, B], acceptance [k, B], residual [B])."""
  k = int(n_draft)
  r = u[1 + i * lookup_uniforms_per_round(k):1 + (i + 1) * lookup_uniforms_per_round(k)]
  return r[:k + 1], r[k + 1:2 * k + 1], r[2 * k + 1]


class _LookupSession:
  """One generate_lookup call between its rounds: the model and its cache, the length the cache is set to after every round, every
  sequence's token history (prompt and emitted tokens, the newest included) with the tokens the next ops.lookup_draft launch appends to
  it, the round counter and - when the call samples (``sampling`` = check_sampling's triple, else None) - its uniforms ``u``.  The methods
  are the callables ``speculative_loop`` documents; there is no draft cache, so the loop's carry arguments are not used.  ``fused`` adds
  fused=True to the round's ``extend`` call and changes nothing else.  ``lookup``,
  ``sampler`` and ``verify`` stand in for ops.lookup_draft / ops.sample_logits / ops.spec_verify_lookup in the host tests."""

  def __init__(self, model, cache, prompt, first_tok, k, ngram, max_new_tokens, sampling, u, lookup=None, sampler=None, verify=None, fused=False):
    self.model, self.cache, self.k, self.ngram = model, cache, k, tuple(ngram)
    self.extend_kw = dict(fused=True) if fused else {}  # what target_round adds to its extend call (generate_lookup_fused)
    self.sampling, self.sampled, self.u, self.round = sampling, sampling is not None, u, 0
    self.lookup = ops.lookup_draft if lookup is None else lookup
    self.sampler = ops.sample_logits if sampler is None else sampler
    self.verify = ops.spec_verify_lookup if verify is None else verify
    B, T = prompt.shape
    self.tlen = cache.lens.clone()  # the cache holds the sequence up to, not including, its newest token
    # a sequence emits at most max_new_tokens tokens, so T + max_new_tokens columns hold every history; columns beyond hlen are never read
    self.hist = torch.zeros((B, T + int(max_new_tokens)), dtype=torch.int64, device=prompt.device)
    self.hist[:, :T] = prompt
    self.hlen = cache.lens.clone()
    self.status = torch.zeros((1,), dtype=torch.int32, device=prompt.device)
    self.add, self.n_add = first_tok[:, None].contiguous(), None  # round 0 appends the first token
    self.n_prop = self.n_accept = self.next_tok = None

  def draft_round(self, last, carry_tok, carry, live):
    d = self.lookup(self.hist, self.hlen, self.add, self.n_add, k=self.k, ngram=self.ngram, status=self.status)
    self.n_prop = d.n_prop
    return d.draft_tokens, None

  def target_round(self, last, draft_tok, live):
    chunk = torch.cat([last[:, None], draft_tok], dim=1)
    return self.model.extend(chunk, self.cache, token_lens=live.to(torch.int32) * (self.n_prop + 1), logits=self.sampled, all_rows=True,
                             **self.extend_kw)

  def accept(self, draft_tok, draft_out, out):
    if not self.sampled:
      res = greedy_accept(draft_tok, out.tokens, self.n_prop) + (out.logprob,)
    else:
      ut, ua, ures = lookup_round_uniforms(self.u, self.round, self.k)
      rows = out.view(-1, out.shape[-1])  # [B * (k + 1), V]
      st = self.sampler(rows, ut.t().reshape(-1), *self.sampling, want_stats=True)  # row b * (k + 1) + r draws with ut[r, b]
      res = tuple(self.verify(rows, draft_tok, self.n_prop, st.cutoff, st.tokens, ua, ures, self.sampling[0]))
    self.n_accept, self.next_tok = res[0], res[1]
    self.draft_tok = draft_tok
    return res

  def drafted(self):
    return self.n_prop

  def advance(self, moved, live):
    self.tlen.add_(moved)
    self.cache.set_lens(self.tlen)
    # what the round committed, for the next launch to append: the accepted proposals, then the round's own token; `moved` of them
    j = torch.arange(self.k + 1, device=moved.device)[None, :]
    self.add = torch.where(j < self.n_accept.to(torch.int64)[:, None], torch.nn.functional.pad(self.draft_tok, (0, 1)), self.next_tok[:, None])
    self.n_add = moved
    self.round += 1

  def check(self):
    """Raises if a round's tokens did not fit the history (reads the device flag, so it waits for the GPU)."""
    if int(self.status.item()) != 0:
      raise RuntimeError('generate_lookup: a round\'s tokens did not fit the token history: they were not stored')


# ---- beam search ---------------------------------------------------------------------------------------------------
def check_beam(num_beams, num_return=1, length_penalty=1.0, vocab_size=None, eos_id=None, pad_id=None, temperature=None, top_k=None, top_p=None,
               seed=None, sample=None):
  """The refusals of generate_beam / beam_loop that need no GPU; returns (G, R, length_penalty, pad_id) - pad_id defaults to eos_id, then 0."""
  who = 'generate_beam'
  given = [n for n, v in (('temperature', temperature), ('top_k', top_k), ('top_p', top_p), ('seed', seed), ('sample', sample)) if v is not None]
  if given:
    raise ValueError(f'{who}: beam search is deterministic and takes no sampling arguments ({", ".join(given)}): use generate_samples to sample')
  for name, v in (('num_beams', num_beams), ('num_return', num_return)):
    if isinstance(v, bool) or not isinstance(v, int):
      raise TypeError(f'{who}: {name} must be an int, got {type(v).__name__}')
  if not 1 <= num_beams <= ops.BEAM_MAX:
    raise ValueError(f'{who}: num_beams must be in [1, {ops.BEAM_MAX}] (the beams of a prompt are one MFMA tile of queries), got {num_beams}')
  if not 1 <= num_return <= num_beams:
    raise ValueError(f'{who}: num_return must be in [1, num_beams={num_beams}], got {num_return}')
  if vocab_size is not None and vocab_size < 2 * num_beams:
    raise ValueError(f'{who}: a vocabulary of {vocab_size} is too small for {num_beams} beams (a step keeps 2 * num_beams candidates per prompt)')
  lp = float(length_penalty)
  if not math.isfinite(lp):
    raise ValueError(f'{who}: length_penalty must be finite, got {length_penalty}')
  for name, v in (('eos_id', eos_id), ('pad_id', pad_id)):
    if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0 or (vocab_size is not None and v >= vocab_size)):
      raise ValueError(f'{who}: {name} must be a token id, got {v!r}')
  return num_beams, num_return, lp, (pad_id if pad_id is not None else (eos_id if eos_id is not None else 0))


def beam_loop(first_logits, step, max_new_tokens, num_beams, num_return=1, length_penalty=1.0, early_stopping=False, eos_id=None, pad_id=None,
              buffers=None, check_every=FINISH_CHECK_EVERY):
  """The beam-search loop over a callable.  first_logits bf16 [P, V]: the prompts' last-row logits; ``step(tokens int64 [P*G]) -> logits
  bf16 [P*G, V]`` is one decode step of all beams, row p*G + n = live beam n of prompt p.  Every token costs one ops.beam_select and one
  ops.beam_advance on ``buffers`` (ops.BeamBuffers; made here when None - a ``step`` that attends through ``buffers.anc`` brings its own);
  ``buffers.done`` - the one device-to-host read - is looked at once every ``check_every`` steps and ends the loop when every prompt is
  done.  Returns ops.beam_finalize's (tokens int64 [P, R, N], lengths int32 [P, R], scores fp32 [P, R])."""
  N = int(max_new_tokens)
  if N < 1:
    raise ValueError(f'generate_beam: max_new_tokens must be at least 1, got {max_new_tokens}')
  G, R, lp, pad = check_beam(num_beams, num_return, length_penalty, first_logits.shape[-1], eos_id, pad_id)
  buf = ops.BeamBuffers(first_logits.shape[0], G, N, first_logits.device) if buffers is None else buffers
  if (buf.P, buf.G, buf.N, buf.steps) != (first_logits.shape[0], G, N, 0):
    raise ValueError(f'generate_beam: the buffers (P={buf.P}, G={buf.G}, N={buf.N}, steps={buf.steps}) are not fresh ones for P={first_logits.shape[0]}, '
                     f'G={G}, N={N}')
  tok = ops.beam_advance(buf, ops.beam_select(first_logits, buf.score0, G, 1), eos_id, lp, early_stopping)
  for t in range(1, N):
    if t % check_every == 0 and bool(buf.done.all()):
      break
    tok = ops.beam_advance(buf, ops.beam_select(step(tok), buf.score, G, G), eos_id, lp, early_stopping)
  return ops.beam_finalize(buf, R, lp, eos_id, pad)


# ---- tree verification for lookup decoding -------------------------------------------------------------------------------
def refuse_tree_cache(what, cache):
  """The cache refusals of the tree methods: a SharedPrefixCache (TypeError) and an FP8 cache (ValueError) - the tree kernels read and move
  bf16 rows."""
  refuse_shared(what, cache)
  refuse_paged(what, cache)
  if getattr(cache, 'kv_dtype', 'bf16') != 'bf16':
    raise ValueError(f"Transformer.{what}: a {cache.kv_dtype!r} cache has no tree path (the tree kernels read and move bf16 rows): prefill with "
                     "kv_dtype='bf16'")


def check_tree_rows(who, n):
  if not 1 <= n <= ops.TREE_MAX_ROWS:
    raise ValueError(f'{who}: a tree chunk holds 1 to {ops.TREE_MAX_ROWS} rows per sequence (one bit of the ancestor mask each), got {n}')


def tree_rows(n_draft, n_branch, max_rows=None):
  """Rows of generate_lookup_tree's chunk: the root and up to n_branch continuations of n_draft tokens, at most ops.TREE_MAX_ROWS and at
  most max_rows (the caller's cap, e.g. 32 // B to fit the fused path); the trie is filled most recent match first."""
  return min(1 + int(n_draft) * int(n_branch), ops.TREE_MAX_ROWS if max_rows is None else int(max_rows))


def check_lookup_tree(T, max_new_tokens, n_draft, n_branch, ngram, cfg, max_rows=None):
  """The refusals of generate_lookup_tree that need no GPU; returns (cache rows per sequence, rows per chunk).  A round may write a whole
  chunk past the last token a sequence keeps, hence the longer cache."""
  who = 'generate_lookup_tree'
  for name, v in (('n_draft', n_draft), ('n_branch', n_branch)):
    if isinstance(v, bool) or not isinstance(v, int):
      raise TypeError(f'{who}: {name} must be an int, got {type(v).__name__}')
  if n_draft < 1 or n_draft > MAX_DRAFT:
    raise ValueError(f'{who}: n_draft must be in [1, {MAX_DRAFT}], got {n_draft}')
  if n_branch < 1 or n_branch > ops.TREE_MAX_BRANCH:
    raise ValueError(f'{who}: n_branch must be in [1, {ops.TREE_MAX_BRANCH}], got {n_branch}')
  if not isinstance(ngram, (tuple, list)) or len(ngram) != 2 or any(isinstance(g, bool) or not isinstance(g, int) for g in ngram):
    raise TypeError(f'{who}: ngram must be two ints (g_min, g_max), got {ngram!r}')
  if not 1 <= ngram[0] <= ngram[1] <= MAX_NGRAM:
    raise ValueError(f'{who}: ngram must satisfy 1 <= g_min <= g_max <= {MAX_NGRAM}, got {tuple(ngram)}')
  if max_rows is not None and (isinstance(max_rows, bool) or not isinstance(max_rows, int) or not 2 <= max_rows <= ops.TREE_MAX_ROWS):
    raise ValueError(f'{who}: max_rows must be an int in [2, {ops.TREE_MAX_ROWS}] (the root and at least one node), got {max_rows!r}')
  n = tree_rows(n_draft, n_branch, max_rows)
  return _check_new_tokens(who, T, max_new_tokens, n, f' + a chunk of {n} tree rows', [('', cfg.seq_len)]), n


class _TreeSession(_LookupSession):
  """_LookupSession whose draft is a trie (ops.lookup_draft_tree) verified by one ``extend_tree``: greedy only.  The loop's "draft tokens"
  are the ACCEPTED tokens in path order, which exist only after the verify step: draft_round hands the loop a buffer and accept has
  ops.tree_accept write into it, before commit_round reads it.  ``self.k`` = n - 1, the buffer's width; n_draft is the length of one
  continuation.  advance keeps the accepted path's cache rows (ops.kv_tree_commit) before the lengths move."""

  def __init__(self, model, cache, prompt, first_tok, n_draft, n_branch, n, ngram, max_new_tokens, fused=False):
    super().__init__(model, cache, prompt, first_tok, n - 1, ngram, max_new_tokens, None, None, fused=fused)
    self.n, self.n_draft, self.n_branch = n, n_draft, n_branch
    self.acc = torch.zeros((prompt.shape[0], n - 1), dtype=torch.int64, device=prompt.device)
    self.nodes = torch.zeros((prompt.shape[0],), dtype=torch.int64, device=prompt.device)  # rows verified, the roots included

  def draft_round(self, last, carry_tok, carry, live):
    self.tree = ops.lookup_draft_tree(self.hist, self.hlen, self.add, self.n_add, n=self.n, k=self.n_draft, n_branch=self.n_branch, ngram=self.ngram,
                                      status=self.status)
    self.tree.tokens[:, 0] = last  # the root: the history's newest token (a refused history has none to read)
    self.n_new = live.to(torch.int32) * self.tree.n_new.clamp(min=1)
    self.nodes += self.n_new
    return self.acc, None

  def target_round(self, last, draft_tok, live):
    return self.model.extend_tree(self.tree.tokens, self.tree.parent, self.cache, token_lens=self.n_new, **self.extend_kw)

  def accept(self, draft_tok, draft_out, out):
    a = ops.tree_accept(self.tree.tokens, self.tree.parent, out.tokens, out.logprob, n_new=self.n_new, tokens_out=draft_tok)
    self.n_accept, self.next_tok, self.path, self.draft_tok = a.n_accept, a.next_token, a.path, draft_tok
    return a.n_accept, a.next_token, a.logprob

  def drafted(self):
    return (self.n_new - 1).clamp(min=0)

  def advance(self, moved, live):
    ops.kv_tree_commit(self.cache.kv, self.tlen, self.path, self.n_accept, self.cache.n_heads)  # tlen: the lengths before the chunk
    super().advance(moved, live)


class Generation:
  """KV-cached generation, mixed into ``Transformer`` (DESIGN.md sections 12 to 16).  What it asks of its host class:
    attributes  cfg (the ModelConfig), n_layers, head_dim, lm_head (its weight tells the model's device)
    methods     _rope(device), trunk(x, attn_mask, cache), cached_layers(tokens, cache, attend), fused_layers(tokens, cache, rope,
                chunk=None | (lens0, n_new, n)), head(y, logits, shape); the middle three call refresh_shadows() themselves.  _rope
                keeps its underscore: tools and tests from before the mixin call it by that name."""

  @torch.compiler.disable
  def prefill(self, x, prompt_lens=None, max_len=None, logits=False, kv_dtype=None):
    """Run the prompt x int64 [B, T] through the trunk once and keep every layer's rotated k | v: returns (KVCache, HeadPrediction [B]) -
    the greedy next token of every sequence, its log-probability and the entropy, from row prompt_lens[b] - 1 (host integers; default T).
    Prompts are right-padded to a multiple of 4 (the attention kernels' granularity), which under a causal mask changes no earlier row;
    with prompt_lens shorter rows hold padding the cache never reads (lens = prompt_lens).  max_len: cache rows per sequence (default
    cfg.seq_len).  logits=True returns the bf16 [B, V] logits of those rows in
    place of the prediction.  kv_dtype: 'bf16' | 'fp8' (DESIGN.md section 20), None: cfg.kv_cache.  Runs under no_grad."""
    guard('prefill', x, self, rank2=True)
    kv_dtype = check_kv_dtype(self.cfg.kv_cache if kv_dtype is None else kv_dtype)
    B, T = x.shape
    lens = prompt_lens_list(prompt_lens, B, T)
    Tp = pad4(T)
    Tmax, fits = cache_rows(max_len, self.cfg.seq_len, least=Tp)
    if not fits:
      raise ValueError(f'prefill: the padded prompt ({Tp} rows) must fit max_len {Tmax}, and max_len cfg.seq_len {self.cfg.seq_len}')
    with torch.no_grad():
      if Tp != T:
        x = torch.nn.functional.pad(x, (0, Tp - T))
      cache = KVCache(self.n_layers, B, Tmax, self.cfg.n_heads, self.head_dim, x.device, kv_dtype)
      lens_dev = torch.tensor(lens, dtype=torch.int32).to(x.device)
      cache.set_lens(lens_dev)
      y, _, _ = self.trunk(x.contiguous(), None, cache)
      return cache, self.head(last_rows(y, B, Tp, lens_dev), logits, (B,))

  @torch.compiler.disable
  def decode_step(self, tokens, cache, logits=False, fused=False):
    """One token per sequence on top of ``cache``: tokens int64 [B] are appended at positions cache.lens (then lens += 1, on the device)
    and the HeadPrediction [B] of the NEXT token is returned - or, with logits=True, its bf16 logits [B, V].  The Block structure as it
    is (``cached_layers``), with ops.kv_append_rope / ops.attn_decode as the attention stage.  fused=True runs
    every layer as one library call over the skinny-M kernels (``fused_layers``: the same rounding points, other fp32 summation orders,
    so close to but not the bits of the default); it serves B <= ops.FUSED_DECODE_MAX_ROWS and raises ValueError otherwise."""
    if isinstance(cache, SharedPrefixCache):
      refuse_shared_mxfp8('decode_step', self)
    guard('decode_step', tokens, self)
    B = cache.B
    if tuple(tokens.shape) != (B,):
      raise ValueError(f'decode_step: tokens {tuple(tokens.shape)} do not match the cache\'s batch of {B}')
    if fused:
      check_fused('decode_step', B, self.cfg.dim)
    check_cache('decode_step', cache, self)
    nh = self.cfg.n_heads
    with torch.no_grad():
      rope = self._rope(tokens.device)
      cache.advance()  # pos = the appended token's position, lens = pos + 1: what this step's attention sees
      if fused:
        return self.head(self.fused_layers(tokens.contiguous(), cache, rope), logits, (B,))

      def attend(i, qkv):
        if isinstance(cache, PagedKVCache):  # the chunk append at n = 1 into the sequence's page, chunks of its own keys
          q, _ = ops.kv_paged_append_rope_rows(qkv, cache.pos, rope[0], rope[1], cache.kv[i], cache.table, nh, n_new=cache.live,
                                               status=cache.status)
          return ops.attn_decode_paged(q, cache.kv[i], cache.table, cache.lens, nh, Lcap=cache.lcap())
        if isinstance(cache, SharedPrefixCache):  # row pos of the suffix, rotated at rot0 + pos; prefix, then suffix
          q, _ = ops.kv_append_rope_at(qkv, cache.pos, cache.rot0, rope[0], rope[1], cache.kv[i], nh, status=cache.status)
          if cache.beam is not None:  # the suffix rows the beam's ancestor table names
            return ops.attn_decode_beam(q, cache.prefix.kv[i], cache.prefix.lens, cache.kv[i], cache.lens, cache.beam.anc, nh)
          return ops.attn_decode_shared(q, cache.prefix.kv[i], cache.prefix.lens, cache.kv[i], cache.lens, nh)
        if cache.kv_dtype == 'fp8':  # the decode step is the chunk append at n = 1
          q, _ = ops.kv8_append_rope_rows(qkv, cache.pos, rope[0], rope[1], cache.kv[i], nh, status=cache.status)
          return ops.attn_decode_kv8(q, cache.kv[i], cache.lens, nh)
        q, _ = ops.kv_append_rope(qkv, cache.pos, rope[0], rope[1], cache.kv[i], nh, status=cache.status)
        return ops.attn_decode(q, cache.kv[i], cache.lens, nh)
      return self.head(self.cached_layers(tokens.contiguous(), cache, attend), logits, (B,))

  def new_cache(self, B, max_len=None, kv_dtype=None):
    """An empty KVCache for B sequences (lens 0) of max_len rows each (default and at most cfg.seq_len): the start of a chunked prefill
    through ``extend``.  kv_dtype: 'bf16' | 'fp8', None: cfg.kv_cache."""
    refuse_mxfp8('new_cache', self)
    kv_dtype = check_kv_dtype(self.cfg.kv_cache if kv_dtype is None else kv_dtype)
    Tmax, fits = cache_rows(max_len, self.cfg.seq_len)
    if int(B) < 1 or not fits:
      raise ValueError(f'new_cache: need B >= 1 and 1 <= max_len <= cfg.seq_len {self.cfg.seq_len}, got B={B} max_len={Tmax}')
    device = self.lm_head.weight.device
    if device.type != 'cuda':
      raise RuntimeError('plainlm_amd.Transformer runs on MI355X only (the model is on CPU; there is no CPU fallback)')
    return KVCache(self.n_layers, int(B), Tmax, self.cfg.n_heads, self.head_dim, device, kv_dtype)

  @torch.compiler.disable
  def extend(self, tokens, cache, token_lens=None, logits=False, all_rows=False, fused=False):
    """Append a chunk of tokens to a live cache: tokens int64 [B, n], right-padded; sequence b's first token_lens[b] tokens are appended
    at positions cache.lens[b] .. (then lens += token_lens, on the device).  token_lens: None (all n), host integers in [0, n], or an
    int32 [B] device tensor (clamped to [0, n], never read back).  A new user turn on top of a cached conversation, one chunk of a long
    prompt's prefill (start from ``new_cache``), or k drafted tokens to verify (roll back with ``cache.set_lens``).
    Returns the HeadPrediction [B] of the token after each sequence's last appended row (row token_lens[b] - 1; a sequence that appended
    nothing gets row 0's, which means nothing) - with logits=True the bf16 logits [B, V] of that row; with all_rows=True the [B, n]
    predictions, or [B, n, V] logits, of every chunk row (rows at and beyond token_lens[b] belong to padding and mean nothing).
    The Block structure as decode_step runs it, through ops calls on the bf16 shadows at M = B * n: the same launches as one decode step,
    whatever n.  A chunk that does not fit the cache (or the RoPE table) stores nothing for that sequence and surfaces through
    ``cache.check()``.  Runs under no_grad.  fused=True runs every layer as one library call over the skinny-M
    kernels (``fused_layers`` with the chunk: the same rounding points, other fp32 summation orders, so close to but not the bits of the default);
    it serves B * n <= ops.FUSED_EXTEND_MAX_ROWS chunk rows and raises ValueError otherwise, before anything is launched."""
    refuse_shared('extend', cache)
    if isinstance(tokens, torch.Tensor) and (tokens.dim() != 2 or tokens.shape[0] != cache.B or tokens.shape[1] < 1):
      raise ValueError(f'extend: tokens {tuple(tokens.shape)} are not a [B, n] chunk for the cache\'s batch of {cache.B}')
    guard('extend', tokens, self)
    check_cache('extend', cache, self)
    B, n = tokens.shape
    if fused:
      check_fused_rows('extend', B, n, self.cfg.dim)
    nh = self.cfg.n_heads
    paged = isinstance(cache, PagedKVCache)
    with torch.no_grad():
      adv, n_new = chunk_lens(token_lens, B, n, tokens.device)
      rope = self._rope(tokens.device)
      lens0 = cache.lens  # the lengths before the chunk: what every layer's append and attention see; moved once, after the last layer
      if paged:  # the chunk's pages, on the host: by the token_lens the host knows, else by the chunk's width - a device token_lens is
        # never read back, so every live bound then moves by the full n and the pages it took beyond the real length stay until release
        host = token_lens is not None and not (isinstance(token_lens, torch.Tensor) and token_lens.is_cuda)
        cache.reserve([int(v) if live else 0 for v, live in zip(token_lens, cache._live)] if host else int(n))
        n_new = cache.live * n if n_new is None else n_new * cache.live  # an idle slot appends nothing, whatever its entry says
        adv = n_new

      append, attn = (ops.kv8_append_rope_rows, ops.attn_extend_kv8) if cache.kv_dtype == 'fp8' else (ops.kv_append_rope_rows, ops.attn_extend)

      def attend(i, qkv):
        if paged:
          q, _ = ops.kv_paged_append_rope_rows(qkv, lens0, rope[0], rope[1], cache.kv[i], cache.table, nh, n_new=n_new, status=cache.status)
          return ops.attn_extend_paged(q, cache.kv[i], cache.table, lens0, nh, n_new=n_new)  # Lcap = the table's width: S from the shape alone
        q, _ = append(qkv, lens0, rope[0], rope[1], cache.kv[i], nh, n_new=n_new, status=cache.status)
        return attn(q, cache.kv[i], lens0, nh, n_new=n_new)
      flat = tokens.reshape(-1).contiguous()
      y = self.fused_layers(flat, cache, rope, (lens0, n_new, n)) if fused else self.cached_layers(flat, cache, attend)
      cache.advance_by(adv)
      if all_rows:
        return self.head(y, logits, (B, n))
      if n_new is None:
        y = y.view(B, n, self.cfg.dim)[:, -1].contiguous()
      else:
        y = last_rows(y, B, n, n_new.clamp(min=1))
      return self.head(y, logits, (B,))

  # ---- the paged KV cache.  prefill / new_cache keep their pinned parameter lists: the paged forms are methods of
  # their own, as generate_fused is
  def new_page_pool(self, n_pages, kv_dtype=None):
    """A PagePool of n_pages pages of ops.KV_PAGE_ROWS token rows for this model, on its device.  bf16 pages only: kv_dtype 'fp8', a
    model with cfg.kv_cache = 'fp8' and an mxfp8 model raise ValueError."""
    refuse_paged_model('new_page_pool', self)
    device = self.lm_head.weight.device
    if device.type != 'cuda':
      raise RuntimeError('plainlm_amd.Transformer runs on MI355X only (the model is on CPU; there is no CPU fallback)')
    return PagePool(self.n_layers, n_pages, self.cfg.n_heads, self.head_dim, device, 'bf16' if kv_dtype is None else kv_dtype)

  def new_cache_paged(self, B, pool, max_len=None):
    """``new_cache`` over a PagePool: an empty PagedKVCache of B idle slots, max_len tokens each at most (default and at most
    cfg.seq_len).  It holds no page until a sequence is adopted or its lengths are set."""
    refuse_paged_model('new_cache_paged', self)
    Tmax, fits = cache_rows(max_len, self.cfg.seq_len)
    if int(B) < 1 or not fits:
      raise ValueError(f'new_cache_paged: need B >= 1 and 1 <= max_len <= cfg.seq_len {self.cfg.seq_len}, got B={B} max_len={Tmax}')
    cache = PagedKVCache(pool, int(B), Tmax)
    check_cache('new_cache_paged', cache, self)
    return cache

  @torch.compiler.disable
  def prefill_paged(self, x, pool, prompt_lens=None, max_len=None, logits=False):
    """``prefill`` into a PagedKVCache on ``pool``: the trunk as it is, every layer's rotated k | v rows scattered into the sequences'
    pages by one ops.kv_paged_store_rows launch.  Pages are taken for prompt_lens[b] tokens, not for the padded width; max_len (default
    cfg.seq_len) bounds what a sequence may grow to and costs nothing until it does.  Returns (PagedKVCache, HeadPrediction [B]) as
    ``prefill`` does.  A pool that is short of pages raises RuntimeError before anything is launched."""
    refuse_paged_model('prefill_paged', self)
    guard('prefill_paged', x, self, rank2=True)
    B, T = x.shape
    lens = prompt_lens_list(prompt_lens, B, T)
    Tp = pad4(T)
    Tmax, fits = cache_rows(max_len, self.cfg.seq_len, least=max(lens))
    if not fits or Tp > self.cfg.seq_len:
      raise ValueError(f'prefill_paged: the prompts ({max(lens)} tokens, {Tp} padded rows) must fit max_len {Tmax} and cfg.seq_len {self.cfg.seq_len}')
    cache = PagedKVCache(pool, B, Tmax)
    check_cache('prefill_paged', cache, self)
    with torch.no_grad():
      if Tp != T:
        x = torch.nn.functional.pad(x, (0, Tp - T))
      try:
        cache.set_lens(lens)
        y, _, _ = self.trunk(x.contiguous(), None, cache)
      except Exception:
        for b in range(B):
          cache.release(b)
        raise
      return cache, self.head(last_rows(y, B, Tp, cache.lens), logits, (B,))

  @torch.compiler.disable
  def prefill_prefix(self, tokens, pool):
    """A prompt prefix kept once on ``pool``: tokens int64 [n]; its first 64 * floor(n / 64) tokens are
    prefilled as a one-sequence paged cache whose pages the returned ``PagedPrefix`` holds, the tokens past the last whole page are
    its ``rest``.  Sequences start on it through ``PagedKVCache.admit_prefix`` / ``serve_shared``; ``release()`` it afterwards.  A
    prefix shorter than a page holds no page: rest is all of it."""
    refuse_paged_model('prefill_prefix', self)
    if not isinstance(tokens, torch.Tensor) or tokens.dtype != torch.int64 or tokens.dim() != 1:
      raise TypeError('Transformer.prefill_prefix: tokens must be a 1-D int64 tensor')
    if not isinstance(pool, PagePool):
      raise TypeError(f'Transformer.prefill_prefix: pool must be a PagePool, got {type(pool).__name__}')
    n = tokens.numel() // ops.KV_PAGE_ROWS * ops.KV_PAGE_ROWS
    if not n:
      return PagedPrefix(pool, [], tokens)
    cache, _ = self.prefill_paged(tokens[:n].view(1, -1), pool, max_len=n)
    cache.check()
    prefix = PagedPrefix(pool, cache.pages[0], tokens[n:])
    cache.pages[0] = []  # the prefix object is the pages' holder now
    return prefix

  @torch.compiler.disable
  def step_ragged(self, tokens, counts, cache, logits=False, all_rows=False, fused=False):
    """One ragged step on a PagedKVCache: tokens int64 [R], packed in slot order, of which slot b contributes
    counts[b] (host integers: 0 - the slot takes no part, and an idle slot must have 0; 1 - a decode row; or a chunk of a prompt).
    Slot b's rows are appended at positions cache.lens[b] .. and attended over its pages in one pass per layer (ops.kv_paged_append_rope_packed
    / ops.attn_ragged_paged as ``cached_layers``' attention stage); then lens += counts, on the device.  Pages are reserved on the host
    by the counts, before anything is launched.  Returns the HeadPrediction [B] of the token after each participating slot's last row
    (a slot with count 0 gets row 0's, which means nothing) - with logits=True the bf16 logits [B, V]; with all_rows=True the [R]
    predictions or [R, V] logits of every packed row.  fused=True runs every layer as one ops.ragged_layer_paged call and serves
    R <= ops.FUSED_EXTEND_MAX_ROWS rows, ValueError beyond; fused='wide'  one ops.ragged_layer_paged_wide call
    and R <= ops.FUSED_WIDE_MAX_ROWS rows, at every R, so that a row's bits do not depend on the step's width.  A cache with a live
    slot on shared prefix pages (``admit_prefix``) attends through ops.attn_ragged_paged_cascade - fused='wide':
    ops.ragged_layer_paged_wide_cascade; fused=True: ValueError.  A non-paged cache raises TypeError; an mxfp8 model, counts that do not sum
    to R and a count that does not fit max_len raise ValueError.  Runs under no_grad."""
    if not isinstance(cache, PagedKVCache):
      raise TypeError(f'Transformer.step_ragged: the cache must be a PagedKVCache, got {type(cache).__name__} (ragged steps run on pages only)')
    refuse_paged_model('step_ragged', self)
    R, counts = check_ragged(tokens, counts, cache, fused, self.cfg.dim)
    guard('step_ragged', tokens, self)
    check_cache('step_ragged', cache, self)
    nh = self.cfg.n_heads
    with torch.no_grad():
      rope = self._rope(tokens.device)
      lens0 = cache.lens  # the lengths before the step: what every layer's append and attention see; moved once, after the last layer
      cache.reserve(counts)
      adv, cascade = torch.tensor(counts, dtype=torch.int32), ()
      if any(cache.key_lo):  # a live slot stands on shared pages - every step of this cache attends by the cascade
        cu, row_seq, last_row, NT, key_lo, tile_rows, tile_seq, tile_keys, NTg, Pcap = ops.cascade_plan(counts, cache.key_lo, cache.group)
        cu, row_seq, last_row, adv, key_lo, tile_rows, tile_seq, tile_keys = cache.ship(cu, row_seq, last_row, adv, key_lo, tile_rows, tile_seq,
                                                                                         tile_keys)
        cascade = (key_lo, tile_rows.view(NTg, -1), tile_seq, tile_keys, NTg, Pcap)
      else:
        cu, row_seq, last_row, NT = ops.ragged_plan(counts)
        cu, row_seq, last_row, adv = cache.ship(cu, row_seq, last_row, adv)
      table, Lcap = cache.table, cache.lcap()

      def attend(i, qkv):
        q, _ = ops.kv_paged_append_rope_packed(qkv, lens0, cu, row_seq, rope[0], rope[1], cache.kv[i], table, nh, status=cache.status)
        if cascade:
          return ops.attn_ragged_paged_cascade(q, cache.kv[i], table, lens0, cascade[0], cu, row_seq, *cascade[1:4], nh, NT, *cascade[4:], Lcap=Lcap)
        return ops.attn_ragged_paged(q, cache.kv[i], table, lens0, cu, row_seq, nh, NT, Lcap=Lcap)
      flat = tokens.contiguous()
      # fused='wide': every step runs the wide kernels, the narrow ones included, so a sequence's bits never depend on what shared its step
      kind = 'wide' if fused == 'wide' else 'ragged'
      y = self.fused_layers(flat, cache, rope, (kind, lens0, cu, row_seq, NT) + cascade) if fused else self.cached_layers(flat, cache, attend)
      cache.advance_by(adv)
      if all_rows:
        return self.head(y, logits, (R,))
      return self.head(y.index_select(0, last_row.clamp(min=0).long()), logits, (cache.B,))  # the head runs on at most B rows

  def _serve_ragged(self, who, prompts, budget, total, pages, S, pool, eos_id, fused, C, prefix=None):
    """serve(prefill_chunk=C): every step is one ``step_ragged`` - a row per decoding slot plus, in slot order, up to C prompt rows of
    the admitted prompts.  A prompt whose last row is in the step gets its first token from it and decodes from the next."""
    N, dev = len(prompts), prompts[0].device
    with torch.no_grad():
      slots = self.new_cache_paged(S, pool, max(total))
      owner, fed, left, promised = [None] * S, [0] * S, [0] * S, [0] * S  # per slot: its prompt, the prompt rows fed, tokens and pages still due
      steps, where = [], [[] for _ in range(N)]  # where[i]: (step, slot) of sequence i's tokens
      cur = torch.zeros((S,), dtype=torch.int64, device=dev)
      done = torch.zeros((S,), dtype=torch.bool, device=dev)
      waiting = list(range(N))

      def leave(b):
        slots.release(b)
        owner[b], promised[b] = None, 0

      while waiting or any(o is not None for o in owner):
        for b in range(S):  # admission: in prompt order, into the lowest free slot, while the pool can hold the sequence to its end
          if owner[b] is None and waiting and pool.n_free - sum(promised) >= pages[waiting[0]]:
            i = waiting.pop(0)
            slots.admit(b) if prefix is None else slots.admit_prefix(b, prefix)  # serve_shared: on the shared pages
            owner[b], fed[b], left[b], promised[b] = i, 0, budget[i], pages[i]
            done[b] = False
        if all(o is None for o in owner):
          raise RuntimeError(f'{who}: the pool cannot hold prompt {waiting[0]} ({pages[waiting[0]]} pages, {pool.n_free} free)')
        counts, parts, room = [0] * S, [], C
        for b in range(S):  # a row per decoding slot; prompt rows in slot order while the step's C last
          if owner[b] is None:
            continue
          n = prompts[owner[b]].numel()
          if fed[b] == n:
            counts[b] = 1
            parts.append(cur[b:b + 1])
          elif room:
            counts[b] = min(n - fed[b], room)
            room -= counts[b]
            parts.append(prompts[owner[b]][fed[b]:fed[b] + counts[b]])
        held = [len(p) for p in slots.pages]
        cur = self.step_ragged(torch.cat(parts), counts, slots, fused=fused).tokens
        steps.append(cur)
        emits = [0] * S
        for b in range(S):
          if owner[b] is None:
            continue
          promised[b] -= len(slots.pages[b]) - held[b]
          n = prompts[owner[b]].numel()
          was_decoding = fed[b] == n
          fed[b] = min(n, fed[b] + counts[b]) if not was_decoding else n
          if was_decoding or (counts[b] and fed[b] == n):  # the slot's last row was a decode row or its prompt's last row: a token
            emits[b] = 1
            where[owner[b]].append((len(steps) - 1, b))
            left[b] -= 1
            if left[b] == 0:
              leave(b)
        if eos_id is not None:
          done = done | ((cur == eos_id) & slots.ship(torch.tensor(emits, dtype=torch.int32))[0].bool())
          if len(steps) % FINISH_CHECK_EVERY == 0:  # the one device-to-host read
            for b, d in enumerate(done.tolist()):
              if d and owner[b] is not None and fed[b] == prompts[owner[b]].numel():
                leave(b)
      slots.check()
      out, grid = [], torch.stack(steps)
      for i in range(N):
        st, sl = zip(*where[i])
        t = grid[torch.tensor(st, device=dev), torch.tensor(sl, device=dev)]
        if eos_id is not None:
          hit = (t == eos_id).nonzero()
          if hit.numel():
            t = t[:int(hit[0]) + 1]
        out.append(t)
      return out

  @torch.compiler.disable
  def serve(self, prompts, max_new_tokens, max_batch, pool=None, eos_id=None, fused=False, temperature=None, top_k=None, top_p=None,
            sample=None, seed=None, prefill_chunk=None):
    """Continuous batching: continue every prompt of ``prompts`` - a list of 1-D int64 token tensors of any
    lengths - by up to max_new_tokens tokens (an int, or one int per prompt), greedily, with at most max_batch sequences in flight.
    Returns a list of int64 tensors, the new tokens of every prompt, ended by eos_id when the sequence emitted it.  A waiting prompt is
    prefilled as a one-sequence PagedKVCache on ``pool`` (default: a pool made here, large enough for max_batch full sequences) and
    adopted into a free slot of the batch; a sequence that reaches its budget - or, as seen by the one device-to-host read every
    FINISH_CHECK_EVERY steps, emitted eos_id - is released and its slot refilled; idle slots step with length 0.  A prompt is admitted
    only when the pool can hold it to the end of its budget, so a step never runs out of pages; a pool too small for one sequence raises
    RuntimeError.  Greedy only: the on-device sampler's per-call uniforms do not map onto sequences that start at different steps, so
    sampling arguments raise ValueError.  fused=True runs the steps through ops.decode_layer_paged and serves max_batch <=
    ops.FUSED_DECODE_MAX_ROWS, ValueError beyond.  prefill_chunk=C (an int >= 1) feeds the prompts in chunks inside
    the decode steps in place of a prefill call per prompt: every step is one ``step_ragged`` of a row per decoding slot plus, in slot
    order, up to C prompt rows in total; a prompt whose last row is in the step gets its first token from it.  Admission, release, eos_id
    and the one read stay as they are; with fused=True it needs max_batch + C <= ops.FUSED_EXTEND_MAX_ROWS, ValueError otherwise.
    fused='wide'  runs every one of those steps through ops.ragged_layer_paged_wide and needs prefill_chunk and
    max_batch + C <= ops.FUSED_WIDE_MAX_ROWS; any other value of fused raises ValueError."""
    who = 'serve'
    refuse_paged_model(who, self)
    if any(a is not None for a in (temperature, top_k, top_p, sample, seed)):
      raise ValueError(f'{who}: greedy only - the sampler\'s uniforms are drawn per call for a fixed batch and do not map onto sequences that '
                       'join at different steps: drop temperature / top_k / top_p / sample / seed')
    check_fused_kind(who, fused)
    if fused == 'wide':
      if prefill_chunk is None:
        raise ValueError(f'{who}: fused=\'wide\' needs prefill_chunk (there is no wide decode-only path: fused=True serves those steps)')
      check_wide_dim(who, self.cfg.dim)
    elif fused:
      check_fused(who, int(max_batch), self.cfg.dim)
    if prefill_chunk is not None:
      prefill_chunk = check_prefill_chunk(who, prefill_chunk, max_batch, fused)
    prompts = list(prompts)
    if not prompts or int(max_batch) < 1:
      raise ValueError(f'{who}: need at least one prompt and max_batch >= 1')
    for t in prompts:
      if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 1:
        raise TypeError(f'{who}: every prompt must be a non-empty 1-D int64 tensor')
    guard(who, prompts[0], self, forward_only=True)
    N, S = len(prompts), int(max_batch)
    budget = [int(max_new_tokens)] * N if isinstance(max_new_tokens, int) else [int(v) for v in max_new_tokens]
    if len(budget) != N:
      raise ValueError(f'{who}: {len(budget)} budgets for {N} prompts')
    total = [_check_new_tokens(who, prompts[i].numel(), budget[i], 0, '', [('', self.cfg.seq_len)]) for i in range(N)]
    pages = [-(-t // ops.KV_PAGE_ROWS) for t in total]  # what sequence i holds at the end of its budget
    if pool is None:
      pool = self.new_page_pool(min(S, N) * max(pages))
    if max(pages) > pool.n_free:
      raise RuntimeError(f'{who}: the pool has {pool.n_free} free pages, one sequence needs {max(pages)}')
    if prefill_chunk is not None:  # prompts enter in chunks inside the decode steps
      return self._serve_ragged(who, prompts, budget, total, pages, S, pool, eos_id, fused, prefill_chunk)
    dev = prompts[0].device
    with torch.no_grad():
      slots = self.new_cache_paged(S, pool, max(total))
      owner, left, promised = [None] * S, [0] * S, [0] * S  # per slot: its prompt, the tokens it may still emit, the pages it may still take
      first, steps, where = [None] * N, [], [[] for _ in range(N)]  # where[i]: (step, slot) of sequence i's decode tokens
      cur = torch.zeros((S,), dtype=torch.int64, device=dev)
      done = torch.zeros((S,), dtype=torch.bool, device=dev)
      waiting = list(range(N))

      def leave(b):
        slots.release(b)
        owner[b], promised[b] = None, 0

      while waiting or any(o is not None for o in owner):
        for b in range(S):  # admission: in prompt order, into the lowest free slot, while the pool can hold the sequence to its end
          while owner[b] is None and waiting and pool.n_free - sum(promised) >= pages[waiting[0]]:
            i = waiting.pop(0)
            one, r = self.prefill_paged(prompts[i].view(1, -1), pool, max_len=total[i])
            first[i] = r.tokens
            if budget[i] == 1:
              one.release(0)
              continue
            slots.adopt(b, one, 0)
            owner[b], left[b], promised[b] = i, budget[i] - 1, pages[i] - len(slots.pages[b])
            cur[b:b + 1] = r.tokens
            done[b:b + 1] = (r.tokens == eos_id) if eos_id is not None else False
        if all(o is None for o in owner):
          if waiting:
            raise RuntimeError(f'{who}: the pool cannot hold prompt {waiting[0]} ({pages[waiting[0]]} pages, {pool.n_free} free)')
          break
        held = [len(p) for p in slots.pages]
        steps.append(self.decode_step(cur, slots, fused=fused).tokens)
        cur = steps[-1].clone()  # admission writes a new sequence's first token into its slot: not into the recorded step
        if eos_id is not None:
          done = done | (cur == eos_id)
        for b in range(S):
          if owner[b] is not None:
            promised[b] -= len(slots.pages[b]) - held[b]
            where[owner[b]].append((len(steps) - 1, b))
            left[b] -= 1
            if left[b] == 0:
              leave(b)
        if eos_id is not None and len(steps) % FINISH_CHECK_EVERY == 0:  # the one device-to-host read
          for b, d in enumerate(done.tolist()):
            if d and owner[b] is not None:
              leave(b)
      slots.check()
      out = []
      grid = torch.stack(steps) if steps else None
      for i in range(N):
        t = first[i]
        if where[i]:
          st, sl = zip(*where[i])
          t = torch.cat([t, grid[torch.tensor(st, device=dev), torch.tensor(sl, device=dev)]])
        if eos_id is not None:
          hit = (t == eos_id).nonzero()
          if hit.numel():
            t = t[:int(hit[0]) + 1]
        out.append(t)
      return out

  @torch.compiler.disable
  def serve_shared(self, prefix, prompts, max_new_tokens, max_batch, pool=None, eos_id=None, fused=False, prefill_chunk=128):
    """``serve(prefill_chunk=...)`` for prompts that start alike: every sequence is ``prefix`` - a 1-D int64
    tensor, prefilled here once and released at the end, or a ``PagedPrefix`` of ``prefill_prefix``, which stays the caller's - followed
    by its own prompt.  The prefix's whole pages are held once for the call and every sequence is admitted onto them
    (``admit_prefix``); its fed rows are prefix.rest, then its prompt, and every step attends through the cascade.  Admission
    promises a sequence's OWN pages only.  Returns serve's list of new tokens.  Greedy only; fused is False or 'wide' (the 32-row
    fused layer has no cascade variant: fused=True raises ValueError); an mxfp8 model and cfg.kv_cache = 'fp8' are refused as in serve."""
    who = 'serve_shared'
    refuse_paged_model(who, self)
    check_fused_kind(who, fused)
    if fused is True:
      raise ValueError(f'{who}: fused=True has no cascade variant: pass fused=\'wide\' or leave fused off')
    if fused == 'wide':
      check_wide_dim(who, self.cfg.dim)
    prefill_chunk = check_prefill_chunk(who, prefill_chunk, max_batch, fused)
    prompts = list(prompts)
    if not prompts or int(max_batch) < 1:
      raise ValueError(f'{who}: need at least one prompt and max_batch >= 1')
    for t in prompts:
      if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 1:
        raise TypeError(f'{who}: every prompt must be a non-empty 1-D int64 tensor')
    held = isinstance(prefix, PagedPrefix)
    if not held and (not isinstance(prefix, torch.Tensor) or prefix.dtype != torch.int64 or prefix.dim() != 1):
      raise TypeError(f'{who}: the prefix must be a 1-D int64 tensor or a PagedPrefix')
    if held and pool is not None and pool is not prefix.pool:
      raise ValueError(f'{who}: the PagedPrefix lives on another pool')
    guard(who, prompts[0], self, forward_only=True)
    N, S = len(prompts), int(max_batch)
    budget = [int(max_new_tokens)] * N if isinstance(max_new_tokens, int) else [int(v) for v in max_new_tokens]
    if len(budget) != N:
      raise ValueError(f'{who}: {len(budget)} budgets for {N} prompts')
    n_prefix = prefix.n_tokens + prefix.rest.numel() if held else prefix.numel()
    shared = n_prefix // ops.KV_PAGE_ROWS  # the pages held once
    total = [_check_new_tokens(who, n_prefix + prompts[i].numel(), budget[i], 0, '', [('', self.cfg.seq_len)]) for i in range(N)]
    pages = [-(-t // ops.KV_PAGE_ROWS) - shared for t in total]  # what sequence i holds of its own at the end of its budget
    if held:
      pool = prefix.pool
    elif pool is None:
      pool = self.new_page_pool(shared + min(S, N) * max(pages))
    if not held:
      prefix = self.prefill_prefix(prefix, pool)
    try:
      if max(pages) > pool.n_free:
        raise RuntimeError(f'{who}: the pool has {pool.n_free} free pages beside the prefix, one sequence needs {max(pages)}')
      return self._serve_ragged(who, [torch.cat([prefix.rest, t]) for t in prompts], budget, total, pages, S, pool, eos_id, fused, prefill_chunk,
                                prefix=prefix)
    finally:
      if not held:
        prefix.release()

  def fork(self, cache, n_samples, max_new_tokens):
    """A SharedPrefixCache for n_samples continuations of every prompt of the prefilled bf16 ``cache``, max_new_tokens suffix rows each.
    The prompts' rows stay where they are, once; ``cache`` must not be appended to afterwards.  Refused: an FP8 cache (ValueError), a
    SharedPrefixCache (TypeError), an mxfp8 model (ValueError)."""
    refuse_shared_mxfp8('fork', self)
    check_fork(cache, n_samples, max_new_tokens)
    check_cache('fork', cache, self)
    return SharedPrefixCache(cache, n_samples, max_new_tokens)

  @torch.compiler.disable
  def generate_samples(self, prompt, n_samples, max_new_tokens, prompt_lens=None, eos_id=None, temperature=None, top_k=None, top_p=None,
                       seed=None, return_logprobs=False, fused=False):
    """n_samples continuations of every prompt of prompt int64 [P, T] (best-of-n, self-consistency, policy-gradient rollouts): returns the
    new tokens int64 [P, n_samples, max_new_tokens], with return_logprobs also their log-probabilities fp32 of that shape.  ONE prefill of
    the P prompts; their k | v rows are stored once (``fork``) and every decode step reads them once per 32 samples (DESIGN.md section
    21).  The first token of all samples is drawn from the prompt's one last-row logits (the row repeated, one ops.sample_logits launch),
    the rest are decode steps on the SharedPrefixCache.  temperature / top_k / top_p / seed / eos_id / prompt_lens as ``generate`` takes
    them; the uniforms of the whole call are drawn once for P * n_samples rows, so a seed reproduces it bit for bit.  Without sampling
    arguments the call is greedy and the samples of a prompt are identical.  fused=True runs the decode steps through
    ops.decode_layer_shared and serves P * n_samples <= ops.FUSED_DECODE_MAX_ROWS, ValueError beyond."""
    who = 'generate_samples'
    refuse_shared_mxfp8(who, self)
    guard(who, prompt, self, forward_only=True, rank2=True)
    if isinstance(n_samples, bool) or not isinstance(n_samples, int) or n_samples < 1:
      raise ValueError(f'{who}: n_samples must be an int >= 1, got {n_samples!r}')
    P, T = prompt.shape
    G, N = n_samples, int(max_new_tokens)
    check_lengths(T, max_new_tokens, self.cfg.seq_len)
    on_device = check_sampling(temperature, top_k, top_p, None, seed)
    if fused:
      check_fused(who, P * G, self.cfg.dim)
    want_logits = on_device is not None
    cache, r = self.prefill(prompt, prompt_lens, max_len=pad4(T), logits=want_logits, kv_dtype='bf16')
    shared = self.fork(cache, G, N)
    with torch.no_grad():
      if want_logits:
        pick = sampling_pick(draw_uniforms(N, P * G, prompt.device, seed), *on_device)
        first = pick(r.repeat_interleave(G, dim=0))
      else:
        pick = lambda o: (o.tokens, o.logprob)  # noqa: E731
        first = (r.tokens.repeat_interleave(G), r.logprob.repeat_interleave(G))
      toks, lps = generate_loop(first, lambda t: pick(self.decode_step(t, shared, logits=want_logits, fused=fused)), N, eos_id)
    shared.check()
    toks, lps = toks.view(P, G, N), lps.view(P, G, N)
    return (toks, lps) if return_logprobs else toks

  def fork_beam(self, cache, num_beams, max_new_tokens):
    """``fork`` for beam search: a SharedPrefixCache of num_beams suffix slots per prompt with fresh ops.BeamBuffers
    as its ``beam``.  decode_step on it stores beam n's row in slot n and attends the rows ``beam.anc`` names; ops.beam_advance moves the
    table.  Refused: what ``fork`` refuses (an FP8 cache, a fork, an mxfp8 model) and num_beams outside [1, ops.BEAM_MAX]."""
    G = check_beam(num_beams)[0]
    shared = self.fork(cache, G, max_new_tokens)
    shared.beam = ops.BeamBuffers(shared.P, G, shared.Tmax, shared.status.device)
    return shared

  @torch.compiler.disable
  def generate_beam(self, prompt, max_new_tokens, num_beams, num_return=1, length_penalty=1.0, early_stopping=False, eos_id=None, pad_id=None,
                    prompt_lens=None, fused=False, temperature=None, top_k=None, top_p=None, seed=None, sample=None):
    """Beam search: the num_return <= num_beams best continuations of every prompt of prompt int64 [P, T] by score / length **
    length_penalty, score = the sum of the tokens' log-probabilities.  Returns (tokens int64 [P, num_return, max_new_tokens] padded with
    pad_id - default eos_id, then 0 - after a hypothesis's length, lengths int32 [P, num_return] with EOS counted, scores fp32 [P,
    num_return], best first).  ONE prefill; the prompts' k | v rows are stored once (``fork_beam``) and the beams' own rows are never copied
    when beams are re-parented: a decode step attends them through an ancestor table (ops.attn_decode_beam).  Every token is one decode
    step of P * num_beams rows with logits, one ops.beam_select (the 2 * num_beams best continuations per prompt; ties by beam, then
    token) and one ops.beam_advance.  A hypothesis ends at eos_id; a prompt is done when it holds num_beams finished hypotheses and
    (early_stopping, or no live beam can still beat the worst of them at the current length); the call ends when all are, looked at every
    FINISH_CHECK_EVERY steps.  Deterministic and bit-reproducible.  fused=True runs the decode steps through ops.decode_layer_beam and
    serves P * num_beams <= ops.FUSED_DECODE_MAX_ROWS.  Refused before any launch (ValueError / TypeError): num_beams outside [1, 32],
    num_return > num_beams, a vocabulary below 2 * num_beams, sampling arguments, an mxfp8 model, fused with too many rows;
    cfg.kv_cache = 'fp8' does not apply (the call prefills a bf16 cache, and ``fork_beam`` refuses an FP8 one)."""
    who = 'generate_beam'
    refuse_shared_mxfp8(who, self)
    guard(who, prompt, self, forward_only=True, rank2=True)
    G, R, lp, pad = check_beam(num_beams, num_return, length_penalty, self.cfg.vocab_size, eos_id, pad_id, temperature, top_k, top_p, seed, sample)
    P, T = prompt.shape
    check_lengths(T, max_new_tokens, self.cfg.seq_len)
    if fused:
      check_fused(who, P * G, self.cfg.dim)
    cache, first = self.prefill(prompt, prompt_lens, max_len=pad4(T), logits=True, kv_dtype='bf16')
    shared = self.fork_beam(cache, G, int(max_new_tokens))
    with torch.no_grad():
      out = beam_loop(first, lambda t: self.decode_step(t, shared, logits=True, fused=fused), max_new_tokens, G, R, lp, early_stopping, eos_id, pad,
                      buffers=shared.beam)
    shared.check()
    return out

  @torch.compiler.disable
  def generate(self, prompt, max_new_tokens, prompt_lens=None, eos_id=None, sample=None, return_logprobs=False, temperature=None,
               top_k=None, top_p=None, seed=None):
    """Continue prompt int64 [B, T] by max_new_tokens tokens: returns the new tokens int64 [B, max_new_tokens], with return_logprobs
    also their log-probabilities fp32 [B, max_new_tokens].  Greedy by default, through the fused prediction head (no logits are built);
    ``sample`` is an optional callable fp32 logits [B, V] -> int64 [B] (temperature, top-k, nucleus: the caller's few lines of torch),
    with which every step returns logits instead.  prompt_lens: host integers, the true length of every right-padded prompt.  After a
    sequence emits eos_id its later tokens are eos_id and their log-probabilities 0.  No device-to-host copy happens per token.
    temperature / top_k / top_p sample on the device (one ops.sample_logits launch per token next to the logits
    GEMM; top-k keeps ties with the k-th value, top-p keeps or drops equal logits together; the returned log-probabilities stay the
    model's, at temperature 1).  The uniforms of the whole call are drawn once, from a generator seeded with ``seed`` (bit-reproducible)
    or from torch's default generator.  temperature None or 0 without a filter is greedy; ``sample`` excludes all four.
    ``generate_fused`` is the same call with the decode steps run fused."""
    return self._generate('generate', False, prompt, max_new_tokens, prompt_lens, eos_id, sample, return_logprobs, temperature, top_k,
                          top_p, seed)

  @torch.compiler.disable
  def generate_fused(self, prompt, max_new_tokens, prompt_lens=None, eos_id=None, sample=None, return_logprobs=False, temperature=None,
                     top_k=None, top_p=None, seed=None):
    """``generate`` with every decode step run as ``decode_step(..., fused=True)`` (the prefill is unchanged): the
    same arguments, refusals and return values, tokens close to but not bit for bit those of ``generate`` (other fp32 summation
    orders).  Serves B <= ops.FUSED_DECODE_MAX_ROWS sequences and raises ValueError beyond, before anything is launched.  It is a method
    of its own, not a keyword of ``generate``, whose parameter list is pinned."""
    return self._generate('generate_fused', True, prompt, max_new_tokens, prompt_lens, eos_id, sample, return_logprobs, temperature, top_k,
                          top_p, seed)

  def _generate(self, who, fused, prompt, max_new_tokens, prompt_lens, eos_id, sample, return_logprobs, temperature, top_k, top_p, seed):
    guard(who, prompt, self, forward_only=True, rank2=True)
    max_len = check_lengths(prompt.shape[1], max_new_tokens, self.cfg.seq_len)
    on_device = check_sampling(temperature, top_k, top_p, sample, seed)
    if fused:
      check_fused(who, prompt.shape[0], self.cfg.dim)
    want_logits = sample is not None or on_device is not None
    if on_device is not None:
      pick = sampling_pick(draw_uniforms(max_new_tokens, prompt.shape[0], prompt.device, seed), *on_device)
    else:
      pick = (lambda r: sampled(sample, r)) if want_logits else (lambda r: (r.tokens, r.logprob))  # noqa: E731
    cache, r = self.prefill(prompt, prompt_lens, max_len=max_len, logits=want_logits)
    toks, lps = generate_loop(pick(r), lambda t: pick(self.decode_step(t, cache, logits=want_logits, fused=fused)), max_new_tokens,
                               eos_id)
    cache.check()
    return (toks, lps) if return_logprobs else toks

  @torch.compiler.disable
  def generate_speculative(self, prompt, max_new_tokens, draft, n_draft=4, prompt_lens=None, eos_id=None, return_logprobs=False,
                           temperature=None, top_k=None, top_p=None, seed=None, return_stats=False):
    """``generate`` by draft-and-verify rounds: ``draft`` - another Transformer of the same vocabulary, any shape - proposes n_draft
    tokens with decode steps, this model checks them in one ``extend`` of n_draft + 1 rows, and a sequence keeps the accepted tokens
    plus one of this model's own, so a round of one target step yields 1 .. n_draft + 1 tokens.  Greedy (temperature None or 0 without
    a filter): the tokens are what ``generate`` decodes greedily, the target side runs through the fused prediction head.  With
    temperature / top_k / top_p the draft samples on the device and ops.spec_verify applies the speculative-sampling acceptance rule, which
    leaves every token distributed as ``generate`` samples it (not the same tokens: the uniforms are used differently).  All uniforms of
    the call are drawn once, under ``seed`` (bit-reproducible) or from torch's default generator.  Returns the tokens int64 [B, N]; with
    return_logprobs also this model's log-probabilities at temperature 1, with return_stats also dict(rounds, drafted int64 [B], accepted
    int64 [B]).  After eos_id a sequence holds eos_id with log-probability 0.  One int32 is read from the device per round (are all
    sequences finished?); both caches move by device tensors only."""
    guard('generate_speculative', prompt, self, draft, forward_only=True, rank2=True)
    B, T = prompt.shape
    k, N = n_draft, int(max_new_tokens)
    max_len, sampling = check_speculative(T, max_new_tokens, k, self.cfg, draft.cfg, self.lm_head.weight.device,
                                          draft.lm_head.weight.device, temperature, top_k, top_p, seed)
    tcache, r = self.prefill(prompt, prompt_lens, max_len=max_len, logits=sampling is not None)
    dcache, _ = draft.prefill(prompt, prompt_lens, max_len=max_len)
    u = None if sampling is None else speculative_uniforms(N, k, B, prompt.device, seed)
    s = _SpecSession(self, draft, tcache, dcache, k, sampling, u)
    first = (r.tokens, r.logprob) if sampling is None else ops.sample_logits(r, u[0], *sampling)[:2]
    with torch.no_grad():
      toks, lps, stats = speculative_loop(first, s.draft_round, s.target_round, s.accept, N, k, eos_id, s.advance)
    tcache.check()
    dcache.check()
    res = (toks,) + ((lps,) if return_logprobs else ()) + ((stats,) if return_stats else ())
    return res[0] if len(res) == 1 else res

  @torch.compiler.disable
  def generate_lookup(self, prompt, max_new_tokens, n_draft=8, ngram=(1, 4), prompt_lens=None, eos_id=None, return_logprobs=False,
                      temperature=None, top_k=None, top_p=None, seed=None, return_stats=False):
    """``generate_speculative`` without a draft model: every round, one ops.lookup_draft launch finds the most recent
    earlier occurrence of the sequence's last ngram[0] .. ngram[1] tokens (the longest match wins) in its own prompt and output and
    proposes the n_draft tokens that followed; this model checks them in one ``extend`` of n_draft + 1 rows and a sequence keeps the
    accepted tokens plus one of this model's own.  A sequence without a match proposes nothing and the round is a plain decode step for
    it.  Greedy: the tokens are what ``generate`` decodes greedily.  With temperature / top_k / top_p, ops.spec_verify_lookup applies the
    acceptance rule of a deterministic draft (accept x with probability p(x), else draw from p without x), which leaves every token
    distributed as ``generate`` samples it.  The uniforms of the call are drawn once, under ``seed`` (bit-reproducible) or from torch's
    default generator.  Returns what generate_speculative returns: the tokens int64 [B, N]; with return_logprobs also this model's
    log-probabilities at temperature 1, with return_stats also dict(rounds, drafted int64 [B] = the proposals actually made, accepted
    int64 [B]).  After eos_id a sequence holds eos_id with log-probability 0.  One int32 is read from the device per round; there is no
    second cache and no draft prefill.  ``generate_lookup_fused`` is the same call with the rounds' chunks run fused."""
    return self._generate_lookup('generate_lookup', False, prompt, max_new_tokens, n_draft, ngram, prompt_lens, eos_id, return_logprobs,
                                 temperature, top_k, top_p, seed, return_stats)

  @torch.compiler.disable
  def generate_lookup_fused(self, prompt, max_new_tokens, n_draft=8, ngram=(1, 4), prompt_lens=None, eos_id=None, return_logprobs=False,
                            temperature=None, top_k=None, top_p=None, seed=None, return_stats=False):
    """``generate_lookup`` with every round's chunk - the first token's included - run as ``extend(..., fused=True)`` (DESIGN.md section
    18; the prefill is unchanged): the same arguments, refusals and return values, tokens close to but not bit for bit those of
    ``generate_lookup`` (other fp32 summation orders).  Serves B * (n_draft + 1) <= ops.FUSED_EXTEND_MAX_ROWS chunk rows and raises
    ValueError beyond, before anything is launched.  A method of its own, as ``generate_fused`` is."""
    return self._generate_lookup('generate_lookup_fused', True, prompt, max_new_tokens, n_draft, ngram, prompt_lens, eos_id, return_logprobs,
                                 temperature, top_k, top_p, seed, return_stats)

  def _generate_lookup(self, who, fused, prompt, max_new_tokens, n_draft, ngram, prompt_lens, eos_id, return_logprobs, temperature, top_k, top_p,
                       seed, return_stats):
    guard(who, prompt, self, forward_only=True, rank2=True)
    B, T = prompt.shape
    k, N = n_draft, int(max_new_tokens)
    max_len, sampling = check_lookup(T, max_new_tokens, k, ngram, self.cfg, temperature, top_k, top_p, seed)
    if fused:
      check_fused_rows(who, B, k + 1, self.cfg.dim)
    cache, r = self.prefill(prompt, prompt_lens, max_len=max_len, logits=sampling is not None)
    u = None if sampling is None else lookup_uniforms(N, k, B, prompt.device, seed)
    first = (r.tokens, r.logprob) if sampling is None else ops.sample_logits(r, u[0], *sampling)[:2]
    with torch.no_grad():
      s = _LookupSession(self, cache, prompt, first[0], k, ngram, N, sampling, u, fused=fused)
      toks, lps, stats = speculative_loop(first, s.draft_round, s.target_round, s.accept, N, k, eos_id, s.advance, drafted_in_round=s.drafted)
    cache.check()
    s.check()
    res = (toks,) + ((lps,) if return_logprobs else ()) + ((stats,) if return_stats else ())
    return res[0] if len(res) == 1 else res

  @torch.compiler.disable
  def extend_tree(self, tokens, parent, cache, token_lens=None, logits=False, fused=False):
    """``extend`` over a token TREE: tokens int64 [B, n], n <= ops.TREE_MAX_ROWS; row 0 is the root (the newest
    committed token, not yet in the cache) and parent int32 [B, n] on the device names every other row's parent (parent[b, 0] = -1,
    0 <= parent[b, r] < r).  Row r is stored at cache row lens[b] + r, rotated at position lens[b] + depth(r), and attends the cache and
    its own ancestors only, so its output is what ``extend`` gives it on its root-to-node path run as a chain.  token_lens: the real
    rows per sequence, as ``extend`` takes them.  Returns the [B, n] predictions - with logits=True the [B, n, V] logits - of ALL rows
    (rows at and beyond token_lens[b] mean nothing).  It advances nothing: the caller picks a path (ops.tree_accept) and commits it with
    ``cache.commit_tree(path, n_accept)``.  A tree whose parents break the rule stores nothing for its sequence and surfaces through
    ``cache.check()``.  fused=True runs every layer as one ops.extend_layer_tree call and serves B * n <= ops.FUSED_EXTEND_MAX_ROWS.
    Refused before any launch: a SharedPrefixCache (TypeError), an FP8 cache, n > 32, fused with too many rows (ValueError), an mxfp8 model."""
    who = 'extend_tree'
    refuse_tree_cache(who, cache)
    if isinstance(tokens, torch.Tensor) and (tokens.dim() != 2 or tokens.shape[0] != cache.B or tokens.shape[1] < 1):
      raise ValueError(f'{who}: tokens {tuple(tokens.shape)} are not a [B, n] chunk for the cache\'s batch of {cache.B}')
    guard(who, tokens, self)
    check_cache(who, cache, self)
    B, n = tokens.shape
    check_tree_rows(who, n)
    if not isinstance(parent, torch.Tensor) or parent.dtype != torch.int32 or tuple(parent.shape) != (B, n) or parent.device != tokens.device:
      raise TypeError(f'{who}: parent must be an int32 [{B}, {n}] tensor on the tokens\' device')
    if fused:
      check_fused_rows(who, B, n, self.cfg.dim)
    nh = self.cfg.n_heads
    with torch.no_grad():
      _, n_new = chunk_lens(token_lens, B, n, tokens.device)
      rope = self._rope(tokens.device)
      lens0 = cache.lens
      plan = ops.tree_plan(parent.contiguous(), n_new, status=cache.status)

      def attend(i, qkv):
        q, _ = ops.kv_append_rope_tree(qkv, lens0, plan.depth, rope[0], rope[1], cache.kv[i], nh, n_new=n_new, status=cache.status)
        return ops.attn_extend_tree(q, cache.kv[i], lens0, plan.anc, nh, n_new=n_new)
      flat = tokens.reshape(-1).contiguous()
      y = self.fused_layers(flat, cache, rope, (lens0, n_new, n, plan.depth, plan.anc)) if fused else self.cached_layers(flat, cache, attend)
      return self.head(y, logits, (B, n))

  @torch.compiler.disable
  def generate_lookup_tree(self, prompt, max_new_tokens, n_draft=8, n_branch=3, ngram=(1, 4), prompt_lens=None, eos_id=None, return_logprobs=False,
                           return_stats=False, fused=False, max_rows=None):
    """``generate_lookup`` that verifies several continuations per round: one ops.lookup_draft_tree launch keeps the
    up to n_branch most recent occurrences of the longest n-gram match and merges the n_draft tokens that followed each into a trie of at
    most min(1 + n_draft * n_branch, 32) rows; one ``extend_tree`` checks every node, ops.tree_accept takes the longest root-to-leaf path
    this model's greedy predictions follow, and ops.kv_tree_commit keeps that path's cache rows.  Greedy only: the tokens are what
    ``generate`` decodes greedily.  Sampled acceptance over a tree (sibling rejection sampling) is deliberately not built - there are no
    sampling arguments; use ``generate_lookup`` to sample.  Returns the tokens int64 [B, N]; with return_logprobs also this model's
    log-probabilities, with return_stats also dict(rounds, drafted int64 [B] = the nodes proposed below the roots, accepted int64 [B],
    nodes int64 [B] = the tree rows verified, the roots included).  One int32 is read from the device per round.  fused=True runs the
    rounds' chunks through ops.extend_layer_tree and serves B * rows <= ops.FUSED_EXTEND_MAX_ROWS, ValueError beyond: at the default width that
    is one sequence of n_draft 8, n_branch 3 - max_rows caps the rows per sequence (32 // B fits any B <= 16), the trie then keeps what the most
    recent matches fill first.  Refused before any
    launch: an mxfp8 model; cfg.kv_cache = 'fp8' does not apply (the call prefills a bf16 cache)."""
    who = 'generate_lookup_tree'
    guard(who, prompt, self, forward_only=True, rank2=True)
    B, T = prompt.shape
    N = int(max_new_tokens)
    max_len, n = check_lookup_tree(T, max_new_tokens, n_draft, n_branch, ngram, self.cfg, max_rows)
    if fused:
      check_fused_rows(who, B, n, self.cfg.dim)
    cache, r = self.prefill(prompt, prompt_lens, max_len=max_len, kv_dtype='bf16')
    first = (r.tokens, r.logprob)
    with torch.no_grad():
      s = _TreeSession(self, cache, prompt, first[0], n_draft, n_branch, n, ngram, N, fused=fused)
      toks, lps, stats = speculative_loop(first, s.draft_round, s.target_round, s.accept, N, n - 1, eos_id, s.advance, drafted_in_round=s.drafted)
    stats['nodes'] = s.nodes
    cache.check()
    s.check()
    res = (toks,) + ((lps,) if return_logprobs else ()) + ((stats,) if return_stats else ())
    return res[0] if len(res) == 1 else res
