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
fused_layers dispatch on the cache to the ops.*_kv8 twins of the same calls, and nothing else here knows about it.
"""

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
    if isinstance(tokens, torch.Tensor) and (tokens.dim() != 2 or tokens.shape[0] != cache.B or tokens.shape[1] < 1):
      raise ValueError(f'extend: tokens {tuple(tokens.shape)} are not a [B, n] chunk for the cache\'s batch of {cache.B}')
    guard('extend', tokens, self)
    check_cache('extend', cache, self)
    B, n = tokens.shape
    if fused:
      check_fused_rows('extend', B, n, self.cfg.dim)
    nh = self.cfg.n_heads
    with torch.no_grad():
      adv, n_new = chunk_lens(token_lens, B, n, tokens.device)
      rope = self._rope(tokens.device)
      lens0 = cache.lens  # the lengths before the chunk: what every layer's append and attention see; moved once, after the last layer

      append, attn = (ops.kv8_append_rope_rows, ops.attn_extend_kv8) if cache.kv_dtype == 'fp8' else (ops.kv_append_rope_rows, ops.attn_extend)

      def attend(i, qkv):
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
