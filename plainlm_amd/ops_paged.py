"""The ops wrappers of the paged KV cache: ``ops.kv_paged_append_rope_rows`` (a chunk's rotated k | v rows into the
pages of a pool, the decode step at n = 1), ``ops.kv_paged_store_rows`` (prefill's scatter of a prompt's rows), ``ops.attn_decode_paged``
(one query row per sequence, split by length into chunks of KV_PAGED_CHUNK keys) and ``ops.attn_extend_paged`` (a chunk of query rows,
page-aligned splits).

Operands: pool bf16 [n_pages, KV_PAGE_ROWS, 2*nh*hd] is one layer's pages in ops.kv_append_rope's row layout (the row stride may be
padded); table int32 [B, max_pages] names the page of tokens 64*i .. 64*i + 63 of sequence b, -1 for none.  bf16 pages only: an FP8 pool
is refused.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract - the operand validator (``ops._need``), the
workspace arena of the current stream, ``_lib.check`` around the one library call - and, like every wrapper there, launch hand-written
gfx950 kernels with no torch fallback.  They live in a module of their own for ops_decode.py's reason."""

import torch

from . import _lib
from . import ops as O

KV_PAGE_ROWS = 64      # PLM_KV_PAGE_ROWS: token rows per page
KV_PAGED_CHUNK = 512   # PLM_KV_PAGED_CHUNK of csrc/attn_paged.hip: keys per workgroup of attn_decode_paged (it decides the bits)


def _paged_operands(name, rows, width, pool, table, nh, lens, lens_name, n_new=None, rope=None):
  """The operand checks of the paged cached-step ops, returns (B, n, hd, max_pages, n_pages).  rows: bf16 [B*n, width*nh*hd] - width 3
  the UN-rotated qkv (row stride free), width 1 the rotated q; the batch is the table's."""
  try:
    if width == 3:
      O._need(rows, O.BF16, 'qkv', strided=True)
    else:
      O._need(rows, O.BF16, 'q', 2)
    if rows.shape[1] % (width * nh) != 0:
      raise ValueError(f'{"qkv" if width == 3 else "q"}: need rows of {width}*nh*hd columns, got {rows.shape[1]} for nh={nh}')
    hd = rows.shape[1] // (width * nh)
    _need_pool(pool, nh, hd)
    O._need(table, torch.int32, 'table', 2)
    O._need(lens, torch.int32, lens_name, 1)
    if rope is not None:
      O._need(rope[0], O.F32, 'rope_cos', 2)
      O._need(rope[1], O.F32, 'rope_sin', 2)
    if n_new is not None:
      O._need(n_new, torch.int32, 'n_new', 1)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  B = table.shape[0]
  fits = B >= 1 and table.shape[1] >= 1 and lens.shape[0] == B and rows.shape[0] >= B and rows.shape[0] % B == 0
  if rope is not None:
    fits = fits and rope[0].shape == rope[1].shape and rope[0].shape[1] == hd // 2
  if not fits:
    raise ValueError(f'{name}: rows {tuple(rows.shape)}, table {tuple(table.shape)}, {lens_name} {tuple(lens.shape)} do not fit nh={nh}'
                     + ('' if rope is None else f', or the RoPE tables {tuple(rope[0].shape)} / {tuple(rope[1].shape)} the head_dim'))
  if n_new is not None and n_new.shape[0] != B:
    raise ValueError(f'{name}: n_new {tuple(n_new.shape)} does not fit the batch of {B}')
  return B, rows.shape[0] // B, hd, table.shape[1], pool.shape[0]


def _need_pool(pool, nh, hd):
  """pool bf16 [n_pages, 64, >= 2*nh*hd]: rows may be padded (stride(1) a multiple of 8), pages are 64 rows apart."""
  if not pool.is_cuda:
    raise RuntimeError('pool: tensor must live on the GPU (plainlm_amd has no CPU path)')
  if pool.dtype == torch.uint8:
    raise TypeError('pool: FP8 pages are not served by the paged kernels (bf16 pages only)')
  if pool.dtype != O.BF16 or pool.dim() != 3 or pool.shape[1] != KV_PAGE_ROWS or pool.shape[2] != 2 * nh * hd or pool.stride(2) != 1 or \
     pool.stride(0) != KV_PAGE_ROWS * pool.stride(1):
    raise ValueError(f'pool: need a bf16 [n_pages, {KV_PAGE_ROWS}, 2*nh*hd] pool with unit inner stride and page stride {KV_PAGE_ROWS} * row stride')


def _lcap(name, Lcap, max_pages):
  cap = max_pages * KV_PAGE_ROWS
  Lcap = cap if Lcap is None else int(Lcap)
  if not 1 <= Lcap <= cap:
    raise ValueError(f'{name}: Lcap={Lcap} outside [1, max_pages * {KV_PAGE_ROWS} = {cap}]')
  return Lcap


def kv_paged_append_rope_rows(qkv, lens0, rope_cos, rope_sin, pool, table, nh, n_new=None, q_out=None, status=None):
  """ops.kv_append_rope_rows into a paged cache: rows r < n_new[b] of qkv bf16 [B*n, 3*nh*hd] are rotated at position lens0[b] + r -
  rotated q to q_out [B*n, nh*hd] (that op's bits), rotated k | untouched v into row (lens0[b] + r) % 64 of page
  table[b, (lens0[b] + r) / 64].  A sequence whose chunk leaves the table or the RoPE rows, or needs a page that is -1 or outside the
  pool, stores nothing, gets zero q_out rows and sets status[0] = 1.  n = 1 is the decode step's append.  Returns (q_out, status)."""
  name = 'kv_paged_append_rope_rows'
  B, n, hd, max_pages, n_pages = _paged_operands(name, qkv, 3, pool, table, nh, lens0, 'lens0', n_new=n_new, rope=(rope_cos, rope_sin))
  q_out, status = O._append_outputs(name, qkv, B * n, nh * hd, q_out, status)
  _lib.check(_lib.load().plm_kv_paged_append_rope_rows(O._p(qkv), qkv.stride(0), O._p(lens0), O._p(n_new), O._p(rope_cos), O._p(rope_sin),
                                                       rope_cos.shape[0], O._p(q_out), O._p(pool), pool.stride(1), O._p(table), O._p(status), B, n,
                                                       max_pages, n_pages, nh, hd, O._stream()), 'plm_kv_paged_append_rope_rows')
  return q_out, status


def kv_paged_store_rows(rows, lens, pool, table, nh, status=None):
  """Prefill's scatter: rows bf16 [B, T, 2*nh*hd] (unit inner stride, any row stride, batch stride T * row stride: the k | v columns of
  the trunk's rotated qkv); row t < lens[b] goes to its page.  Rows at or beyond lens[b] are never read and need no page; a row whose
  page is missing is not stored and sets status[0] = 1.  Returns status."""
  name = 'kv_paged_store_rows'
  if not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dtype != O.BF16 or rows.dim() != 3 or rows.stride(2) != 1 or \
     rows.stride(0) != rows.shape[1] * rows.stride(1) or rows.shape[2] % (2 * nh) != 0:
    raise ValueError(f'{name}.rows: need a bf16 [B, T, 2*nh*hd] GPU tensor with unit inner stride and batch stride T * row stride')
  B, T, hd = rows.shape[0], rows.shape[1], rows.shape[2] // (2 * nh)
  try:
    _need_pool(pool, nh, hd)
    O._need(table, torch.int32, 'table', 2)
    O._need(lens, torch.int32, 'lens', 1)
    if status is not None:
      O._need(status, torch.int32, 'status')
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  if table.shape[0] != B or lens.shape[0] != B:
    raise ValueError(f'{name}: rows {tuple(rows.shape)}, table {tuple(table.shape)}, lens {tuple(lens.shape)} do not fit')
  if status is None:
    status = torch.zeros((1,), dtype=torch.int32, device=rows.device)
  _lib.check(_lib.load().plm_kv_paged_store_rows(O._p(rows), rows.stride(1), O._p(lens), O._p(pool), pool.stride(1), O._p(table), O._p(status), B, T,
                                                 table.shape[1], pool.shape[0], nh, hd, O._stream()), 'plm_kv_paged_store_rows')
  return status


def attn_decode_paged_workspace_bytes(B, nh, hd, Lcap):
  """Workspace bytes of attn_decode_paged; a shape the library refuses (more than 64 chunks among them) raises."""
  nbytes = O._ws_bytes('plm_attn_decode_paged_workspace_bytes', B, nh, hd, int(Lcap))
  if nbytes == 0:
    raise ValueError(f'attn_decode_paged: unsupported shape B={B} nh={nh} hd={hd} Lcap={Lcap} (at most 64 chunks of {KV_PAGED_CHUNK} keys)')
  return nbytes


def attn_decode_paged(q, pool, table, lens, nh, Lcap=None, want_lse=False):
  """Attention of one rotated query row per sequence over its pages: q bf16 [B, nh*hd]; sequence b attends keys 0 .. lens[b]-1 (lens
  clamped to [0, Lcap]; 0 gives out = 0 and lse = +inf).  Lcap: the keys of the table to walk (host int, default max_pages * 64) - it
  sizes the grid, ceil(Lcap / KV_PAGED_CHUNK) chunks per (sequence, head), never the bits.  Returns out bf16 [B, nh*hd], or (out, lse
  fp32 [B, nh], base 2) with want_lse."""
  name = 'attn_decode_paged'
  B, n, hd, max_pages, n_pages = _paged_operands(name, q, 1, pool, table, nh, lens, 'lens')
  if n != 1:
    raise ValueError(f'{name}: q {tuple(q.shape)} is not one row per sequence of the table {tuple(table.shape)}')
  Lcap = _lcap(name, Lcap, max_pages)
  nbytes = attn_decode_paged_workspace_bytes(B, nh, hd, Lcap)
  stream = O._stream()
  ws = O._workspace(q.device, nbytes, stream)
  out = torch.empty((B, nh * hd), dtype=O.BF16, device=q.device)
  lse = torch.empty((B, nh), dtype=O.F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_decode_paged(O._p(q), O._p(pool), pool.stride(1), O._p(table), O._p(lens), O._p(out), O._p(lse), B, Lcap,
                                               max_pages, n_pages, nh, hd, O._p(ws), nbytes, stream), 'plm_attn_decode_paged')
  return (out, lse) if want_lse else out


def attn_extend_paged(q, pool, table, lens0, nh, n_new=None, Lcap=None, splits=0, want_lse=False):
  """ops.attn_extend over a paged cache: q bf16 [B*n, nh*hd] (kv_paged_append_rope_rows's q_out), the chunk already appended, lens0 the
  lengths BEFORE the chunk (clamped to [0, Lcap]).  Row r < n_new[b] attends keys 0 .. lens0[b] + r; rows past n_new[b] give out = 0 and
  lse = +inf.  splits: 0 automatic (from the shape alone) | 1..64 forced; a split is whole pages.  Returns out bf16 [B*n, nh*hd], or
  (out, lse fp32 [B, nh, n], base 2) with want_lse."""
  name = 'attn_extend_paged'
  B, n, hd, max_pages, n_pages = _paged_operands(name, q, 1, pool, table, nh, lens0, 'lens0', n_new=n_new)
  Lcap = _lcap(name, Lcap, max_pages)
  nbytes = O._ws_bytes('plm_attn_extend_paged_workspace_bytes', B, n, nh, hd, Lcap, int(splits))
  if nbytes == 0:
    raise ValueError(f'{name}: unsupported shape B={B} n={n} nh={nh} hd={hd} Lcap={Lcap} or splits={splits} (0 = automatic, 1..64)')
  stream = O._stream()
  ws = O._workspace(q.device, nbytes, stream)
  out = torch.empty((B * n, nh * hd), dtype=O.BF16, device=q.device)
  lse = torch.empty((B, nh, n), dtype=O.F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_extend_paged(O._p(q), O._p(pool), pool.stride(1), O._p(table), O._p(lens0), O._p(n_new), O._p(out), O._p(lse), B,
                                               n, Lcap, max_pages, n_pages, nh, hd, int(splits), O._p(ws), nbytes, stream), 'plm_attn_extend_paged')
  return (out, lse) if want_lse else out


# ---- the fused layer over a paged cache: ops_decode.py's stage and layers with the pool and the table in the cache's place --------------------
def _fused_paged_operands(name, x, norms, weights, pool, table, lengths, rope_cos, rope_sin, nh):
  """ops_decode's operand checks with a pool for the cache; returns (M, d, hd, B, n, max_pages, n_pages)."""
  from . import ops_decode as D
  M, d = D._decode_operands(name, x, norms, weights)
  w_qkv = weights[0]
  if d % nh != 0 or tuple(w_qkv.shape) != (3 * d, d):
    raise ValueError(f'{name}: x {tuple(x.shape)}, w_qkv {tuple(w_qkv.shape)} do not fit nh={nh}')
  hd = d // nh
  try:
    _need_pool(pool, nh, hd)
    O._need(table, torch.int32, 'table', 2)
    for what, t in lengths.items():
      if t is not None:
        O._need(t, torch.int32, what, 1)
    O._need(rope_cos, O.F32, 'rope_cos', 2)
    O._need(rope_sin, O.F32, 'rope_sin', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  B = table.shape[0]
  if B < 1 or table.shape[1] < 1 or M % B != 0 or any(t is not None and t.shape[0] != B for t in lengths.values()) or \
     rope_cos.shape != rope_sin.shape or rope_cos.shape[1] != hd // 2:
    raise ValueError(f'{name}: table {tuple(table.shape)}, the per-sequence operands or the RoPE tables {tuple(rope_cos.shape)} do not fit '
                     f'{M} rows, head_dim={hd}')
  return M, d, hd, B, M // B, table.shape[1], pool.shape[0]


def extend_norm_qkv_append_paged(x, norm_w, eps, w_qkv, lens0, rope_cos, rope_sin, pool, table, nh, n_new=None, q_out=None, status=None):
  """ops.extend_norm_qkv_append into a paged cache: x fp32 [B*n, d] (B = table.shape[0], B*n <= FUSED_EXTEND_MAX_ROWS); the same
  arithmetic, so q_out and the stored rows are that op's bits, at kv_paged_append_rope_rows's addresses and under its refusal predicate.
  Returns (rotated q bf16 [B*n, d], status)."""
  name = 'extend_norm_qkv_append_paged'
  M, d, hd, B, n, max_pages, n_pages = _fused_paged_operands(name, x, (norm_w,), (w_qkv,), pool, table, {'lens0': lens0, 'n_new': n_new},
                                                             rope_cos, rope_sin, nh)
  q_out, status = O._append_outputs(name, x, M, d, q_out, status)
  with O._Launch('hbm:decode_fused', 2.0 * w_qkv.numel()):
    _lib.check(_lib.load().plm_extend_norm_qkv_append_paged_bf16(O._p(x), O._p(norm_w), float(eps), O._p(w_qkv), O._p(lens0), O._p(n_new),
                                                                 O._p(rope_cos), O._p(rope_sin), rope_cos.shape[0], O._p(q_out), O._p(pool),
                                                                 pool.stride(1), O._p(table), O._p(status), B, n, max_pages, n_pages, nh, hd,
                                                                 O._stream()), 'plm_extend_norm_qkv_append_paged_bf16')
  return q_out, status


def _layer_paged(name, decode, x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lengths, rope_cos, rope_sin, pool, table, nh, kind,
                 status, Lcap, splits):
  """Both paged layers: ``lengths`` are the entry point's per-sequence operands in its order."""
  from . import ops_decode as D
  M, d, hd, B, n, max_pages, n_pages = _fused_paged_operands(name, x, (attn_norm_w, mlp_norm_w), (w_qkv, w_out, w_fc1, w_fc2), pool, table,
                                                             lengths, rope_cos, rope_sin, nh)
  k = D._decode_mlp_kind(name, kind)
  hidden = w_fc2.shape[1]
  if tuple(w_out.shape) != (d, d) or w_fc2.shape[0] != d or tuple(w_fc1.shape) != ((2 if kind == 'glu' else 1) * hidden, d) or (decode and n != 1):
    raise ValueError(f'{name}: the weights {tuple(w_out.shape)}, {tuple(w_fc1.shape)}, {tuple(w_fc2.shape)} do not fit x {tuple(x.shape)}, '
                     f'kind {kind!r}' + (f', or x is not one row per sequence of the table {tuple(table.shape)}' if decode else ''))
  try:
    O._need(status, torch.int32, 'status')
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  Lcap = _lcap(name, Lcap, max_pages)
  rows, tail = ((B,), ()) if decode else ((B, n), (int(splits),))
  nbytes = O._ws_bytes(f'plm_{name}_workspace_bytes', *rows, nh, hd, hidden, Lcap, *tail)
  if nbytes == 0:
    raise ValueError(f'{name}: unsupported shape B={B} n={n} nh={nh} hd={hd} hidden={hidden} Lcap={Lcap} splits={splits}')
  stream = O._stream()
  ws = O._workspace(x.device, nbytes, stream)
  with O._Launch('hbm:decode_fused', 2.0 * (w_qkv.numel() + w_out.numel() + w_fc1.numel() + w_fc2.numel())):
    _lib.check(getattr(_lib.load(), f'plm_{name}_bf16')(O._p(x), O._p(attn_norm_w), O._p(mlp_norm_w), float(eps), O._p(w_qkv), O._p(w_out),
                                                        O._p(w_fc1), O._p(w_fc2), *map(O._p, lengths.values()), O._p(rope_cos), O._p(rope_sin),
                                                        rope_cos.shape[0], O._p(pool), pool.stride(1), O._p(table), O._p(status), *rows, Lcap,
                                                        max_pages, n_pages, nh, hd, hidden, k, *tail, O._p(ws), nbytes, stream),
               f'plm_{name}_bf16')
  return x


def decode_layer_paged(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, pos, lens, rope_cos, rope_sin, pool, table, nh, kind, status,
                       live=None, Lcap=None):
  """ops.decode_layer over a paged cache, one library call: extend_norm_qkv_append_paged at n = 1 (lens0 = pos, n_new = live: a slot with
  live[b] = 0 appends nothing), attn_decode_paged over lens, then decode_layer's out, fc1 and fc2 stages.  x fp32 [B, d] is updated in
  place and returned."""
  return _layer_paged('decode_layer_paged', True, x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2,
                      {'pos': pos, 'lens': lens, 'live': live}, rope_cos, rope_sin, pool, table, nh, kind, status, Lcap, 0)


def extend_layer_paged(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, n_new, rope_cos, rope_sin, pool, table, nh, kind,
                       status, Lcap=None, splits=0):
  """ops.extend_layer over a paged cache, one library call: extend_norm_qkv_append_paged, attn_extend_paged, then the same three stages.
  x fp32 [B*n, d] (B = table.shape[0]) is updated in place and returned; n_new may be None."""
  return _layer_paged('extend_layer_paged', False, x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, {'lens0': lens0, 'n_new': n_new},
                      rope_cos, rope_sin, pool, table, nh, kind, status, Lcap, splits)
