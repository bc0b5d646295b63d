"""The ops wrappers of the ragged step over the paged KV cache: one packed list of R rows to which sequence b
contributes counts[b] of them - 0, 1 (a decode row) or a chunk of its prompt.  ``ops.ragged_plan`` (pure host) turns the counts into
the packed-row words; ``ops.kv_paged_append_rope_packed`` and ``ops.attn_ragged_paged`` are the attention stage of a cached step over
them, ``ops.ragged_norm_qkv_append_paged`` and ``ops.ragged_layer_paged`` the fused stage and layer at R <= FUSED_EXTEND_MAX_ROWS.

The packed-row contract: cu_rows int32 [B+1] (cu[0] = 0, non-decreasing), row_seq int32 [R], both on the device; row r is row
r - cu[b] of sequence b = row_seq[r] when 0 <= b < B and cu[b] <= r < cu[b+1], else padding (it stores nothing, gets zero q / out rows
and lse = +inf).  pool and table as ops_paged.py; bf16 pages only.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract, like ops_paged.py; no torch fallback."""

import torch

from . import _lib
from . import ops as O
from . import ops_paged as PG

RAGGED_TILE_ROWS = 32  # query rows per workgroup of attn_ragged_paged: what NT counts


def ragged_plan(counts):
  """Per-slot row counts (host ints >= 0) -> (cu_rows int32 [B+1], row_seq int32 [R], last_row int32 [B], NT) on the CPU: the packed
  order is the slot order, last_row[b] the packed index of sequence b's last row (-1: it has none), NT the number of 32-row tiles,
  sum of ceil(counts[b] / 32).  The caller ships the three tensors to the device as one non-blocking copy from a pinned snapshot."""
  counts = [int(c) for c in counts]
  if not counts or any(c < 0 for c in counts):
    raise ValueError(f'ragged_plan: need at least one count and none negative, got {counts}')
  cu, row_seq, last_row = [0], [], []
  for b, c in enumerate(counts):
    cu.append(cu[-1] + c)
    row_seq += [b] * c
    last_row.append(cu[-1] - 1 if c else -1)
  i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
  return i32(cu), i32(row_seq), i32(last_row), sum(-(-c // RAGGED_TILE_ROWS) for c in counts)


def _ragged_operands(name, rows, width, pool, table, nh, lens0, cu_rows, row_seq, rope=None):
  """The operand checks of the ragged ops, returns (R, B, hd, max_pages, n_pages).  rows: bf16 [R, width*nh*hd] - width 3 the UN-rotated
  qkv (row stride free), width 1 the rotated q; the batch is the table's."""
  try:
    if width == 3:
      O._need(rows, O.BF16, 'qkv', strided=True)
    else:
      O._need(rows, O.BF16, 'q', 2)
    if rows.shape[1] % (width * nh) != 0:
      raise ValueError(f'{"qkv" if width == 3 else "q"}: need rows of {width}*nh*hd columns, got {rows.shape[1]} for nh={nh}')
    hd = rows.shape[1] // (width * nh)
    PG._need_pool(pool, nh, hd)
    O._need(table, torch.int32, 'table', 2)
    O._need(lens0, torch.int32, 'lens0', 1)
    O._need(cu_rows, torch.int32, 'cu_rows', 1)
    O._need(row_seq, torch.int32, 'row_seq', 1)
    if rope is not None:
      O._need(rope[0], O.F32, 'rope_cos', 2)
      O._need(rope[1], O.F32, 'rope_sin', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  _fits(name, rows.shape[0], table, lens0, cu_rows, row_seq, hd, rope)
  return rows.shape[0], table.shape[0], hd, table.shape[1], pool.shape[0]


def _fits(name, R, table, lens0, cu_rows, row_seq, hd, rope):
  B = table.shape[0]
  fits = R >= 1 and B >= 1 and table.shape[1] >= 1 and lens0.shape[0] == B and cu_rows.shape[0] == B + 1 and row_seq.shape[0] == R
  if rope is not None:
    fits = fits and rope[0].shape == rope[1].shape and rope[0].shape[1] == hd // 2
  if not fits:
    raise ValueError(f'{name}: {R} rows, table {tuple(table.shape)}, lens0 {tuple(lens0.shape)}, cu_rows {tuple(cu_rows.shape)} (B + 1), row_seq '
                     f'{tuple(row_seq.shape)} (R) do not fit' + ('' if rope is None else f', or the RoPE tables {tuple(rope[0].shape)} the head_dim'))


def _tiles(name, NT, R):
  NT = int(NT)
  if not 1 <= NT <= R:
    raise ValueError(f'{name}: NT={NT} tiles outside [1, R = {R}] (ragged_plan counts them)')
  return NT


def kv_paged_append_rope_packed(qkv, lens0, cu_rows, row_seq, rope_cos, rope_sin, pool, table, nh, q_out=None, status=None):
  """ops.kv_paged_append_rope_rows over packed rows: qkv bf16 [R, 3*nh*hd]; row r (row j of sequence b) is rotated at lens0[b] + j -
  rotated q to q_out [R, nh*hd], rotated k | untouched v into its page - with that op's bits for the same row at the same position.
  A sequence whose rows leave the table or the RoPE rows, or need a page outside the pool, stores nothing, gets zero q_out rows and
  sets status[0] = 1; a padding row stores nothing and gets a zero q_out row.  Returns (q_out, status)."""
  name = 'kv_paged_append_rope_packed'
  R, B, hd, max_pages, n_pages = _ragged_operands(name, qkv, 3, pool, table, nh, lens0, cu_rows, row_seq, rope=(rope_cos, rope_sin))
  q_out, status = O._append_outputs(name, qkv, R, nh * hd, q_out, status)
  _lib.check(_lib.load().plm_kv_paged_append_rope_packed(O._p(qkv), qkv.stride(0), O._p(lens0), O._p(cu_rows), O._p(row_seq), O._p(rope_cos),
                                                         O._p(rope_sin), rope_cos.shape[0], O._p(q_out), O._p(pool), pool.stride(1), O._p(table),
                                                         O._p(status), R, B, max_pages, n_pages, nh, hd, O._stream()),
             'plm_kv_paged_append_rope_packed')
  return q_out, status


def attn_ragged_paged(q, pool, table, lens0, cu_rows, row_seq, nh, NT, Lcap=None, want_lse=False):
  """Attention of the packed rows over their sequences' pages: q bf16 [R, nh*hd] (kv_paged_append_rope_packed's q_out), the rows
  already appended, lens0 the lengths BEFORE the step (clamped to [0, Lcap]).  Row j of sequence b attends keys 0 .. lens0[b] + j; a
  padding row gives out = 0 and lse = +inf.  NT: ragged_plan's tile count (host int).  Lcap sizes the grid, never the bits.  Returns
  out bf16 [R, nh*hd], or (out, lse fp32 [R, nh], base 2) with want_lse."""
  name = 'attn_ragged_paged'
  R, B, hd, max_pages, n_pages = _ragged_operands(name, q, 1, pool, table, nh, lens0, cu_rows, row_seq)
  NT = _tiles(name, NT, R)
  Lcap = PG._lcap(name, Lcap, max_pages)
  nbytes = O._ws_bytes('plm_attn_ragged_paged_workspace_bytes', R, nh, hd, Lcap)
  if nbytes == 0:
    raise ValueError(f'{name}: unsupported shape R={R} nh={nh} hd={hd} Lcap={Lcap} (at most 64 chunks of {PG.KV_PAGED_CHUNK} keys)')
  stream = O._stream()
  ws = O._workspace(q.device, nbytes, stream)
  out = torch.empty((R, nh * hd), dtype=O.BF16, device=q.device)
  lse = torch.empty((R, nh), dtype=O.F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_ragged_paged(O._p(q), O._p(pool), pool.stride(1), O._p(table), O._p(lens0), O._p(cu_rows), O._p(row_seq), O._p(out),
                                               O._p(lse), R, B, NT, Lcap, max_pages, n_pages, nh, hd, O._p(ws), nbytes, stream), 'plm_attn_ragged_paged')
  return (out, lse) if want_lse else out


# ---- the fused layer over a ragged step: ops_paged.py's stage and layers under the packed-row map ---------------------------------------------
def _fused_ragged_operands(name, x, norms, weights, pool, table, lens0, cu_rows, row_seq, rope_cos, rope_sin, nh):
  """ops_decode's operand checks with a pool for the cache and the packed-row words; returns (R, d, hd, B, max_pages, n_pages)."""
  from . import ops_decode as D
  R, d = D._decode_operands(name, x, norms, weights)
  w_qkv = weights[0]
  if d % nh != 0 or tuple(w_qkv.shape) != (3 * d, d):
    raise ValueError(f'{name}: x {tuple(x.shape)}, w_qkv {tuple(w_qkv.shape)} do not fit nh={nh}')
  hd = d // nh
  try:
    PG._need_pool(pool, nh, hd)
    O._need(table, torch.int32, 'table', 2)
    O._need(lens0, torch.int32, 'lens0', 1)
    O._need(cu_rows, torch.int32, 'cu_rows', 1)
    O._need(row_seq, torch.int32, 'row_seq', 1)
    O._need(rope_cos, O.F32, 'rope_cos', 2)
    O._need(rope_sin, O.F32, 'rope_sin', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  _fits(name, R, table, lens0, cu_rows, row_seq, hd, (rope_cos, rope_sin))
  return R, d, hd, table.shape[0], table.shape[1], pool.shape[0]


def ragged_norm_qkv_append_paged(x, norm_w, eps, w_qkv, lens0, cu_rows, row_seq, rope_cos, rope_sin, pool, table, nh, q_out=None, status=None):
  """ops.extend_norm_qkv_append_paged over packed rows: x fp32 [R, d], R <= FUSED_EXTEND_MAX_ROWS; the same arithmetic, so q_out and the
  stored rows are that op's bits for the same rows at the same positions, under kv_paged_append_rope_packed's refusal predicate.
  Returns (rotated q bf16 [R, d], status)."""
  name = 'ragged_norm_qkv_append_paged'
  R, d, hd, B, max_pages, n_pages = _fused_ragged_operands(name, x, (norm_w,), (w_qkv,), pool, table, lens0, cu_rows, row_seq, rope_cos, rope_sin, nh)
  q_out, status = O._append_outputs(name, x, R, d, q_out, status)
  with O._Launch('hbm:decode_fused', 2.0 * w_qkv.numel()):
    _lib.check(_lib.load().plm_ragged_norm_qkv_append_paged_bf16(O._p(x), O._p(norm_w), float(eps), O._p(w_qkv), O._p(lens0), O._p(cu_rows),
                                                                 O._p(row_seq), O._p(rope_cos), O._p(rope_sin), rope_cos.shape[0], O._p(q_out),
                                                                 O._p(pool), pool.stride(1), O._p(table), O._p(status), R, B, max_pages, n_pages, nh,
                                                                 hd, O._stream()), 'plm_ragged_norm_qkv_append_paged_bf16')
  return q_out, status


def ragged_layer_paged(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, cu_rows, row_seq, rope_cos, rope_sin, pool, table, nh,
                       kind, status, NT, Lcap=None):
  """One layer of a ragged step, one library call: ragged_norm_qkv_append_paged, attn_ragged_paged, then decode_layer's out, fc1 and fc2
  stages.  x fp32 [R, d] (R <= FUSED_EXTEND_MAX_ROWS packed rows) is updated in place and returned."""
  from . import ops_decode as D
  name = 'ragged_layer_paged'
  R, d, hd, B, max_pages, n_pages = _fused_ragged_operands(name, x, (attn_norm_w, mlp_norm_w), (w_qkv, w_out, w_fc1, w_fc2), pool, table, lens0,
                                                           cu_rows, row_seq, rope_cos, rope_sin, nh)
  k = D._decode_mlp_kind(name, kind)
  hidden = w_fc2.shape[1]
  if tuple(w_out.shape) != (d, d) or w_fc2.shape[0] != d or tuple(w_fc1.shape) != ((2 if kind == 'glu' else 1) * hidden, d):
    raise ValueError(f'{name}: the weights {tuple(w_out.shape)}, {tuple(w_fc1.shape)}, {tuple(w_fc2.shape)} do not fit x {tuple(x.shape)}, '
                     f'kind {kind!r}')
  try:
    O._need(status, torch.int32, 'status')
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  NT = _tiles(name, NT, R)
  Lcap = PG._lcap(name, Lcap, max_pages)
  nbytes = O._ws_bytes('plm_ragged_layer_paged_workspace_bytes', R, nh, hd, hidden, Lcap)
  if nbytes == 0:
    raise ValueError(f'{name}: unsupported shape R={R} nh={nh} hd={hd} hidden={hidden} Lcap={Lcap}')
  stream = O._stream()
  ws = O._workspace(x.device, nbytes, stream)
  with O._Launch('hbm:decode_fused', 2.0 * (w_qkv.numel() + w_out.numel() + w_fc1.numel() + w_fc2.numel())):
    _lib.check(_lib.load().plm_ragged_layer_paged_bf16(O._p(x), O._p(attn_norm_w), O._p(mlp_norm_w), float(eps), O._p(w_qkv), O._p(w_out),
                                                       O._p(w_fc1), O._p(w_fc2), O._p(lens0), O._p(cu_rows), O._p(row_seq), O._p(rope_cos),
                                                       O._p(rope_sin), rope_cos.shape[0], O._p(pool), pool.stride(1), O._p(table), O._p(status), R, B,
                                                       NT, Lcap, max_pages, n_pages, nh, hd, hidden, k, O._p(ws), nbytes, stream),
               'plm_ragged_layer_paged_bf16')
  return x
