"""The ops wrappers of the wide fused layer: the ragged paged layer over 1 <= R <= FUSED_WIDE_MAX_ROWS packed rows
on a kernel family of its own (csrc/layer_wide.hip).  ``ops.wide_gemm_residual`` and ``ops.wide_norm_fc1_act`` are ops.decode_gemm_residual
and ops.decode_norm_fc1_act at up to 256 rows, ``ops.ragged_norm_qkv_append_paged_wide`` and ``ops.ragged_layer_paged_wide`` the ragged
stage and layer of ops_ragged.py at up to 256 rows.  The same rounding points as their skinny-M namesakes, another order of the fp32
sums: close to their results, not their bits.  A row's bits depend on that row and the weights alone, whatever shared its launch.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract, like ops_ragged.py; no torch fallback."""

import torch

from . import _lib
from . import ops as O
from . import ops_decode as D
from . import ops_paged as PG
from . import ops_ragged as RG

FUSED_WIDE_MAX_ROWS = 256  # M of the wide kernels: four 64-row tiles


def _wide_operands(name, x, norms, weights):
  """ops_decode._decode_operands at the wide cap: x fp32 [M, d] with 1 <= M <= FUSED_WIDE_MAX_ROWS.  Returns (M, d)."""
  try:
    O._need(x, O.F32, 'x', 2)
    for w in norms:
      if O._need(w, O.F32, 'norm weight', 1).shape[0] != x.shape[1]:
        raise ValueError(f'norm weight: need [{x.shape[1]}], got {tuple(w.shape)}')
    for w in weights:
      O._need(w, O.BF16, 'weight', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  M, d = x.shape
  if not 1 <= M <= FUSED_WIDE_MAX_ROWS:
    raise ValueError(f'{name}: {M} rows; the wide fused kernels take 1 to {FUSED_WIDE_MAX_ROWS}')
  return M, d


def wide_gemm_residual(x, a, w):
  """x[M, N] += float(bf16(a[M, K] @ w[N, K]^T)) in place on the fp32 residual stream; M <= FUSED_WIDE_MAX_ROWS.  Returns x."""
  name = 'wide_gemm_residual'
  M, N = _wide_operands(name, x, (), (a, w))
  if a.shape[0] != M or w.shape[0] != N or w.shape[1] != a.shape[1]:
    raise ValueError(f'{name}: x {tuple(x.shape)}, a {tuple(a.shape)}, w {tuple(w.shape)} do not fit')
  with O._Launch('hbm:layer_wide', 2.0 * w.numel()):
    _lib.check(_lib.load().plm_wide_gemm_residual_bf16(O._p(x), O._p(a), O._p(w), M, N, a.shape[1], O._stream()), 'plm_wide_gemm_residual_bf16')
  return x


def wide_norm_fc1_act(x, norm_w, eps, w_fc1, kind):
  """rmsnorm_fwd -> gemm_nt -> swiglu_fwd / act_fwd in one launch: x fp32 [M, d] (M <= FUSED_WIDE_MAX_ROWS), w_fc1 bf16 [2h, d] ('glu':
  gate | up) or [h, d] ('silu', 'relu_sq').  Returns the activation bf16 [M, h]."""
  name = 'wide_norm_fc1_act'
  M, d = _wide_operands(name, x, (norm_w,), (w_fc1,))
  k = D._decode_mlp_kind(name, kind)
  mult = 2 if kind == 'glu' else 1
  if w_fc1.shape[1] != d or w_fc1.shape[0] % mult != 0:
    raise ValueError(f'{name}: x {tuple(x.shape)}, w_fc1 {tuple(w_fc1.shape)} do not fit kind {kind!r}')
  h = w_fc1.shape[0] // mult
  act = torch.empty((M, h), dtype=O.BF16, device=x.device)
  with O._Launch('hbm:layer_wide', 2.0 * w_fc1.numel()):
    _lib.check(_lib.load().plm_wide_norm_fc1_act_bf16(O._p(x), O._p(norm_w), float(eps), O._p(w_fc1), O._p(act), M, d, h, k, O._stream()),
               'plm_wide_norm_fc1_act_bf16')
  return act


def _wide_ragged_operands(name, x, norms, weights, pool, table, lens0, cu_rows, row_seq, rope_cos, rope_sin, nh):
  """ops_ragged._fused_ragged_operands at the wide cap; returns (R, d, hd, B, max_pages, n_pages)."""
  R, d = _wide_operands(name, x, norms, weights)
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
  RG._fits(name, R, table, lens0, cu_rows, row_seq, hd, (rope_cos, rope_sin))
  return R, d, hd, table.shape[0], table.shape[1], pool.shape[0]


def ragged_norm_qkv_append_paged_wide(x, norm_w, eps, w_qkv, lens0, cu_rows, row_seq, rope_cos, rope_sin, pool, table, nh, q_out=None, status=None):
  """ops.ragged_norm_qkv_append_paged at R <= FUSED_WIDE_MAX_ROWS packed rows: x fp32 [R, d]; row r (row j of sequence b) is normed,
  projected, rotated at lens0[b] + j; q to q_out, k | v into its page, under kv_paged_append_rope_packed's refusal predicate (a chunk may
  touch five pages).  Returns (rotated q bf16 [R, d], status)."""
  name = 'ragged_norm_qkv_append_paged_wide'
  R, d, hd, B, max_pages, n_pages = _wide_ragged_operands(name, x, (norm_w,), (w_qkv,), pool, table, lens0, cu_rows, row_seq, rope_cos, rope_sin, nh)
  q_out, status = O._append_outputs(name, x, R, d, q_out, status)
  with O._Launch('hbm:layer_wide', 2.0 * w_qkv.numel()):
    _lib.check(_lib.load().plm_ragged_norm_qkv_append_paged_wide_bf16(O._p(x), O._p(norm_w), float(eps), O._p(w_qkv), O._p(lens0), O._p(cu_rows),
                                                                      O._p(row_seq), O._p(rope_cos), O._p(rope_sin), rope_cos.shape[0],
                                                                      O._p(q_out), O._p(pool), pool.stride(1), O._p(table), O._p(status), R, B,
                                                                      max_pages, n_pages, nh, hd, O._stream()),
               'plm_ragged_norm_qkv_append_paged_wide_bf16')
  return q_out, status


def ragged_layer_paged_wide(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, cu_rows, row_seq, rope_cos, rope_sin, pool, table,
                            nh, kind, status, NT, Lcap=None):
  """One layer of a ragged step of R <= FUSED_WIDE_MAX_ROWS packed rows, one library call: ragged_norm_qkv_append_paged_wide,
  attn_ragged_paged, wide_gemm_residual with w_out, wide_norm_fc1_act, wide_gemm_residual with w_fc2.  x fp32 [R, d] is updated in place
  and returned."""
  name = 'ragged_layer_paged_wide'
  R, d, hd, B, max_pages, n_pages = _wide_ragged_operands(name, x, (attn_norm_w, mlp_norm_w), (w_qkv, w_out, w_fc1, w_fc2), pool, table, lens0,
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
  NT = RG._tiles(name, NT, R)
  Lcap = PG._lcap(name, Lcap, max_pages)
  nbytes = O._ws_bytes('plm_ragged_layer_paged_wide_workspace_bytes', R, nh, hd, hidden, Lcap)
  if nbytes == 0:
    raise ValueError(f'{name}: unsupported shape R={R} nh={nh} hd={hd} hidden={hidden} Lcap={Lcap}')
  stream = O._stream()
  ws = O._workspace(x.device, nbytes, stream)
  with O._Launch('hbm:layer_wide', 2.0 * (w_qkv.numel() + w_out.numel() + w_fc1.numel() + w_fc2.numel())):
    _lib.check(_lib.load().plm_ragged_layer_paged_wide_bf16(O._p(x), O._p(attn_norm_w), O._p(mlp_norm_w), float(eps), O._p(w_qkv), O._p(w_out),
                                                            O._p(w_fc1), O._p(w_fc2), O._p(lens0), O._p(cu_rows), O._p(row_seq), O._p(rope_cos),
                                                            O._p(rope_sin), rope_cos.shape[0], O._p(pool), pool.stride(1), O._p(table),
                                                            O._p(status), R, B, NT, Lcap, max_pages, n_pages, nh, hd, hidden, k, O._p(ws), nbytes,
                                                            stream), 'plm_ragged_layer_paged_wide_bf16')
  return x
