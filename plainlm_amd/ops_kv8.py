"""The ops wrappers of the FP8 KV cache: ``ops.kv8_quant_rows`` / ``ops.kv8_dequant_rows`` (bf16 k | v rows to
cache rows and back), ``ops.kv8_append_rope_rows`` (the append of a chunk, a decode step at n = 1), ``ops.attn_decode_kv8`` /
``ops.attn_extend_kv8`` (the two attention kernels over this cache) and the fused wrappers ``ops.extend_norm_qkv_append_kv8``,
``ops.decode_layer_kv8``, ``ops.extend_layer_kv8``.

A cache is uint8 [B, Tmax, row_bytes], row = k codes dm | v codes dm | k scales dm/16 | v scales dm/16 (dm = nh*hd): OCP e4m3fn codes
under one E8M0 scale per 16 elements of a head, 0.53 of the bf16 cache's bytes.  Dequantisation is exact, so every attention op here
returns, bit for bit, what its bf16 twin returns on ``kv8_dequant_rows`` of the cache.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract - the operand validator (``ops._need``), the launch
bracket (``ops._Launch``), the workspace arena of the current stream, ``_lib.check`` around the one library call - and, like every wrapper
there, launch hand-written gfx950 kernels with no torch fallback.  They live in a module of their own for ops_decode.py's reason:
tests/test_ops_trace_host.py holds every function defined in ops.py to a trace recorded on an earlier commit."""

import torch

from . import _lib
from . import ops as O
from . import ops_decode as D

U8 = torch.uint8
KV8_BLOCK = 16  # elements of a head under one scale byte


def kv8_row_bytes(dm):
  """Bytes of a cache row for dm = nh*hd: 2*dm codes and dm/8 scale bytes, rounded up to the 16 the row stride must be a multiple of."""
  return (2 * dm + dm // 8 + 15) // 16 * 16


def _need_kv8(kv, nh, hd, name='kv8'):
  """kv uint8 [B, Tmax, kv8_row_bytes(nh*hd)]: rows may be padded (stride(1) a multiple of 16), sequences are Tmax rows apart."""
  if not kv.is_cuda:
    raise RuntimeError(f'{name}: tensor must live on the GPU (plainlm_amd has no CPU path)')
  if kv.dtype != U8 or kv.dim() != 3 or kv.shape[2] != kv8_row_bytes(nh * hd) or kv.stride(2) != 1 or kv.stride(1) % 16 != 0 or \
     kv.stride(0) != kv.shape[1] * kv.stride(1):
    raise ValueError(f'{name}: need a uint8 [B, Tmax, {kv8_row_bytes(nh * hd)}] FP8 cache (nh={nh}, hd={hd}) with unit inner stride, a row '
                     f'stride that is a multiple of 16 and batch stride Tmax * row stride')
  return kv


def _rows_operands(name, rows, kv, nh):
  """bf16 k | v rows [B, T, 2*nh*hd] (unit inner stride, row stride free, batch stride T * row stride) against a cache: (B, T, hd)."""
  if not rows.is_cuda:
    raise RuntimeError(f'{name}.rows: tensor must live on the GPU (plainlm_amd has no CPU path)')
  if rows.dtype != O.BF16 or rows.dim() != 3 or rows.shape[2] % (2 * nh) != 0 or rows.stride(2) != 1 or \
     rows.stride(0) != rows.shape[1] * rows.stride(1):
    raise ValueError(f'{name}: need bf16 k | v rows [B, T, 2*nh*hd] with unit inner stride and batch stride T * row stride')
  hd = rows.shape[2] // (2 * nh)
  try:
    _need_kv8(kv, nh, hd)
  except (RuntimeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  B, T = rows.shape[:2]
  if kv.shape[0] != B or not 1 <= T <= kv.shape[1]:
    raise ValueError(f'{name}: rows {tuple(rows.shape)} do not fit the cache {tuple(kv.shape)}')
  return B, T, hd


def kv8_quant_rows(rows, kv, nh):
  """Quantise bf16 k | v rows [B, T, 2*nh*hd] (k already rotated; a column slice of the rotated qkv is fine) into rows 0 .. T-1 of every
  sequence of the FP8 cache kv: a prefill's write.  Returns kv."""
  B, T, hd = _rows_operands('kv8_quant_rows', rows, kv, nh)
  with O._Launch('hbm:kv8', 2.0 * rows.numel()):
    _lib.check(_lib.load().plm_kv8_quant_rows(O._p(rows), rows.stride(1), O._p(kv), kv.stride(1), B, T, kv.shape[1], nh, hd, O._stream()),
               'plm_kv8_quant_rows')
  return kv


def kv8_dequant_rows(kv, nh, hd, T=None, out=None):
  """Rows 0 .. T-1 (default: all Tmax) of every sequence of the FP8 cache kv as bf16 [B, T, 2*nh*hd]: code * 2^(scale - 127), exact.
  out: the caller's bf16 [B, T, 2*nh*hd] (as kv8_quant_rows takes its rows: a column slice of a wider buffer is fine), which sets T."""
  _need_kv8(kv, nh, hd, 'kv8_dequant_rows.kv8')
  B, Tmax = kv.shape[:2]
  if out is not None:
    if _rows_operands('kv8_dequant_rows', out, kv, nh)[2] != hd:
      raise ValueError(f'kv8_dequant_rows: out {tuple(out.shape)} does not fit nh={nh}, hd={hd}')
    T = out.shape[1]
  T = Tmax if T is None else int(T)
  if not 1 <= T <= Tmax:
    raise ValueError(f'kv8_dequant_rows: T={T} outside [1, {Tmax}]')
  if out is None:
    out = torch.empty((B, T, 2 * nh * hd), dtype=O.BF16, device=kv.device)
  with O._Launch('hbm:kv8', 2.0 * out.numel()):
    _lib.check(_lib.load().plm_kv8_dequant_rows(O._p(kv), kv.stride(1), O._p(out), out.stride(1), B, T, Tmax, nh, hd, O._stream()),
               'plm_kv8_dequant_rows')
  return out


def kv8_append_rope_rows(qkv, lens0, rope_cos, rope_sin, kv, nh, n_new=None, q_out=None, status=None):
  """ops.kv_append_rope_rows over an FP8 cache: the same arguments, refusals, q_out bits and status; the rotated k | v rows are quantised
  into kv[b, lens0[b] + r].  A decode step is a chunk of one row per sequence: qkv [B, 3*nh*hd], lens0 = the positions, n_new = None."""
  B, n, hd = O._cached_operands('kv8_append_rope_rows', qkv, 3, kv, nh, lens0, 'lens0', True, n_new=n_new, rope=(rope_cos, rope_sin),
                                  need_kv=_need_kv8)
  q_out, status = O._append_outputs('kv8_append_rope_rows', qkv, B * n, nh * hd, q_out, status)
  _lib.check(_lib.load().plm_kv8_append_rope_rows(O._p(qkv), qkv.stride(0), O._p(lens0), O._p(n_new), O._p(rope_cos), O._p(rope_sin),
                                                  rope_cos.shape[0], O._p(q_out), O._p(kv), kv.stride(1), O._p(status), B, n, kv.shape[1], nh,
                                                  hd, O._stream()), 'plm_kv8_append_rope_rows')
  return q_out, status


def attn_decode_kv8(q, kv, lens, nh, splits=0, want_lse=False, workspace=None):
  """ops.attn_decode over an FP8 cache: the same arguments, split rule and workspace (ops.attn_decode_workspace); bit for bit what
  ops.attn_decode returns on kv8_dequant_rows(kv) for the same splits."""
  B, _, hd = O._cached_operands('attn_decode_kv8', q, 1, kv, nh, lens, 'lens', False, need_kv=_need_kv8)
  Tmax = kv.shape[1]
  ws, nbytes, stream = O._cached_workspace('attn_decode', B, 1, nh, hd, Tmax, splits, q.device, workspace)
  out = torch.empty((B, nh * hd), dtype=O.BF16, device=q.device)
  lse = torch.empty((B, nh), dtype=O.F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_decode_kv8(O._p(q), O._p(kv), kv.stride(1), O._p(lens), O._p(out), O._p(lse), B, Tmax, nh, hd, int(splits),
                                             O._p(ws), nbytes, stream), 'plm_attn_decode_kv8')
  return (out, lse) if want_lse else out


def attn_extend_kv8(q, kv, lens0, nh, n_new=None, splits=0, want_lse=False, workspace=None):
  """ops.attn_extend over an FP8 cache: the same arguments, split rule and workspace (ops.attn_extend_workspace); bit for bit what
  ops.attn_extend returns on kv8_dequant_rows(kv) for the same splits."""
  B, n, hd = O._cached_operands('attn_extend_kv8', q, 1, kv, nh, lens0, 'lens0', True, n_new=n_new, need_kv=_need_kv8)
  Tmax = kv.shape[1]
  ws, nbytes, stream = O._cached_workspace('attn_extend', B, n, nh, hd, Tmax, splits, q.device, workspace)
  out = torch.empty((B * n, nh * hd), dtype=O.BF16, device=q.device)
  lse = torch.empty((B, nh, n), dtype=O.F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_extend_kv8(O._p(q), O._p(kv), kv.stride(1), O._p(lens0), O._p(n_new), O._p(out), O._p(lse), B, n, Tmax, nh, hd,
                                             int(splits), O._p(ws), nbytes, stream), 'plm_attn_extend_kv8')
  return (out, lse) if want_lse else out


# ---- the fused stage and layers (DESIGN.md sections 17, 18 and 20): ops_decode's private functions with the FP8 cache's operand check ------
def extend_norm_qkv_append_kv8(x, norm_w, eps, w_qkv, lens0, rope_cos, rope_sin, kv, nh, n_new=None, q_out=None, status=None):
  """ops.extend_norm_qkv_append over an FP8 cache: the same rounding points, rotation and q_out bits; the bf16 k | v values that op would
  store are quantised into kv[b, lens0[b] + r] by the same launch.  The decode stage is this one at n = 1 (lens0 = the positions)."""
  return D._norm_qkv_append('extend_norm_qkv_append_kv8', 'plm_extend_norm_qkv_append_kv8_bf16', x, norm_w, eps, w_qkv,
                            {'lens0': lens0, 'n_new': n_new}, rope_cos, rope_sin, kv, nh, q_out, status, None, need_kv=_need_kv8)


def decode_layer_kv8(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, pos, lens, rope_cos, rope_sin, kv, nh, kind, status, splits=0,
                     workspace=None):
  """ops.decode_layer over an FP8 cache: one library call, six launches, ops.decode_layer_workspace's workspace."""
  return D._layer('decode_layer_kv8', 'plm_decode_layer_kv8_bf16', 'plm_decode_layer_workspace_bytes', x, attn_norm_w, mlp_norm_w, eps, w_qkv,
                  w_out, w_fc1, w_fc2, {'pos': pos, 'lens': lens}, rope_cos, rope_sin, kv, nh, kind, status, splits, workspace, 1,
                  need_kv=_need_kv8)


def extend_layer_kv8(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, n_new, rope_cos, rope_sin, kv, nh, kind, status, splits=0,
                     workspace=None):
  """ops.extend_layer over an FP8 cache: one library call, ops.extend_layer_workspace's workspace."""
  return D._layer('extend_layer_kv8', 'plm_extend_layer_kv8_bf16', 'plm_extend_layer_workspace_bytes', x, attn_norm_w, mlp_norm_w, eps, w_qkv,
                  w_out, w_fc1, w_fc2, {'lens0': lens0, 'n_new': n_new}, rope_cos, rope_sin, kv, nh, kind, status, splits, workspace, None,
                  need_kv=_need_kv8)
