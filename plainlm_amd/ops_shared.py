"""The ops wrappers of parallel sampling from one prompt: ``ops.attn_decode_shared`` (G samples per prompt attend
the prompt's prefix cache, held once, then their own suffix cache), ``ops.kv_append_rope_at`` (the append that stores at one row and
rotates at another position), ``ops.decode_norm_qkv_append_at`` (the fused qkv stage under that contract) and ``ops.decode_layer_shared``
(a whole decode layer over the two caches from one library call).

Operands: P prompts, G samples each; row i = p*G + g of every [P*G, ...] tensor is sample g of prompt p.  kv_p bf16 [P, Tp_max, 2*nh*hd]
with lens_p int32 [P] is the prefix cache, kv_s bf16 [P*G, Ts_max, 2*nh*hd] with lens_s int32 [P*G] the suffix cache, both in
ops.kv_append_rope's row layout.  bf16 caches only: an FP8 cache is refused.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract - the operand validator (``ops._need``), the launch
bracket (``ops._Launch``), the workspace arena of the current stream, ``_lib.check`` around the one library call - and, like every wrapper
there, launch hand-written gfx950 kernels with no torch fallback.  They live in a module of their own for ops_decode.py's reason."""

import torch

from . import _lib
from . import ops as O
from . import ops_decode as D


def _shared_operands(name, rows_dm, kv_p, lens_p, kv_s, lens_s, nh, hd):
  """The two caches and their lengths against rows_dm = (P*G, nh*hd); returns (P, G)."""
  try:
    for what, kv in (('kv_p', kv_p), ('kv_s', kv_s)):
      if isinstance(kv, torch.Tensor) and kv.dtype == torch.uint8:
        raise TypeError(f'{what}: an FP8 cache is not served by the shared-prefix kernels (bf16 caches only)')
      O._need_kv(kv, nh, hd, what)
    O._need(lens_p, torch.int32, 'lens_p', 1)
    O._need(lens_s, torch.int32, 'lens_s', 1)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  M, P = rows_dm[0], kv_p.shape[0]
  if P < 1 or M < P or M % P != 0 or kv_s.shape[0] != M or lens_p.shape[0] != P or lens_s.shape[0] != M or rows_dm[1] != nh * hd:
    raise ValueError(f'{name}: {M} rows of {rows_dm[1]}, kv_p {tuple(kv_p.shape)}, lens_p {tuple(lens_p.shape)}, kv_s {tuple(kv_s.shape)}, lens_s '
                     f'{tuple(lens_s.shape)} do not fit nh={nh}, hd={hd} (kv_s and lens_s hold P*G sequences, row p*G + g = sample g of prompt p)')
  return P, M // P


def attn_decode_shared_workspace_bytes(P, G, nh, hd, Tp_max, Ts_max, splits_p=0, splits_s=0):
  """Workspace bytes of attn_decode_shared at this shape and these splits arguments; a shape the library refuses raises."""
  nbytes = O._ws_bytes('plm_attn_decode_shared_workspace_bytes', P, G, nh, hd, Tp_max, Ts_max, int(splits_p), int(splits_s))
  if nbytes == 0:
    raise ValueError(f'attn_decode_shared: unsupported shape P={P} G={G} nh={nh} hd={hd} Tp_max={Tp_max} Ts_max={Ts_max} or splits_p={splits_p} / '
                     f'splits_s={splits_s} (0 = automatic, 1..64)')
  return nbytes


def attn_decode_shared(q, kv_p, lens_p, kv_s, lens_s, nh, splits_p=0, splits_s=0, want_lse=False):
  """Attention of one rotated query row per sample over its prompt's prefix and its own suffix: q bf16 [P*G, nh*hd]; sample i = p*G + g
  attends keys 0 .. lens_p[p]-1 of kv_p[p], then keys 0 .. lens_s[i]-1 of kv_s[i] (both lens clamped on the device; rows beyond them are
  never read; both 0 give out = 0, lse = +inf).  Every prefix row is read once per 32 samples of the prompt.  splits_p / splits_s: 0
  automatic (from the shapes alone) | 1..64 forced.  Returns out bf16 [P*G, nh*hd], or (out, lse fp32 [P*G, nh], base 2) with want_lse."""
  name = 'attn_decode_shared'
  try:
    O._need(q, O.BF16, 'q', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  if q.shape[1] % nh != 0:
    raise ValueError(f'{name}: q {tuple(q.shape)} does not fit nh={nh}')
  hd = q.shape[1] // nh
  P, G = _shared_operands(name, tuple(q.shape), kv_p, lens_p, kv_s, lens_s, nh, hd)
  Tp, Ts = kv_p.shape[1], kv_s.shape[1]
  nbytes = attn_decode_shared_workspace_bytes(P, G, nh, hd, Tp, Ts, splits_p, splits_s)
  stream = O._stream()
  ws = O._workspace(q.device, nbytes, stream)
  out = torch.empty((P * G, nh * hd), dtype=O.BF16, device=q.device)
  lse = torch.empty((P * G, nh), dtype=O.F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_decode_shared(O._p(q), O._p(kv_p), kv_p.stride(1), O._p(lens_p), O._p(kv_s), kv_s.stride(1), O._p(lens_s),
                                                O._p(out), O._p(lse), P, G, Tp, Ts, nh, hd, int(splits_p), int(splits_s), O._p(ws), nbytes, stream),
             'plm_attn_decode_shared')
  return (out, lse) if want_lse else out


def _need_rot0(name, rot0, B):
  try:
    O._need(rot0, torch.int32, 'rot0', 1)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  if rot0.shape[0] != B:
    raise ValueError(f'{name}: rot0 {tuple(rot0.shape)} does not fit the batch of {B}')


def kv_append_rope_at(qkv, row, rot0, rope_cos, rope_sin, kv, nh, q_out=None, status=None):
  """ops.kv_append_rope with the cache row and the RoPE position told apart: sequence b's token is rotated at position rot0[b] + row[b]
  and stored in kv[b, row[b]] (row, rot0 int32 [B]).  A row outside [0, Tmax) or a position outside the RoPE table stores nothing for that
  sequence, leaves a q_out row of zeros and sets status[0] = 1.  Returns (q_out, status)."""
  B, _, hd = O._cached_operands('kv_append_rope_at', qkv, 3, kv, nh, row, 'row', False, rope=(rope_cos, rope_sin))
  _need_rot0('kv_append_rope_at', rot0, B)
  q_out, status = O._append_outputs('kv_append_rope_at', qkv, B, nh * hd, q_out, status)
  _lib.check(_lib.load().plm_kv_append_rope_at(O._p(qkv), qkv.stride(0), O._p(row), O._p(rot0), O._p(rope_cos), O._p(rope_sin), rope_cos.shape[0],
                                               O._p(q_out), O._p(kv), kv.stride(1), O._p(status), B, kv.shape[1], nh, hd, O._stream()),
             'plm_kv_append_rope_at')
  return q_out, status


def decode_norm_qkv_append_at(x, norm_w, eps, w_qkv, row, rot0, rope_cos, rope_sin, kv, nh, q_out=None, status=None):
  """ops.decode_norm_qkv_append under kv_append_rope_at's contract: rmsnorm_fwd -> gemm_nt -> kv_append_rope_at in one launch.  Returns
  (rotated q bf16 [B, d], status); rotated k | v went into kv[b, row[b]], rotated at rot0[b] + row[b]."""
  return D._norm_qkv_append('decode_norm_qkv_append_at', 'plm_decode_norm_qkv_append_at_bf16', x, norm_w, eps, w_qkv, {'row': row, 'rot0': rot0},
                            rope_cos, rope_sin, kv, nh, q_out, status, 1)


def decode_layer_shared(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, row, lens_s, rot0, lens_p, rope_cos, rope_sin, kv_p, kv_s, nh,
                        kind, status, splits_p=0, splits_s=0):
  """ops.decode_layer for P*G <= FUSED_DECODE_MAX_ROWS samples over a shared prefix, one library call (seven launches):
  decode_norm_qkv_append_at into the suffix cache (row, rot0), attn_decode_shared (lens_p; lens_s = row + 1 during a step),
  decode_gemm_residual with w_out, decode_norm_fc1_act, decode_gemm_residual with w_fc2.  x fp32 [P*G, d] is updated in place and returned."""
  return _layer_two_caches('decode_layer_shared', 'plm_decode_layer_shared', x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, row, lens_s,
                           rot0, lens_p, (), rope_cos, rope_sin, kv_p, kv_s, nh, kind, status, splits_p, splits_s)


def _layer_two_caches(name, sym, x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, row, lens_s, rot0, lens_p, anc, rope_cos, rope_sin, kv_p,
                      kv_s, nh, kind, status, splits_p, splits_s):
  """decode_layer_shared and ops_beam.decode_layer_beam: the entry points ``sym``_bf16 / ``sym``_workspace_bytes differ by the operands ``anc``
  (none, or the beam layer's ancestor table) behind lens_p."""
  M, d = D._decode_operands(name, x, (attn_norm_w, mlp_norm_w), (w_qkv, w_out, w_fc1, w_fc2))
  k = D._decode_mlp_kind(name, kind)
  hidden = w_fc2.shape[1]
  if d % nh != 0 or tuple(w_qkv.shape) != (3 * d, d) or tuple(w_out.shape) != (d, d) or w_fc2.shape[0] != d or \
     tuple(w_fc1.shape) != ((2 if kind == 'glu' else 1) * hidden, d):
    raise ValueError(f'{name}: the weights {tuple(w_qkv.shape)}, {tuple(w_out.shape)}, {tuple(w_fc1.shape)}, {tuple(w_fc2.shape)} do not fit '
                     f'x {tuple(x.shape)}, nh={nh}, kind {kind!r}')
  hd = d // nh
  P, G = _shared_operands(name, (M, d), kv_p, lens_p, kv_s, lens_s, nh, hd)
  D._row_operands(name, M, hd, kv_s, {'row': row, 'rot0': rot0}, rope_cos, rope_sin, nh, 1)
  try:
    O._need(status, torch.int32, 'status')
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  Tp, Ts = kv_p.shape[1], kv_s.shape[1]
  nbytes = O._ws_bytes(sym + '_workspace_bytes', P, G, nh, hd, hidden, Tp, Ts, int(splits_p), int(splits_s))
  if nbytes == 0:
    raise ValueError(f'{name}: unsupported shape P={P} G={G} nh={nh} hd={hd} hidden={hidden} Tp_max={Tp} Ts_max={Ts} or splits_p={splits_p} / '
                     f'splits_s={splits_s}')
  stream = O._stream()
  ws = O._workspace(x.device, nbytes, stream)
  with O._Launch('hbm:decode_fused', 2.0 * (w_qkv.numel() + w_out.numel() + w_fc1.numel() + w_fc2.numel())):
    _lib.check(getattr(_lib.load(), sym + '_bf16')(
        O._p(x), O._p(attn_norm_w), O._p(mlp_norm_w), float(eps), O._p(w_qkv), O._p(w_out), O._p(w_fc1), O._p(w_fc2), O._p(row), O._p(lens_s),
        O._p(rot0), O._p(lens_p), *[O._p(a) for a in anc], O._p(rope_cos), O._p(rope_sin), rope_cos.shape[0], O._p(kv_p), kv_p.stride(1), O._p(kv_s),
        kv_s.stride(1), O._p(status), P, G, Tp, Ts, nh, hd, hidden, k, int(splits_p), int(splits_s), O._p(ws), nbytes, stream), sym + '_bf16')
  return x
