"""The ops wrappers of the fused decode step: ``ops.decode_norm_qkv_append``, ``ops.decode_gemm_residual``,
``ops.decode_norm_fc1_act`` (the three skinny-M stages) and ``ops.decode_layer`` (a whole decode layer from one library call); and of
the fused extend (section 18): ``ops.extend_norm_qkv_append`` (the qkv stage over chunk rows) and ``ops.extend_layer``.  A decode step is
a chunk of one row per sequence, so each decode / extend pair is one private function here, called with the pair member's name, entry
point and per-sequence operands.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract - the operand validator (``ops._need``), the launch
bracket (``ops._Launch``), the workspace arena of the current stream, ``_lib.check`` around the one library call - and, like every wrapper
there, launch hand-written gfx950 kernels with no torch fallback.  They live in a module of their own for ops_lookup.py's reason:
tests/test_ops_trace_host.py holds every function defined in ops.py to a trace recorded on an earlier commit."""

import torch

from . import _lib
from . import ops as O

FUSED_DECODE_MAX_ROWS = 32  # M of the skinny-M kernels; M = B of the plm_decode_* entry points: one decode token per sequence
FUSED_EXTEND_MAX_ROWS = FUSED_DECODE_MAX_ROWS  # M = B * n of the plm_extend_* entry points: n chunk rows per sequence
DECODE_MLP_KINDS = {'glu': 0, 'silu': 1, 'relu_sq': 2}  # PLM_DECODE_MLP_*


def _decode_operands(name, x, norms, weights):
  """The operand checks the fused ops share: x fp32 [M, d] with 1 <= M <= FUSED_DECODE_MAX_ROWS, fp32 [d] norm weights, contiguous bf16
  2-D weights.  Returns (M, d)."""
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
  if not 1 <= M <= FUSED_DECODE_MAX_ROWS:
    raise ValueError(f'{name}: {M} rows; the fused decode kernels take 1 to {FUSED_DECODE_MAX_ROWS} (one token per sequence)')
  return M, d


def _decode_mlp_kind(name, kind):
  if kind not in DECODE_MLP_KINDS:
    raise ValueError(f'{name}: mlp kind {kind!r} is not one of {sorted(DECODE_MLP_KINDS)}')
  return DECODE_MLP_KINDS[kind]


def _row_operands(name, M, hd, kv, lengths, rope_cos, rope_sin, nh, n, need_kv=None):
  """The operand checks of the ops that put M rows into a cache, beyond _decode_operands: the cache, the RoPE tables and ``lengths``, the
  op's per-sequence operands by name - int32 [B] each, None for one the caller left out (the library refuses a missing one it needs).
  n = 1: a decode op, one row per sequence, M = kv.shape[0]; n = None: a chunk op, M = kv.shape[0] * n.  Returns the row counts the op's
  entry point takes: (B,) of a decode op, (B, n) of a chunk op.  need_kv: another cache format's stand-in for ops._need_kv (ops_kv8.py)."""
  try:
    (need_kv or O._need_kv)(kv, nh, hd, 'kv')
    for what, t in lengths.items():
      if t is not None:
        O._need(t, torch.int32, what, 1)
    O._need(rope_cos, O.F32, 'rope_cos', 2)
    O._need(rope_sin, O.F32, 'rope_sin', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  B = kv.shape[0]
  if B < 1 or M % B != 0 or (n is not None and M != B * n) or any(t is not None and t.shape[0] != B for t in lengths.values()) or \
     rope_cos.shape != rope_sin.shape or rope_cos.shape[1] != hd // 2:
    shapes = ', '.join(f'{what} {None if t is None else tuple(t.shape)}' for what, t in lengths.items())
    raise ValueError(f'{name}: kv {tuple(kv.shape)}, {shapes} or the RoPE tables {tuple(rope_cos.shape)} / {tuple(rope_sin.shape)} do not fit '
                     f'{M} rows' + ('' if n is None else f' of {n} per sequence') + f', head_dim={hd}')
  return (B, M // B) if n is None else (B,)


def _norm_qkv_append(name, entry, x, norm_w, eps, w_qkv, lengths, rope_cos, rope_sin, kv, nh, q_out, status, n, need_kv=None):
  """Both qkv stages.  ``entry`` takes lengths' pointers where its row positions stand and, a chunk entry point (n = None), n after B.
  need_kv: as _row_operands takes it."""
  M, d = _decode_operands(name, x, (norm_w,), (w_qkv,))
  if d % nh != 0 or tuple(w_qkv.shape) != (3 * d, d):
    raise ValueError(f'{name}: x {tuple(x.shape)}, w_qkv {tuple(w_qkv.shape)} do not fit nh={nh}')
  hd = d // nh
  rows = _row_operands(name, M, hd, kv, lengths, rope_cos, rope_sin, nh, n, need_kv)
  q_out, status = O._append_outputs(name, x, M, d, q_out, status)
  with O._Launch('hbm:decode_fused', 2.0 * w_qkv.numel()):
    _lib.check(getattr(_lib.load(), entry)(O._p(x), O._p(norm_w), float(eps), O._p(w_qkv), *map(O._p, lengths.values()), O._p(rope_cos),
                                           O._p(rope_sin), rope_cos.shape[0], O._p(q_out), O._p(kv), kv.stride(1), O._p(status), *rows,
                                           kv.shape[1], nh, hd, O._stream()), entry)
  return q_out, status


def decode_norm_qkv_append(x, norm_w, eps, w_qkv, pos, rope_cos, rope_sin, kv, nh, q_out=None, status=None):
  """rmsnorm_fwd -> gemm_nt -> kv_append_rope of one decode step in one launch: x fp32 [B, d] (B <= FUSED_DECODE_MAX_ROWS), w_qkv bf16
  [3d, d].  Returns (rotated q bf16 [B, d], status); rotated k | v went into kv[b, pos[b]].  A pos[b] outside [0, min(Tmax, rope rows))
  stores nothing for that sequence, leaves a q row of zeros and sets status[0] = 1 (int32 [1], zeroed by the caller; made here when absent)."""
  return _norm_qkv_append('decode_norm_qkv_append', 'plm_decode_norm_qkv_append_bf16', x, norm_w, eps, w_qkv, {'pos': pos}, rope_cos, rope_sin,
                          kv, nh, q_out, status, 1)


def decode_gemm_residual(x, a, w):
  """x[M, N] += float(bf16(a[M, K] @ w[N, K]^T)) in place on the fp32 residual stream (gemm_nt and the add of the next norm in one launch);
  M <= FUSED_DECODE_MAX_ROWS.  Returns x."""
  name = 'decode_gemm_residual'
  M, N = _decode_operands(name, x, (), (a, w))
  if a.shape[0] != M or w.shape[0] != N or w.shape[1] != a.shape[1]:
    raise ValueError(f'{name}: x {tuple(x.shape)}, a {tuple(a.shape)}, w {tuple(w.shape)} do not fit')
  with O._Launch('hbm:decode_fused', 2.0 * w.numel()):
    _lib.check(_lib.load().plm_decode_gemm_residual_bf16(O._p(x), O._p(a), O._p(w), M, N, a.shape[1], O._stream()), 'plm_decode_gemm_residual_bf16')
  return x


def decode_norm_fc1_act(x, norm_w, eps, w_fc1, kind):
  """rmsnorm_fwd -> gemm_nt -> swiglu_fwd / act_fwd of one decode step in one launch: x fp32 [M, d], w_fc1 bf16 [2h, d] ('glu': gate | up)
  or [h, d] ('silu', 'relu_sq').  Returns the activation bf16 [M, h]."""
  name = 'decode_norm_fc1_act'
  M, d = _decode_operands(name, x, (norm_w,), (w_fc1,))
  k = _decode_mlp_kind(name, kind)
  mult = 2 if kind == 'glu' else 1
  if w_fc1.shape[1] != d or w_fc1.shape[0] % mult != 0:
    raise ValueError(f'{name}: x {tuple(x.shape)}, w_fc1 {tuple(w_fc1.shape)} do not fit kind {kind!r}')
  h = w_fc1.shape[0] // mult
  act = torch.empty((M, h), dtype=O.BF16, device=x.device)
  with O._Launch('hbm:decode_fused', 2.0 * w_fc1.numel()):
    _lib.check(_lib.load().plm_decode_norm_fc1_act_bf16(O._p(x), O._p(norm_w), float(eps), O._p(w_fc1), O._p(act), M, d, h, k, O._stream()),
               'plm_decode_norm_fc1_act_bf16')
  return act


def _layer_ws_bytes(name, query, rows, nh, hd, hidden, Tmax, splits):
  """The bytes ``query`` (a layer entry point's workspace query) asks for rows = (B,) | (B, n); a shape the library refuses raises."""
  nbytes = O._ws_bytes(query, *rows, nh, hd, hidden, Tmax, int(splits))
  if nbytes == 0:
    shape = ' '.join(f'{k}={v}' for k, v in zip('Bn', rows))
    raise ValueError(f'{name}: unsupported shape {shape} nh={nh} hd={hd} hidden={hidden} Tmax={Tmax} or splits={splits}')
  return nbytes


def _layer_workspace(name, query, rows, nh, hd, hidden, Tmax, splits, device):
  nbytes = _layer_ws_bytes(name, query, rows, nh, hd, hidden, Tmax, splits)
  return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _layer(name, entry, query, x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lengths, rope_cos, rope_sin, kv, nh, kind, status,
           splits, workspace, n, need_kv=None):
  """Both layers.  ``entry`` and ``query``, its workspace query, take what _norm_qkv_append's entry points take of lengths and n;
  need_kv as there."""
  M, d = _decode_operands(name, x, (attn_norm_w, mlp_norm_w), (w_qkv, w_out, w_fc1, w_fc2))
  k = _decode_mlp_kind(name, kind)
  hidden = w_fc2.shape[1]
  if d % nh != 0 or tuple(w_qkv.shape) != (3 * d, d) or tuple(w_out.shape) != (d, d) or w_fc2.shape[0] != d or \
     tuple(w_fc1.shape) != ((2 if kind == 'glu' else 1) * hidden, d):
    raise ValueError(f'{name}: the weights {tuple(w_qkv.shape)}, {tuple(w_out.shape)}, {tuple(w_fc1.shape)}, {tuple(w_fc2.shape)} do not fit '
                     f'x {tuple(x.shape)}, nh={nh}, kind {kind!r}')
  hd = d // nh
  rows = _row_operands(name, M, hd, kv, lengths, rope_cos, rope_sin, nh, n, need_kv)
  try:
    O._need(status, torch.int32, 'status')
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  Tmax = kv.shape[1]
  stream = O._stream()
  if workspace is not None:
    ws, nbytes = workspace
  else:
    nbytes = _layer_ws_bytes(name, query, rows, nh, hd, hidden, Tmax, splits)
    ws = O._workspace(x.device, nbytes, stream)
  with O._Launch('hbm:decode_fused', 2.0 * (w_qkv.numel() + w_out.numel() + w_fc1.numel() + w_fc2.numel())):
    _lib.check(getattr(_lib.load(), entry)(O._p(x), O._p(attn_norm_w), O._p(mlp_norm_w), float(eps), O._p(w_qkv), O._p(w_out), O._p(w_fc1),
                                           O._p(w_fc2), *map(O._p, lengths.values()), O._p(rope_cos), O._p(rope_sin), rope_cos.shape[0],
                                           O._p(kv), kv.stride(1), O._p(status), *rows, Tmax, nh, hd, hidden, k, int(splits), O._p(ws), nbytes,
                                           stream), entry)
  return x


def decode_layer_workspace(B, nh, hd, hidden, Tmax, splits, device):
  """A caller-owned (uint8 workspace, bytes) pair for decode_layer(..., workspace=) at this shape and splits argument."""
  return _layer_workspace('decode_layer', 'plm_decode_layer_workspace_bytes', (B,), nh, hd, hidden, Tmax, splits, device)


def decode_layer(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, pos, lens, rope_cos, rope_sin, kv, nh, kind, status, splits=0,
                 workspace=None):
  """One decode layer from one library call (six launches): decode_norm_qkv_append, attn_decode, decode_gemm_residual with w_out,
  decode_norm_fc1_act, decode_gemm_residual with w_fc2.  x fp32 [B, d] is updated in place and returned; status is the cache's int32 [1]
  flag; every intermediate lives in the workspace (the caller's pair of decode_layer_workspace for the same splits, else the stream's
  arena).  Shapes the kernels do not serve raise ValueError."""
  return _layer('decode_layer', 'plm_decode_layer_bf16', 'plm_decode_layer_workspace_bytes', x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1,
                w_fc2, {'pos': pos, 'lens': lens}, rope_cos, rope_sin, kv, nh, kind, status, splits, workspace, 1)


# ---- the fused extend: chunk rows on the same kernels ------------------------------------------------------------------
def extend_norm_qkv_append(x, norm_w, eps, w_qkv, lens0, rope_cos, rope_sin, kv, nh, n_new=None, q_out=None, status=None):
  """rmsnorm_fwd -> gemm_nt -> kv_append_rope_rows of a chunk in one launch: x fp32 [B*n, d] (B*n <= FUSED_EXTEND_MAX_ROWS; row b*n + r =
  chunk row r of sequence b, B = kv.shape[0]), w_qkv bf16 [3d, d], lens0 / n_new as kv_append_rope_rows takes them.  Returns (rotated q
  bf16 [B*n, d], status); rows r < n_new[b] went, rotated at lens0[b] + r, into kv[b, lens0[b] + r]; rows past n_new[b] and the rows of a
  sequence whose chunk does not fit (status[0] = 1) store nothing and leave zeros in q."""
  return _norm_qkv_append('extend_norm_qkv_append', 'plm_extend_norm_qkv_append_bf16', x, norm_w, eps, w_qkv, {'lens0': lens0, 'n_new': n_new},
                          rope_cos, rope_sin, kv, nh, q_out, status, None)


def extend_layer_workspace(B, n, nh, hd, hidden, Tmax, splits, device):
  """A caller-owned (uint8 workspace, bytes) pair for extend_layer(..., workspace=) at this shape (chunk width n) and splits argument."""
  return _layer_workspace('extend_layer', 'plm_extend_layer_workspace_bytes', (B, n), nh, hd, hidden, Tmax, splits, device)


def extend_layer(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, n_new, rope_cos, rope_sin, kv, nh, kind, status, splits=0,
                 workspace=None):
  """One layer over a chunk from one library call: extend_norm_qkv_append, attn_extend, decode_gemm_residual with w_out,
  decode_norm_fc1_act, decode_gemm_residual with w_fc2.  x fp32 [B*n, d] (B = kv.shape[0], B*n <= FUSED_EXTEND_MAX_ROWS) is updated in
  place and returned; n_new may be None; status is the cache's int32 [1] flag; every intermediate lives in the workspace (the caller's
  pair of extend_layer_workspace for the same splits, else the stream's arena).  Shapes the kernels do not serve raise ValueError."""
  return _layer('extend_layer', 'plm_extend_layer_bf16', 'plm_extend_layer_workspace_bytes', x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1,
                w_fc2, {'lens0': lens0, 'n_new': n_new}, rope_cos, rope_sin, kv, nh, kind, status, splits, workspace, None)
