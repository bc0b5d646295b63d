"""Tensor-level wrappers over the C ABI: validate, allocate outputs with torch (the caching
allocator owns all memory), pass raw device pointers + the current HIP stream.

Every function here launches hand-written gfx950 kernels; none has a torch fallback.
"""

import collections
import ctypes as C

import torch

from . import _lib

BF16 = torch.bfloat16
F32 = torch.float32
_DTYPE_NAMES = {BF16: 'bf16', F32: 'fp32'}


def _stream():
  return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Optional per-launch timing used by bench.py's roofline leg: when PROFILE is a list, every MFMA kernel launch - and every launch of the
# HBM-bound kernels, whose family names start with 'hbm:' and whose work figure is ALGORITHMIC BYTES instead of
# flops - is bracketed by HIP events on the launch stream and (family, work, start, end) appended.
PROFILE = None
# Called with (family, flops) right before every MFMA kernel launch when set (ddp.GradReducer: it keeps an estimate of the GPU time
# enqueued so far and reserves CUs for RCCL only while a gradient bucket's collective is expected to be running).
LAUNCH_HOOK = None


class _Launch:
  """One launch's (family, work), stated once.  Constructing it reports an MFMA launch to LAUNCH_HOOK (the 'hbm:' families are not
  reported), so construct it BEFORE the call's workspace query: the hook may change the CU reserve, and plans (tile shape, stream-K /
  split-K workspace) are functions of it.  Entered, it brackets the launch with events for PROFILE."""
  __slots__ = ('family', 'work', 'start')

  def __init__(self, family, work):
    self.family, self.work, self.start = family, work, None
    if LAUNCH_HOOK is not None and not family.startswith('hbm:'):
      LAUNCH_HOOK(family, work)

  def __enter__(self):
    if PROFILE is not None:
      self.start = torch.cuda.Event(enable_timing=True)
      self.start.record()
    return self

  def __exit__(self, *exc):
    if self.start is not None:
      end = torch.cuda.Event(enable_timing=True)
      end.record()
      PROFILE.append((self.family, self.work, self.start, end))
    return False


def _p(t):
  return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _need(t, dtype, name, dim=None, strided=False):
  """The operand contract: a GPU tensor of this dtype, contiguous (and of ``dim`` dims when given) - or, with strided, 2-D with unit
  inner stride, its rows any distance apart (a column slice of a wider buffer)."""
  if not t.is_cuda:
    raise RuntimeError(f'{name}: tensor must live on the GPU (plainlm_amd has no CPU path)')
  if strided:
    if t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1:
      raise ValueError(f'{name}: need a 2-D {_DTYPE_NAMES[dtype]} GPU tensor with unit inner stride')
    return t
  if t.dtype != dtype:
    raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
  if not t.is_contiguous():
    raise ValueError(f'{name}: tensor must be contiguous')
  if dim is not None and t.dim() != dim:
    raise ValueError(f'{name}: expected {dim} dims, got {t.dim()}')
  return t


def _need_shadows(dst, dst_t, R, Cc, name, on_gpu=True):
  """The bf16 copies of an fp32 [R, C] weight: dst contiguous [R, C] (None: made by the caller, not checked), dst_t [C, >= R] with unit
  inner stride (its rows may be padded: K-padding for the dX GEMM)."""
  if dst is not None and (dst.dtype != BF16 or tuple(dst.shape) != (R, Cc) or not dst.is_contiguous() or not dst.is_cuda):
    raise ValueError(f'{name}: need contiguous bf16 [rows, cols] on the GPU')
  if dst_t.dtype != BF16 or dst_t.dim() != 2 or dst_t.shape[0] != Cc or dst_t.shape[1] < R or dst_t.stride(1) != 1 or \
     (on_gpu and not dst_t.is_cuda):
    raise ValueError(f'{name}_t: need bf16 [cols, >= rows]' + (' on the GPU' if on_gpu else ''))


# ---- workspaces -------------------------------------------------------------------
# Every workspace (split-K / stream-K slabs, the heads' and the decode / extend partials, the embedding sort) is used on the current stream
# and dead when its wrapper returns: the reduce that reads it runs inside the entry point that filled it, and none reads a byte it did not
# write (tests/footprint.py).  So one grow-only buffer per (device, stream) serves all: the largest request is held, not the sum over shapes.
_arenas = {}    # (device, stream handle) -> uint8 buffer
_ws_sizes = {}  # (size query, its arguments, CU reserve, env epoch) -> bytes


def _workspace(device, nbytes, stream):
  """nbytes of scratch for one launch on ``stream`` (what _stream() gave): the arena of that device and stream, grown when too small."""
  key = (device, stream.value)
  buf = _arenas.get(key)
  if buf is None or buf.numel() < nbytes:
    del buf
    _arenas.pop(key, None)  # the old buffer goes back to the allocator before the larger one is asked for
    buf = _arenas[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
  return buf


def release_workspaces():
  """Drop every workspace arena (torch's caching allocator gets the memory back); the next launch that needs one allocates again."""
  _arenas.clear()


def workspace_bytes():
  """Bytes held by the workspace arenas of all devices and streams."""
  return sum(buf.numel() for buf in _arenas.values())


def _ws_bytes(query, *shape):
  """The answer of a library size query, cached: the plan behind it depends on the shape, the library's environment switches (see
  reload_env) and the CU reserve - all part of the key."""
  key = (query, shape, _cu_reserve, _env_epoch)
  v = _ws_sizes.get(key)
  if v is None:
    v = _ws_sizes[key] = int(getattr(_lib.load(), query)(*shape))
  return v


_cu_reserve = 0


def set_cu_reserve(n):
  """Leave n CUs out of the persistent GEMM grids (RCCL's kernels run there while gradient buckets are in flight); every
  plan (tile shape, hybrid stream-K, split-K) is recomputed per launch from the current value."""
  global _cu_reserve
  _lib.check(_lib.load().plm_set_cu_reserve(int(n)), 'plm_set_cu_reserve')
  _cu_reserve = int(n)


def cu_reserve():
  return _cu_reserve


_env_epoch = 0


def reload_env():
  """Have the library read its PLM_* environment switches again (it reads them once, at its first call; tests and A/B tools
  that change os.environ afterwards call this)."""
  global _env_epoch
  _lib.load().plm_reload_env()
  _env_epoch += 1


# ---- casts ------------------------------------------------------------------
def cast_bf16(src, out=None):
  _need(src, F32, 'cast_bf16.src')
  out = torch.empty(src.shape, dtype=BF16, device=src.device) if out is None else out
  _lib.check(_lib.load().plm_cast_f32_bf16(_p(src), _p(out), src.numel(), _stream()), 'plm_cast_f32_bf16')
  return out


def cast_bf16_t(src, out=None, out_t=None):
  """src fp32 [R, C] -> (bf16 [R, C], bf16 [C, R]).  ``out_t`` may be a zero-initialised [C, R_pad] buffer
  (R_pad >= R): only its first R columns are written, the pad stays zero (K-padding for the dX GEMM)."""
  _need(src, F32, 'cast_bf16_t.src', 2)
  R, Cc = src.shape
  out = torch.empty((R, Cc), dtype=BF16, device=src.device) if out is None else out
  out_t = torch.empty((Cc, R), dtype=BF16, device=src.device) if out_t is None else out_t
  _need_shadows(None, out_t, R, Cc, 'cast_bf16_t.out', on_gpu=False)
  _lib.check(_lib.load().plm_cast_f32_bf16_t(_p(src), _p(out), _p(out_t), R, Cc, out_t.stride(0), _stream()),
             'plm_cast_f32_bf16_t')
  return out, out_t


def cast_bf16_t_multi(items):
  """[(src fp32 [R, C], out bf16 [R, C], out_t bf16 [C, >= R])]: cast_bf16_t for all of them in one launch."""
  if not items:
    return
  arr = (_lib.CastItem * len(items))()
  for i, (src, out, out_t) in enumerate(items):
    _need(src, F32, 'cast_bf16_t_multi.src', 2)
    R, Cc = src.shape
    _need_shadows(out, out_t, R, Cc, 'cast_bf16_t_multi.out')
    arr[i] = _lib.CastItem(src.data_ptr(), out.data_ptr(), out_t.data_ptr(), R, Cc, out_t.stride(0))
  with _Launch('hbm:cast_bf16_t_multi', 8.0 * sum(src.numel() for src, _, _ in items)):  # one fp32 read, the bf16 copy and its transpose written
    _lib.check(_lib.load().plm_cast_f32_bf16_t_multi(arr, len(items), _stream()), 'plm_cast_f32_bf16_t_multi')


# ---- MXFP8 operands and GEMM --------------------------------------------------------------------------------
def mx_pad(k):
  """Padded reduction length of an MX operand: roundup(k, 128)."""
  return (int(k) + 127) // 128 * 128


class MxTensor:
  """One MX-quantized GEMM operand blocked along its reduction dimension: ``data`` uint8 [rows, Kp] (OCP e4m3fn bits), ``scales`` uint8
  [rows, Kp/32] (E8M0 bytes: 2^(byte - 127)), ``shape`` the logical (rows, K) with Kp = roundup(K, 128); the padding is zero."""
  __slots__ = ('data', 'scales', 'shape')

  def __init__(self, data, scales, shape):
    self.data, self.scales, self.shape = data, scales, tuple(shape)

  def nbytes(self):
    return self.data.numel() + self.scales.numel()

  @staticmethod
  def empty(rows, k, device):
    kp = mx_pad(k)
    return MxTensor(torch.empty((rows, kp), dtype=torch.uint8, device=device), torch.empty((rows, kp // 32), dtype=torch.uint8, device=device),
                    (rows, k))


def _mx_item(x, rows, cols, device):
  _need(x, BF16, 'mx_quant.x', strided=True)
  R, Cc = x.shape
  r = MxTensor.empty(R, Cc, x.device) if rows else None
  c = MxTensor.empty(Cc, R, x.device) if cols else None
  item = _lib.MxQuantItem(x.data_ptr(), x.stride(0), R, Cc, r.data.data_ptr() if r else 0, r.scales.data_ptr() if r else 0,
                          c.data.data_ptr() if c else 0, c.scales.data_ptr() if c else 0)
  return item, r, c


def mx_quant(x, rows=True, cols=True):
  """bf16 x [R, C] -> (row-blocked MxTensor of shape (R, C) blocked along C, or None; column-blocked MxTensor of x^T, shape (C, R) blocked
  along R, or None), from one read of x.  The row-blocked copy is the operand of a GEMM reducing over C, the other of one reducing over R."""
  if not (rows or cols):
    raise ValueError('mx_quant: ask for at least one orientation')
  item, r, c = _mx_item(x, rows, cols, x.device)
  with _Launch('hbm:mx_quant', 2.0 * x.numel() + (1.03125 * x.numel() if rows else 0) + (1.03125 * x.numel() if cols else 0)):
    _lib.check(_lib.load().plm_mx_quant(item.x, item.ld, item.rows, item.cols, item.q, item.s, item.qt, item.st, _stream()), 'plm_mx_quant')
  return r, c


def mx_quant_multi(xs, rows=True, cols=True):
  """mx_quant over a list of bf16 tensors in one launch (per 64): a list of (row-blocked, column-blocked) pairs."""
  if not xs:
    return []
  arr = (_lib.MxQuantItem * len(xs))()
  out = []
  for i, x in enumerate(xs):
    arr[i], r, c = _mx_item(x, rows, cols, x.device)
    out.append((r, c))
  n = sum(x.numel() for x in xs)
  with _Launch('hbm:mx_quant_multi', 2.0 * n + 1.03125 * n * (int(rows) + int(cols))):
    _lib.check(_lib.load().plm_mx_quant_multi(arr, len(xs), _stream()), 'plm_mx_quant_multi')
  return out


def gemm_mx_nt(a, b, out=None, accumulate=False, out_dtype=BF16):
  """C[M,N] (+)= deq(a)[M,K] @ deq(b)[N,K]^T for MxTensors a, b blocked along the same K; fp32 accumulation.  out_dtype bf16 (store) or fp32
  (store, or += into ``out`` with accumulate=True)."""
  if not isinstance(a, MxTensor) or not isinstance(b, MxTensor):
    raise TypeError('gemm_mx_nt: a and b must be MxTensors (ops.mx_quant)')
  M, K = a.shape
  N = b.shape[0]
  if b.shape[1] != K or a.data.shape[1] != b.data.shape[1]:
    raise ValueError(f'gemm_mx_nt: reduction lengths differ ({K} vs {b.shape[1]})')
  if out is None:
    if accumulate:
      raise ValueError('gemm_mx_nt: accumulate needs out')
    out = torch.empty((M, N), dtype=out_dtype, device=a.data.device)
  if out.dim() != 2 or out.shape != (M, N) or out.stride(1) != 1 or not out.is_cuda:
    raise ValueError('gemm_mx_nt.out: bad shape/stride')
  if out.dtype == BF16:
    if accumulate:
      raise ValueError('gemm_mx_nt: accumulate needs an fp32 out')
    mode = _lib.MX_OUT_BF16
  elif out.dtype == F32:
    mode = _lib.MX_OUT_F32_ACC if accumulate else _lib.MX_OUT_F32
  else:
    raise TypeError(f'gemm_mx_nt.out: bf16 or fp32, got {out.dtype}')
  with _Launch('gemm_mx_nt', 2.0 * M * N * K):
    _lib.check(_lib.load().plm_gemm_mx_nt(_p(a.data), _p(a.scales), _p(b.data), _p(b.scales), _p(out), out.stride(0), M, N, a.data.shape[1],
                                          mode, _stream()), 'plm_gemm_mx_nt')
  return out


# ---- embedding ----------------------------------------------------------------
def embed_fwd(ids, W):
  _need(ids, torch.int64, 'embed_fwd.ids')
  _need(W, F32, 'embed_fwd.W', 2)
  M = ids.numel()
  out = torch.empty((M, W.shape[1]), dtype=F32, device=W.device)
  with _Launch('hbm:embed_fwd', 8.0 * M * W.shape[1] + 8.0 * M):
    _lib.check(_lib.load().plm_embed_fwd(_p(ids), _p(W), _p(out), M, W.shape[1], W.shape[0], _stream()), 'plm_embed_fwd')
  return out


def embed_bwd(ids, dout, dW):
  """dW[ids[m]] += dout[m]  (dW must hold the value to accumulate onto)."""
  _need(ids, torch.int64, 'embed_bwd.ids')
  _need(dout, F32, 'embed_bwd.dout', 2)
  _need(dW, F32, 'embed_bwd.dW', 2)
  _lib.check(_lib.load().plm_embed_bwd(_p(ids), _p(dout), _p(dW), ids.numel(), dW.shape[1], dW.shape[0], _stream()),
             'plm_embed_bwd')
  return dW


def embed_bwd_sorted(ids, dout, dW, accumulate):
  """dW[v] (+)= sum of dout rows of the tokens with id v, in token order, without atomics (bit-reproducible); with
  accumulate=False every row of dW is written (zeros for unused ids).  Returns False when the shape is not supported
  (V >= 65536) - the caller then falls back to embed_bwd.  The launch sorts at most 65536 tokens (16-bit positions in its keys); longer
  batches go through it in slices of that many tokens, every slice after the first accumulating onto the previous ones - still in token
  order, still without atomics."""
  ids = ids.reshape(-1)
  _need(ids, torch.int64, 'embed_bwd_sorted.ids')
  _need(dout, F32, 'embed_bwd_sorted.dout', 2)
  _need(dW, F32, 'embed_bwd_sorted.dW', 2)
  lib = _lib.load()
  M, lim = ids.numel(), 65536
  if M > lim:
    if lib.plm_embed_bwd_workspace_bytes(lim, dW.shape[0]) == 0:
      return False
    for lo in range(0, M, lim):
      embed_bwd_sorted(ids[lo:lo + lim], dout[lo:lo + lim], dW, accumulate or lo > 0)
    return True
  nbytes = lib.plm_embed_bwd_workspace_bytes(ids.numel(), dW.shape[0])
  if nbytes == 0:
    return False
  stream = _stream()
  ws = _workspace(dout.device, nbytes, stream)
  with _Launch('hbm:embed_bwd', 4.0 * dout.numel() + (8.0 if accumulate else 4.0) * dW.numel() + 8.0 * ids.numel()):
    _lib.check(lib.plm_embed_bwd_sorted(_p(ids), _p(dout), _p(dW), ids.numel(), dW.shape[1], dW.shape[0], int(bool(accumulate)),
                                        _p(ws), nbytes, stream), 'plm_embed_bwd_sorted')
  return True


# ---- rmsnorm --------------------------------------------------------------------
def rmsnorm_fwd(x, w, eps, branch=None, write_xout=False):
  """returns (xout fp32 or None, y bf16, rstd fp32).  r = x + branch; y = bf16(r * rstd * w)."""
  _need(x, F32, 'rmsnorm_fwd.x', 2)
  _need(w, F32, 'rmsnorm_fwd.w', 1)
  M, d = x.shape
  if branch is not None:
    _need(branch, BF16, 'rmsnorm_fwd.branch', 2)
  xout = torch.empty_like(x) if (write_xout or branch is not None) else None
  y = torch.empty((M, d), dtype=BF16, device=x.device)
  rstd = torch.empty((M,), dtype=F32, device=x.device)
  with _Launch('hbm:rmsnorm_fwd', (6.0 + (2.0 if branch is not None else 0.0) + (4.0 if xout is not None else 0.0)) * M * d):
    _lib.check(_lib.load().plm_rmsnorm_fwd(_p(x), _p(branch), _p(xout), _p(w), _p(y), _p(rstd), M, d, float(eps), _stream()),
               'plm_rmsnorm_fwd')
  return xout, y, rstd


def rmsnorm_bwd(dy, x, w, rstd, gin=None, want_bf16=False, dw_out=None, dw_accumulate=False, defer_dw=False):
  """returns (dx fp32, dx_bf16 or None, dw fp32[d]).  dx = gin + d(rmsnorm).
  defer_dw: skip the column sum and return the [nblk, d] per-block partials in place of dw (the caller reduces a whole
  backward pass's norms with ONE colsum_multi launch)."""
  _need(dy, BF16, 'rmsnorm_bwd.dy', 2)
  _need(x, F32, 'rmsnorm_bwd.x', 2)
  M, d = x.shape
  lib = _lib.load()
  if gin is not None:
    _need(gin, F32, 'rmsnorm_bwd.gin', 2)
  dx = torch.empty_like(x)
  dxb = torch.empty((M, d), dtype=BF16, device=x.device) if want_bf16 else None
  nblk = lib.plm_rmsnorm_bwd_blocks(M)
  part = torch.empty((nblk, d), dtype=F32, device=x.device)
  with _Launch('hbm:rmsnorm_bwd', (10.0 + (4.0 if gin is not None else 0.0) + (2.0 if want_bf16 else 0.0)) * M * d):
    _lib.check(lib.plm_rmsnorm_bwd(_p(dy), _p(x), _p(w), _p(rstd), _p(gin), _p(dx), _p(dxb), _p(part), M, d, _stream()),
               'plm_rmsnorm_bwd')
  if defer_dw:
    return dx, dxb, part
  if dw_out is None:
    dw_out = torch.empty((d,), dtype=F32, device=x.device)
    dw_accumulate = False
  _lib.check(lib.plm_colsum_f32(_p(part), _p(dw_out), nblk, d, int(bool(dw_accumulate)), _stream()), 'plm_colsum_f32')
  return dx, dxb, dw_out


def colsum_multi(items):
  """[(part fp32 [rows, d], out fp32 [d], accumulate)] with one common rows x d: out (+)= column sums, ONE launch."""
  if not items:
    return
  rows, d = items[0][0].shape
  arr = (_lib.ColsumItem * len(items))()
  for i, (part, out, acc) in enumerate(items):
    _need(part, F32, 'colsum_multi.part', 2)
    _need(out, F32, 'colsum_multi.out')
    if tuple(part.shape) != (rows, d) or out.numel() != d:
      raise ValueError('colsum_multi: every item needs the same [rows, d] partials and a [d] output')
    arr[i] = _lib.ColsumItem(part.data_ptr(), out.data_ptr(), int(bool(acc)))
  _lib.check(_lib.load().plm_colsum_f32_multi(arr, len(items), rows, d, _stream()), 'plm_colsum_f32_multi')


# ---- swiglu -----------------------------------------------------------------------
def swiglu_fwd(u):
  _need(u, BF16, 'swiglu_fwd.u', 2)
  M, h2 = u.shape
  out = torch.empty((M, h2 // 2), dtype=BF16, device=u.device)
  _lib.check(_lib.load().plm_swiglu_fwd(_p(u), _p(out), M, h2 // 2, _stream()), 'plm_swiglu_fwd')
  return out


def swiglu_bwd(dout, u):
  _need(dout, BF16, 'swiglu_bwd.dout', 2)
  _need(u, BF16, 'swiglu_bwd.u', 2)
  du = torch.empty_like(u)
  _lib.check(_lib.load().plm_swiglu_bwd(_p(dout), _p(u), _p(du), u.shape[0], u.shape[1] // 2, _stream()), 'plm_swiglu_bwd')
  return du


ACT_KINDS = {'silu': 0, 'relu_sq': 1}


def act_fwd(u, kind):
  """bf16 act(u) for the plain MLP classes (components.py:31-40 silu, :59-70 relu squared)."""
  _need(u, BF16, 'act_fwd.u', 2)
  out = torch.empty_like(u)
  _lib.check(_lib.load().plm_act_fwd(_p(u), _p(out), u.numel(), ACT_KINDS[kind], _stream()), 'plm_act_fwd')
  return out


def act_bwd(dout, u, kind):
  _need(dout, BF16, 'act_bwd.dout', 2)
  _need(u, BF16, 'act_bwd.u', 2)
  du = torch.empty_like(u)
  _lib.check(_lib.load().plm_act_bwd(_p(dout), _p(u), _p(du), u.numel(), ACT_KINDS[kind], _stream()), 'plm_act_bwd')
  return du


# ---- GEMMs ------------------------------------------------------------------------
_C_DTYPE = {BF16: 0, F32: 1}  # c_dtype of plm_gemm_bf16_nt_ws


def gemm_nt(A, B, out=None, out_dtype=BF16, accumulate=False, alpha=None, variant=0):
  """C[M,N] = alpha * A[M,K] @ B[N,K]^T ; A, B bf16 (row stride may exceed K).
  variant: 0 auto | 1 128x128 register-staged | 2 128x128 LDS-DMA | 3 persistent 256x256, plain 4-phase ring |
  4 / 5 / 6 / 7 persistent 256x256 / 256x192 / 256x128 / 128x192, deep-prefetch ring with offset wave groups (what auto picks from)."""
  _need(A, BF16, 'gemm_nt.A', strided=True)
  _need(B, BF16, 'gemm_nt.B', strided=True)
  M, K = A.shape
  N = B.shape[0]
  if B.shape[1] != K:
    raise ValueError(f'gemm_nt: inner dims differ ({K} vs {B.shape[1]})')
  if out is None:
    out = torch.empty((M, N), dtype=out_dtype, device=A.device)
  if out.dim() != 2 or out.shape != (M, N) or out.stride(1) != 1:
    raise ValueError('gemm_nt.out: bad shape/stride')
  cd = _C_DTYPE[out.dtype]
  if alpha is not None:
    _need(alpha, F32, 'gemm_nt.alpha')
  launch = _Launch('gemm_nt', 2.0 * M * N * K)
  nbytes = _ws_bytes('plm_gemm_nt_workspace_bytes', M, N, K) if (variant == 0 and cd == 0) else 0
  stream = _stream()
  ws = _workspace(A.device, nbytes, stream) if nbytes else None
  with launch:
    _lib.check(_lib.load().plm_gemm_bf16_nt_ws(_p(A), A.stride(0), _p(B), B.stride(0), _p(out), out.stride(0), M, N, K, cd,
                                               int(bool(accumulate)), _p(alpha), int(variant), _p(ws), nbytes, stream), 'plm_gemm_bf16_nt')
  return out


def gemm_tn(A, B, out=None, accumulate=False, alpha=None):
  """C[M,N] (+)= alpha * A[K,M]^T @ B[K,N] ; A, B bf16, C fp32."""
  _need(A, BF16, 'gemm_tn.A', strided=True)
  _need(B, BF16, 'gemm_tn.B', strided=True)
  K, M = A.shape
  N = B.shape[1]
  if B.shape[0] != K:
    raise ValueError(f'gemm_tn: contraction dims differ ({K} vs {B.shape[0]})')
  if out is None:
    out = torch.empty((M, N), dtype=F32, device=A.device)
    accumulate = False
  if out.dtype != F32 or out.shape != (M, N) or out.stride(1) != 1:
    raise ValueError('gemm_tn.out: need fp32 [M, N] with unit inner stride')
  if alpha is not None:
    _need(alpha, F32, 'gemm_tn.alpha')
  lib = _lib.load()
  launch = _Launch('gemm_tn', 2.0 * M * N * K)
  nbytes = lib.plm_gemm_tn_workspace_bytes(M, N, K)
  stream = _stream()
  ws = _workspace(A.device, nbytes, stream) if nbytes else None
  with launch:
    _lib.check(lib.plm_gemm_bf16_tn(_p(A), A.stride(0), _p(B), B.stride(0), _p(out), out.stride(0), M, N, K,
                                    int(bool(accumulate)), _p(alpha), _p(ws), nbytes, stream), 'plm_gemm_bf16_tn')
  return out


TN_GROUP_MAX = 48  # PLM_TN_GROUP_MAX of csrc/gemm_plan.h


def gemm_tn_grouped(problems):
  """Several dW-style GEMMs with the same contraction length as ONE launch over the union of their output tiles (whole-K tiles for
  the full rounds of the persistent grid, split-K + one reduce for the remainder):
  problems = [(A[K,M] bf16, B[K,N] bf16, out[M,N] fp32, accumulate, alpha or None), ...] (at most TN_GROUP_MAX = 48);
  out (+)= alpha * A^T @ B for each.  Returns False when the shapes cannot be grouped (the caller then uses gemm_tn)."""
  n = len(problems)
  if n < 1 or n > TN_GROUP_MAX:
    return False
  K = problems[0][0].shape[0]
  arr = (_lib.TnProblem * n)()
  Ms, Ns = (C.c_int64 * n)(), (C.c_int64 * n)()
  for i, (A, B, out, accumulate, alpha) in enumerate(problems):
    _need(A, BF16, 'gemm_tn_grouped.A', strided=True)
    _need(B, BF16, 'gemm_tn_grouped.B', strided=True)
    if A.shape[0] != K or B.shape[0] != K:
      return False
    M, N = A.shape[1], B.shape[1]
    if out.dtype != F32 or out.shape != (M, N) or out.stride(1) != 1:
      raise ValueError('gemm_tn_grouped.out: need fp32 [M, N] with unit inner stride')
    if alpha is not None:
      _need(alpha, F32, 'gemm_tn_grouped.alpha')
    Ms[i], Ns[i] = M, N
    arr[i] = _lib.TnProblem(_p(A), A.stride(0), _p(B), B.stride(0), _p(out), out.stride(0), M, N, int(bool(accumulate)), _p(alpha))
  lib = _lib.load()
  if lib.plm_gemm_tn_grouped_workspace_bytes(Ms, Ns, n, K) == 0:  # unsupported shapes (independent of the CU reserve): the caller's
    return False                                                  # per-problem gemm_tn calls report to the launch hook themselves
  flops = sum(2.0 * a.shape[1] * b.shape[1] * K for a, b, *_ in problems)
  launch = _Launch('gemm_tn', flops)  # the hook may change the CU reserve: the plan is taken after it
  nbytes = lib.plm_gemm_tn_grouped_workspace_bytes(Ms, Ns, n, K)
  stream = _stream()
  ws = _workspace(problems[0][0].device, nbytes, stream)
  with launch:
    _lib.check(lib.plm_gemm_bf16_tn_grouped(arr, n, K, _p(ws), nbytes, stream), 'plm_gemm_bf16_tn_grouped')
  return True


def fc1_swiglu(x, w_fc1):
  """fc1 of the SwiGLU MLP with the activation in the GEMM epilogue: returns (u [M, 2h] = x @ w_fc1^T as gate | up, act [M, h])."""
  _need(x, BF16, 'fc1_swiglu.x', 2)
  _need(w_fc1, BF16, 'fc1_swiglu.w', 2)
  M, K = x.shape
  N = w_fc1.shape[0]
  if w_fc1.shape[1] != K or N % 16 != 0 or x.stride(1) != 1 or w_fc1.stride(1) != 1:
    raise ValueError('fc1_swiglu: need x [M, K], w [2h, K] with unit inner strides and h % 8 == 0')
  h = N // 2
  u = torch.empty((M, N), dtype=BF16, device=x.device)
  act = torch.empty((M, h), dtype=BF16, device=x.device)
  with _Launch('gemm_nt_fused', 2.0 * M * N * K):
    _lib.check(_lib.load().plm_fc1_swiglu_bf16(_p(x), x.stride(0), _p(w_fc1), w_fc1.stride(0), _p(u), _p(act), M, h, K, _stream()),
               'plm_fc1_swiglu_bf16')
  return u, act


def fc2_dx_swiglu_bwd(dy, w2t, u):
  """du [M, 2h] = swiglu_bwd(dy @ w2t^T, u): the dX GEMM of fc2 (w2t = bf16 W_fc2^T [h, K(+pad)]) with the SwiGLU backward in its
  epilogue; d(act) is never stored for qualifying shapes."""
  _need(dy, BF16, 'fc2_dx_swiglu_bwd.dy', 2)
  _need(w2t, BF16, 'fc2_dx_swiglu_bwd.w2t', 2)
  _need(u, BF16, 'fc2_dx_swiglu_bwd.u', 2)
  M, K = dy.shape
  h = w2t.shape[0]
  if w2t.shape[1] != K or u.shape != (M, 2 * h) or not u.is_contiguous() or dy.stride(1) != 1 or w2t.stride(1) != 1:
    raise ValueError('fc2_dx_swiglu_bwd: need dy [M, K], w2t [h, K], contiguous u [M, 2h]')
  du = torch.empty((M, 2 * h), dtype=BF16, device=dy.device)
  lib = _lib.load()
  with _Launch('gemm_nt_fused', 2.0 * M * h * K):
    # first without the d(act) scratch: the one-launch path never touches it; the library answers PLM_E_WORKSPACE (-4) when this
    # shape takes the two-launch path, and only then is the buffer allocated
    rc = lib.plm_fc2_dx_swiglu_bwd_bf16(_p(dy), dy.stride(0), _p(w2t), w2t.stride(0), _p(u), _p(du), _p(None), M, h, K, _stream())
    if rc == -4:
      scratch = torch.empty((M, h), dtype=BF16, device=dy.device)
      rc = lib.plm_fc2_dx_swiglu_bwd_bf16(_p(dy), dy.stride(0), _p(w2t), w2t.stride(0), _p(u), _p(du), _p(scratch), M, h, K, _stream())
    _lib.check(rc, 'plm_fc2_dx_swiglu_bwd_bf16')
  return du


# ---- attention ----------------------------------------------------------------------
def rope_qk_(qkv, rope_cos, rope_sin, B, T, nh):
  """Rotate the q and k column blocks of a projection output in place (qkv_rope's fallback; the step uses the fused epilogue)."""
  _need(qkv, BF16, 'rope_qk.qkv', 2)
  hd = qkv.shape[1] // (3 * nh)
  _need(rope_cos, F32, 'rope_qk.rope_cos', 2)
  _need(rope_sin, F32, 'rope_qk.rope_sin', 2)
  if rope_cos.shape[0] < T or rope_cos.shape[1] != hd // 2:
    raise ValueError('rope_qk: RoPE table too short for T or wrong head_dim')
  _lib.check(_lib.load().plm_rope_qk(_p(qkv), _p(rope_cos), _p(rope_sin), B, T, nh, hd, _stream()), 'plm_rope_qk')
  return qkv


def qkv_rope(x, w_qkv, rope_cos, rope_sin, B, T, nh):
  """qkv[M, 3d] = x @ w_qkv^T with q | k rotated: one launch, the rotation in the GEMM's store-side epilogue (shapes that do
  not qualify: GEMM + the in-place rope_qk_ pass, same bits)."""
  _need(x, BF16, 'qkv_rope.x', 2)
  _need(w_qkv, BF16, 'qkv_rope.w', 2)
  M, K = x.shape
  N = w_qkv.shape[0]
  hd = N // (3 * nh)
  out = torch.empty((M, N), dtype=BF16, device=x.device)
  with _Launch('gemm_nt_fused', 2.0 * M * N * K):
    _lib.check(_lib.load().plm_qkv_rope_bf16(_p(x), x.stride(0), _p(w_qkv), w_qkv.stride(0), _p(out), N, M, K, _p(rope_cos),
                                             _p(rope_sin), B, T, nh, hd, _stream()), 'plm_qkv_rope_bf16')
  return out


def doc_start_from_mask(mask):
  """bool [B, T, T] (True = may attend: the reference's mask, engine/engine.py:21-23) -> (doc_start int32 [B, T], status int32 [1]): status
  becomes 1 when some row is not exactly True on [doc_start, i] - the caller decides when to look (it is a device tensor)."""
  if mask.dtype != torch.bool or mask.dim() != 3 or mask.shape[1] != mask.shape[2] or not mask.is_cuda:
    raise ValueError('doc_start_from_mask: need a bool [B, T, T] tensor on the GPU')
  mask = mask.contiguous()
  B, T = mask.shape[0], mask.shape[1]
  ds = torch.empty((B, T), dtype=torch.int32, device=mask.device)
  status = torch.zeros((1,), dtype=torch.int32, device=mask.device)
  _lib.check(_lib.load().plm_attn_doc_start_from_mask(_p(mask), _p(ds), _p(status), B, T, _stream()), 'plm_attn_doc_start_from_mask')
  return ds, status


def attn_doc_plan(doc_start, nh):
  """Plan of a document-masked batch for attention with nh heads (include/plainlm_hip.h: doc_end[B,T] + the sorted item lists): built ONCE
  per batch, shared by every layer's forward / backward launches."""
  _need(doc_start, torch.int32, 'attn_doc_plan.doc_start', 2)
  B, T = doc_start.shape
  lib = _lib.load()
  plan = torch.empty((lib.plm_attn_doc_plan_bytes(B, T) // 4,), dtype=torch.int32, device=doc_start.device)
  _lib.check(lib.plm_attn_doc_plan(_p(doc_start), _p(plan), B, T, nh, _stream()), 'plm_attn_doc_plan')
  return plan


def attn_flops(B, T, nh, hd, doc_start=None):
  """Algorithmic flops of the forward pass: 2 matmuls x 2 flop x hd per visible (query, key) pair - causal T(T+1)/2 pairs per head and
  sequence, with a document mask the pairs doc_start[i] <= j <= i (one small device reduction, cached on the tensor)."""
  if doc_start is None:
    return 4.0 * B * nh * hd * T * (T + 1) / 2
  pairs = getattr(doc_start, '_plm_pairs', None)
  if pairs is None:
    pos = torch.arange(T, device=doc_start.device, dtype=torch.int64)[None, :]
    pairs = float((pos - doc_start.to(torch.int64) + 1).sum().item())
    try:
      doc_start._plm_pairs = pairs
    except AttributeError:
      pass
  return 4.0 * nh * hd * pairs


def _attn_outputs(qkv, B, T, nh, fwd):
  """(hd, out bf16 [B*T, nh*hd], lse fp32 [B, nh, T]) of a forward pass over this projection output, (hd, dqkv, delta) of a backward."""
  hd = qkv.shape[1] // (3 * nh)
  big = torch.empty((B * T, nh * hd), dtype=BF16, device=qkv.device) if fwd else torch.empty_like(qkv)
  return hd, big, torch.empty((B, nh, T), dtype=F32, device=qkv.device)


def _attn_launch(family, passes, B, T, nh, hd, doc_start):
  """The bracket of a causal / document-masked launch: the hook's clock only needs an estimate, so it gets the causal figure; the visible
  pairs under doc_start cost a device reduction, which is paid only when PROFILE is on - never on the launch path."""
  launch = _Launch(family, passes * attn_flops(B, T, nh, hd))
  if PROFILE is not None:
    launch.work = passes * attn_flops(B, T, nh, hd, doc_start)
  return launch


def attn_fwd(qkv_rot, B, T, nh, doc_start=None, plan=None):
  """qkv_rot: projection output with q, k already rotated (rope_qk_).  doc_start: int32 [B,T] document mask; plan: attn_doc_plan(doc_start)
  (built here when absent - pass it when the same batch goes through several layers)."""
  _need(qkv_rot, BF16, 'attn_fwd.qkv', 2)
  if doc_start is not None:
    _need(doc_start, torch.int32, 'attn_fwd.doc_start', 2)
    if plan is None:
      plan = attn_doc_plan(doc_start, nh)
  hd, out, lse = _attn_outputs(qkv_rot, B, T, nh, True)
  with _attn_launch('attn_fwd', 1.0, B, T, nh, hd, doc_start):
    _lib.check(_lib.load().plm_attn_fwd(_p(qkv_rot), _p(doc_start), _p(plan), _p(out), _p(lse), B, T, nh, hd, _stream()), 'plm_attn_fwd')
  return out, lse


def attn_bwd(qkv, out, dout, lse, rope_cos, rope_sin, B, T, nh, doc_start=None, plan=None, return_delta=False):
  """dqkv w.r.t. the UN-rotated projection.  return_delta: also return the kernels' delta = rowsum(dO * O), fp32 [B, nh, T] (the hd = 64
  families store it negated for their dK/dV kernel; it is returned here with the plain sign)."""
  _need(dout, BF16, 'attn_bwd.dout', 2)
  if doc_start is not None and plan is None:
    plan = attn_doc_plan(doc_start, nh)
  hd, dqkv, delta = _attn_outputs(qkv, B, T, nh, False)
  with _attn_launch('attn_bwd', 2.0, B, T, nh, hd, doc_start):
    _lib.check(_lib.load().plm_attn_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(rope_cos), _p(rope_sin), _p(doc_start), _p(plan),
                                        _p(dqkv), _p(delta), B, T, nh, hd, _stream()), 'plm_attn_bwd')
  if return_delta:
    return dqkv, (-delta if hd == 64 else delta)
  return dqkv


def attn_mask_pack(mask):
  """Dense mask mode: bool [B, T, T] (True = may attend, the reference's layout) or [T, T] (one mask for every sequence) on the GPU ->
  (bits int64 [M, T, ceil(T/64)] - the kernels' uint64 words: bit j % 64 of word (m, i, j // 64) is mask[m, i, j] -, tile_class uint8
  [M, ceil(T/128), ceil(T/64)]: 0 = no bit set, 1 = every in-range bit set, 2 = mixed), M = B, or 1 for a [T, T] / [1, T, T] mask.  One launch,
  both results views of one allocation; pack once per batch and pass the pair to every layer's attn_fwd_masked / attn_bwd_masked."""
  if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
    raise TypeError('attn_mask_pack: need a bool mask')
  if mask.dim() not in (2, 3) or mask.shape[-1] != mask.shape[-2] or mask.shape[-1] == 0:
    raise ValueError(f'attn_mask_pack: need a bool [B, T, T] or [T, T] mask, got shape {tuple(mask.shape)}')
  if not mask.is_cuda:
    raise RuntimeError('attn_mask_pack: mask must live on the GPU (plainlm_amd has no CPU path)')
  mask = mask.contiguous()
  T = mask.shape[-1]
  M = mask.shape[0] if mask.dim() == 3 else 1
  if T % 4:
    raise ValueError(f'attn_mask_pack: T={T} must be a multiple of 4')
  W, NQT = (T + 63) // 64, (T + 127) // 128
  lib = _lib.load()
  buf = torch.empty((lib.plm_attn_mask_bytes(M, T),), dtype=torch.uint8, device=mask.device)
  nb = M * T * W * 8
  bits = buf[:nb].view(torch.int64).view(M, T, W)
  tile_class = buf[nb:nb + M * NQT * W].view(M, NQT, W)
  _lib.check(lib.plm_attn_mask_pack(_p(mask), 1 if M > 1 else 0, _p(bits), _p(tile_class), M, T, _stream()), 'plm_attn_mask_pack')
  return bits, tile_class


def _mask_stride(bits, tile_class, B, T, what):
  W = (T + 63) // 64
  if bits.dtype != torch.int64 or tile_class.dtype != torch.uint8 or not bits.is_cuda or not tile_class.is_cuda:
    raise TypeError(f'{what}: bits / tile_class must be the int64 / uint8 GPU tensors of attn_mask_pack')
  if bits.dim() != 3 or bits.shape[0] not in (1, B) or tuple(bits.shape[1:]) != (T, W) or \
     tuple(tile_class.shape) != (bits.shape[0], (T + 127) // 128, W):
    raise ValueError(f'{what}: packed mask of shape {tuple(bits.shape)} / {tuple(tile_class.shape)} does not fit B={B}, T={T}')
  return 1 if bits.shape[0] == B and B > 1 else 0


def attn_fwd_masked(qkv_rot, bits, tile_class, B, T, nh):
  """attn_fwd under a packed dense mask (attn_mask_pack).  A query row with no allowed key gives out = 0 and lse = +inf (torch's SDPA
  returns 0 for such a row)."""
  _need(qkv_rot, BF16, 'attn_fwd_masked.qkv', 2)
  bs = _mask_stride(bits, tile_class, B, T, 'attn_fwd_masked')
  hd, out, lse = _attn_outputs(qkv_rot, B, T, nh, True)
  _Launch('attn_fwd', attn_flops(B, T, nh, hd))  # reported to the hook, not timed
  _lib.check(_lib.load().plm_attn_fwd_masked(_p(qkv_rot), _p(bits), _p(tile_class), bs, _p(out), _p(lse), B, T, nh, hd, _stream()),
             'plm_attn_fwd_masked')
  return out, lse


def attn_bwd_masked(qkv, out, dout, lse, rope_cos, rope_sin, bits, tile_class, B, T, nh, return_delta=False):
  """attn_bwd under a packed dense mask: dqkv w.r.t. the UN-rotated projection; return_delta: also delta = rowsum(dO * O), fp32 [B, nh, T]."""
  _need(dout, BF16, 'attn_bwd_masked.dout', 2)
  bs = _mask_stride(bits, tile_class, B, T, 'attn_bwd_masked')
  hd, dqkv, delta = _attn_outputs(qkv, B, T, nh, False)
  _Launch('attn_bwd', 2.0 * attn_flops(B, T, nh, hd))  # reported to the hook, not timed
  _lib.check(_lib.load().plm_attn_bwd_masked(_p(qkv), _p(out), _p(dout), _p(lse), _p(rope_cos), _p(rope_sin), _p(bits), _p(tile_class), bs,
                                             _p(dqkv), _p(delta), B, T, nh, hd, _stream()), 'plm_attn_bwd_masked')
  if return_delta:
    return dqkv, delta
  return dqkv


# ---- the cached step (DESIGN.md sections 12 and 14): one token per sequence on top of a KV cache, or a chunk of them -------------
def _need_kv(kv, nh, hd, name):
  """kv bf16 [B, Tmax, >= 2*nh*hd]: rows may be padded (stride(1) a multiple of 8), sequences are Tmax rows apart."""
  if not kv.is_cuda:
    raise RuntimeError(f'{name}: tensor must live on the GPU (plainlm_amd has no CPU path)')
  if kv.dtype != BF16 or kv.dim() != 3 or kv.shape[2] != 2 * nh * hd or kv.stride(2) != 1 or kv.stride(0) != kv.shape[1] * kv.stride(1):
    raise ValueError(f'{name}: need a bf16 [B, Tmax, 2*nh*hd] cache with unit inner stride and batch stride Tmax * row stride')
  return kv


def _cached_operands(name, rows, width, kv, nh, lens, lens_name, chunk, n_new=None, rope=None, need_kv=None):
  """The operand checks of the four cached-step ops, returns (B, n, hd).  rows: bf16 [B*n, width*nh*hd] - width 3 the UN-rotated qkv
  (row stride free), width 1 the rotated q; kv: the cache; lens int32 [B]; n_new None | int32 [B]; rope None | (cos, sin) fp32
  [rows, hd/2].  chunk False: one row per sequence (n = 1), the batch is the rows'; True: n = rows / the cache's batch.  need_kv: another
  cache format's stand-in for _need_kv (ops_kv8.py)."""
  try:  # the per-tensor checks name the tensor; the op's name is put in front only when one fails (no string is built per call)
    if width == 3:
      if _need(rows, BF16, 'qkv', strided=True).shape[1] % (3 * nh) != 0:
        raise ValueError(f'qkv: need {"B*n" if chunk else "B"} rows of 3*nh*hd columns, got {rows.shape[1]} for nh={nh}')
    else:
      _need(rows, BF16, 'q', 2)
    hd = rows.shape[1] // (width * nh)
    (need_kv or _need_kv)(kv, nh, hd, 'kv')
    _need(lens, torch.int32, lens_name, 1)
    if rope is not None:
      _need(rope[0], F32, 'rope_cos', 2)
      _need(rope[1], F32, 'rope_sin', 2)
    if n_new is not None:
      _need(n_new, torch.int32, 'n_new', 1)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  B = kv.shape[0] if chunk else rows.shape[0]
  fits = rows.shape[1] == width * nh * hd and kv.shape[0] == B and lens.shape[0] == B
  if chunk:
    fits = fits and B >= 1 and rows.shape[0] >= B and rows.shape[0] % B == 0
  if rope is not None:
    fits = fits and rope[0].shape == rope[1].shape and rope[0].shape[1] == hd // 2
  if not fits:
    raise ValueError(f'{name}: {"qkv" if width == 3 else "q"} {tuple(rows.shape)}, kv {tuple(kv.shape)}, {lens_name} {tuple(lens.shape)} do not '
                     f'fit nh={nh}' + ('' if rope is None else f', or the RoPE tables {tuple(rope[0].shape)} / {tuple(rope[1].shape)} the head_dim'))
  if n_new is not None and n_new.shape[0] != B:
    raise ValueError(f'{name}: n_new {tuple(n_new.shape)} does not fit the batch of {B}')
  return B, rows.shape[0] // B if chunk else 1, hd


def _append_outputs(name, qkv, rows, dm, q_out, status):
  """(q_out bf16 [rows, dm], status int32 [1]) of an append: the caller's, checked, or made here (status zeroed)."""
  try:
    if q_out is not None and tuple(_need(q_out, BF16, 'q_out', 2).shape) != (rows, dm):
      raise ValueError(f'q_out: need [{rows}, {dm}], got {tuple(q_out.shape)}')
    if status is not None:
      _need(status, torch.int32, 'status')
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  return (torch.empty((rows, dm), dtype=BF16, device=qkv.device) if q_out is None else q_out,
          torch.zeros((1,), dtype=torch.int32, device=qkv.device) if status is None else status)


def _cached_ws_bytes(kernel, B, n, nh, hd, Tmax, splits):
  """Workspace bytes of attn_decode / attn_extend for this shape and splits argument; a shape the library refuses raises."""
  nbytes = _ws_bytes('plm_attn_decode_workspace_bytes', B, nh, hd, Tmax, int(splits)) if kernel == 'attn_decode' else \
      _ws_bytes('plm_attn_extend_workspace_bytes', B, n, nh, hd, Tmax, int(splits))
  if nbytes == 0:
    raise ValueError(f'{kernel}: unsupported shape B={B} n={n} nh={nh} hd={hd} Tmax={Tmax} or splits={splits} (0 = automatic, 1..64)')
  return nbytes


def _cached_workspace(kernel, B, n, nh, hd, Tmax, splits, device, workspace):
  """(workspace, bytes, stream) of one attn_decode / attn_extend launch: the caller's pair, else the arena of the launch's stream at the
  size the library asks for."""
  stream = _stream()
  if workspace is not None:
    return workspace[0], workspace[1], stream
  nbytes = _cached_ws_bytes(kernel, B, n, nh, hd, Tmax, splits)
  return _workspace(device, nbytes, stream), nbytes, stream


def kv_append_rope(qkv, pos, rope_cos, rope_sin, kv, nh, q_out=None, status=None):
  """One decode token per sequence: qkv bf16 [B, 3*nh*hd] UN-rotated (row stride may exceed it), pos int32 [B].  Rotates q and k at
  position pos[b] (rope_qk_'s bits), returns rotated q [B, nh*hd] and writes rotated k | untouched v into kv[b, pos[b]].  A pos[b] outside
  [0, min(Tmax, rope rows)) writes nothing for that sequence and sets status[0] = 1 (int32 [1], zeroed by the caller; made here when
  absent).  Returns (q_out, status): status is a device tensor, the caller decides when to look."""
  B, _, hd = _cached_operands('kv_append_rope', qkv, 3, kv, nh, pos, 'pos', False, rope=(rope_cos, rope_sin))
  q_out, status = _append_outputs('kv_append_rope', qkv, B, nh * hd, q_out, status)
  _lib.check(_lib.load().plm_kv_append_rope(_p(qkv), qkv.stride(0), _p(pos), _p(rope_cos), _p(rope_sin), rope_cos.shape[0], _p(q_out), _p(kv),
                                            kv.stride(1), _p(status), B, kv.shape[1], nh, hd, _stream()), 'plm_kv_append_rope')
  return q_out, status


def attn_decode_workspace(B, nh, hd, Tmax, splits, device):
  """A caller-owned (uint8 workspace, bytes) pair for attn_decode(..., workspace=) at this shape and splits argument."""
  return torch.empty(nbytes := _cached_ws_bytes('attn_decode', B, 1, nh, hd, Tmax, splits), dtype=torch.uint8, device=device), nbytes


def attn_decode(q, kv, lens, nh, splits=0, want_lse=False, workspace=None):
  """Attention of one rotated query row per sequence over its cache: q bf16 [B, nh*hd], kv bf16 [B, Tmax, 2*nh*hd] (kv_append_rope's
  layout), lens int32 [B] (clamped to [0, Tmax]; sequence b attends keys 0 .. lens[b]-1, lens[b] == 0 gives out = 0 and lse = +inf).
  splits: 0 automatic (from the shape alone) | 1..64 forced.  Returns out bf16 [B, nh*hd], or (out, lse fp32 [B, nh], base 2 like
  attn_fwd's) with want_lse.  workspace: the caller's (uint8 tensor, bytes) of attn_decode_workspace for the same splits, else the stream's arena."""
  B, _, hd = _cached_operands('attn_decode', q, 1, kv, nh, lens, 'lens', False)
  Tmax = kv.shape[1]
  ws, nbytes, stream = _cached_workspace('attn_decode', B, 1, nh, hd, Tmax, splits, q.device, workspace)
  out = torch.empty((B, nh * hd), dtype=BF16, device=q.device)
  lse = torch.empty((B, nh), dtype=F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_decode(_p(q), _p(kv), kv.stride(1), _p(lens), _p(out), _p(lse), B, Tmax, nh, hd, int(splits), _p(ws), nbytes,
                                         stream), 'plm_attn_decode')
  return (out, lse) if want_lse else out


def kv_append_rope_rows(qkv, lens0, rope_cos, rope_sin, kv, nh, n_new=None, q_out=None, status=None):
  """A chunk of n tokens per sequence: qkv bf16 [B*n, 3*nh*hd] UN-rotated (row b*n + r = chunk row r of sequence b; the row stride may
  exceed the width), lens0 int32 [B] the cache lengths before the chunk, n_new int32 [B] the real rows of every chunk (clamped to
  [0, n]; None: n everywhere).  Rows r < n_new[b] are rotated at position lens0[b] + r (rope_qk_'s bits): rotated q goes to q_out
  [B*n, nh*hd], rotated k | untouched v into kv[b, lens0[b] + r].  Rows past n_new[b] write no cache row and zeros to q_out.  A sequence
  with lens0[b] < 0 or lens0[b] + n_new[b] > min(Tmax, rope rows) stores nothing, gets zero q_out rows and sets status[0] = 1 (int32 [1],
  zeroed by the caller; made here when absent).  Returns (q_out, status): status is a device tensor, the caller decides when to look."""
  B, n, hd = _cached_operands('kv_append_rope_rows', qkv, 3, kv, nh, lens0, 'lens0', True, n_new=n_new, rope=(rope_cos, rope_sin))
  q_out, status = _append_outputs('kv_append_rope_rows', qkv, B * n, nh * hd, q_out, status)
  _lib.check(_lib.load().plm_kv_append_rope_rows(_p(qkv), qkv.stride(0), _p(lens0), _p(n_new), _p(rope_cos), _p(rope_sin), rope_cos.shape[0],
                                                 _p(q_out), _p(kv), kv.stride(1), _p(status), B, n, kv.shape[1], nh, hd, _stream()),
             'plm_kv_append_rope_rows')
  return q_out, status


def attn_extend_workspace(B, n, nh, hd, Tmax, splits, device):
  """A caller-owned (uint8 workspace, bytes) pair for attn_extend(..., workspace=) at this shape (chunk width n) and splits argument."""
  return torch.empty(nbytes := _cached_ws_bytes('attn_extend', B, n, nh, hd, Tmax, splits), dtype=torch.uint8, device=device), nbytes


def attn_extend(q, kv, lens0, nh, n_new=None, splits=0, want_lse=False, workspace=None):
  """Attention of a chunk of n rotated query rows per sequence over its cache: q bf16 [B*n, nh*hd] (kv_append_rope_rows's q_out), kv bf16
  [B, Tmax, 2*nh*hd] with the chunk already appended, lens0 int32 [B] the lengths BEFORE the chunk (clamped to [0, Tmax]), n_new int32 [B]
  the real rows of every chunk (None: n).  Row r < n_new[b] of sequence b attends keys 0 .. lens0[b] + r; rows past n_new[b] give out = 0
  and lse = +inf.  splits: 0 automatic (from the shape alone) | 1..64 forced.  Returns out bf16 [B*n, nh*hd], or (out, lse fp32
  [B, nh, n], base 2 like attn_fwd's) with want_lse.  workspace: the caller's (uint8 tensor, bytes) of attn_extend_workspace for the same splits, else
  the stream's arena."""
  B, n, hd = _cached_operands('attn_extend', q, 1, kv, nh, lens0, 'lens0', True, n_new=n_new)
  Tmax = kv.shape[1]
  ws, nbytes, stream = _cached_workspace('attn_extend', B, n, nh, hd, Tmax, splits, q.device, workspace)
  out = torch.empty((B * n, nh * hd), dtype=BF16, device=q.device)
  lse = torch.empty((B, nh, n), dtype=F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_extend(_p(q), _p(kv), kv.stride(1), _p(lens0), _p(n_new), _p(out), _p(lse), B, n, Tmax, nh, hd, int(splits),
                                         _p(ws), nbytes, stream), 'plm_attn_extend')
  return (out, lse) if want_lse else out


SampleLogits = collections.namedtuple('SampleLogits', ['tokens', 'logprob', 'n_kept', 'cutoff'])


def sample_logits(logits, u, temperature=1.0, top_k=0, top_p=1.0, want_stats=False):
  """One token per row of logits bf16 [B, V] (unit inner stride, any row stride >= V and any 2-byte aligned base: a column slice of a
  wider buffer is fine) by temperature, then top-k, then top-p, then the draw with u fp32 [B] (top-k keeps every
  tie with the k-th value, top-p keeps or drops equal logits together; top_k = 0 and top_p = 1 are off).  One launch, bit-reproducible.
  Returns the named tuple (tokens int64 [B], logprob fp32 [B] = log softmax(logits)[tokens] at temperature 1, n_kept int32 [B],
  cutoff fp32 [B]): the size of the kept set and its lowest logit with want_stats, else None."""
  _need(logits, BF16, 'sample_logits.logits', strided=True)
  if logits.shape[0] < 1 or logits.shape[1] < 1 or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
    raise ValueError('sample_logits.logits: need a 2-D bf16 GPU tensor [B, V] with unit inner stride and row stride >= V')
  B, V = logits.shape
  _need(u, F32, 'sample_logits.u', 1)
  if u.shape[0] != B:
    raise ValueError(f'sample_logits: u {tuple(u.shape)} does not fit logits {tuple(logits.shape)}')
  new = lambda want, dtype: torch.empty((B,), dtype=dtype, device=logits.device) if want else None  # noqa: E731
  tok, logp = new(True, torch.int64), new(True, F32)
  n_kept, cutoff = new(want_stats, torch.int32), new(want_stats, F32)
  _lib.check(_lib.load().plm_sample_logits_bf16(_p(logits), logits.stride(0) if B > 1 else V, _p(u), float(temperature), int(top_k),
                                                float(top_p), _p(tok), _p(logp), _p(n_kept), _p(cutoff), B, V, _stream()),
             'plm_sample_logits_bf16')
  return SampleLogits(tok, logp, n_kept, cutoff)


SpecVerify = collections.namedtuple('SpecVerify', ['n_accept', 'next_token', 'logprob'])


def _logits_rows(t, rows, name):
  _need(t, BF16, name, strided=True)
  if t.shape[0] != rows or t.shape[1] < 1 or (rows > 1 and t.stride(0) < t.shape[1]):
    raise ValueError(f'{name}: need a 2-D bf16 GPU tensor [{rows}, V] with unit inner stride and row stride >= V, got {t.dtype} '
                     f'{tuple(t.shape)}')
  return t.stride(0) if rows > 1 else t.shape[1]


def spec_verify(target_logits, draft_logits, draft_tokens, target_cutoff, draft_cutoff, target_tokens, u_accept, u_resid, temperature=1.0):
  """The speculative-sampling acceptance rule on k drafted tokens per sequence (include/plainlm_hip.h states the
  rule).  target_logits bf16 [B*(k+1), V], row b*(k+1) + r (extend(all_rows=True, logits=True), flattened); draft_logits bf16 [k*B, V],
  step-major (row r*B + b); both with unit inner stride and any row stride >= V.  draft_tokens int64 [k, B]; target_cutoff fp32
  [B*(k+1)] / draft_cutoff fp32 [k*B] and target_tokens int64 [B*(k+1)]: the ``cutoff`` and ``tokens`` of ops.sample_logits(...,
  want_stats=True) on those rows at this temperature; u_accept fp32 [k, B], u_resid fp32 [B].  Two launches, bit-reproducible, nothing is
  read back.  Returns the named tuple (n_accept int32 [B], next_token int64 [B], logprob fp32 [B, k+1]: the target's log-probability at
  temperature 1 of every emitted token, 0 beyond entry n_accept)."""
  _need(draft_tokens, torch.int64, 'spec_verify.draft_tokens', 2)
  k, B = draft_tokens.shape
  ldp = _logits_rows(target_logits, B * (k + 1), 'spec_verify.target_logits')
  ldq = _logits_rows(draft_logits, k * B, 'spec_verify.draft_logits')
  V = target_logits.shape[1]
  if draft_logits.shape[1] != V:
    raise ValueError(f'spec_verify: draft_logits have {draft_logits.shape[1]} columns, target_logits {V}')
  for t, dtype, n, name in ((target_cutoff, F32, B * (k + 1), 'target_cutoff'), (draft_cutoff, F32, k * B, 'draft_cutoff'),
                            (target_tokens, torch.int64, B * (k + 1), 'target_tokens'), (u_accept, F32, k * B, 'u_accept'),
                            (u_resid, F32, B, 'u_resid')):
    _need(t, dtype, f'spec_verify.{name}')
    if t.numel() != n:
      raise ValueError(f'spec_verify: {name} {tuple(t.shape)} does not hold {n} elements (B={B}, k={k})')
  dev = target_logits.device
  n_accept = torch.empty((B,), dtype=torch.int32, device=dev)
  next_tok = torch.empty((B,), dtype=torch.int64, device=dev)
  logp = torch.empty((B, k + 1), dtype=F32, device=dev)
  _lib.check(_lib.load().plm_spec_verify_bf16(_p(target_logits), ldp, _p(draft_logits), ldq, _p(draft_tokens), _p(target_cutoff),
                                              _p(draft_cutoff), _p(target_tokens), _p(u_accept), _p(u_resid), float(temperature),
                                              _p(n_accept), _p(next_tok), _p(logp), B, k, V, _stream()), 'plm_spec_verify_bf16')
  return SpecVerify(n_accept, next_tok, logp)


# ---- cross entropy --------------------------------------------------------------------
def ce_fwd_bwd_(logits, targets, grad_scale, V=None):
  """In place: logits[:, :V] <- (softmax - onehot) * grad_scale, logits[:, V:] <- 0 (logits is bf16 [M, ld], ld >= V).
  Returns per-row losses fp32[M]."""
  _need(logits, BF16, 'ce.logits', 2)
  _need(targets, torch.int64, 'ce.targets', 1)
  M, ld = logits.shape
  V = ld if V is None else V
  rows = torch.empty((M,), dtype=F32, device=logits.device)
  with _Launch('hbm:ce_fwd_bwd', 4.0 * M * V):  # one read + one write of the bf16 logits
    _lib.check(_lib.load().plm_ce_fwd_bwd(_p(logits), _p(targets), _p(rows), M, V, ld, float(grad_scale), _stream()),
               'plm_ce_fwd_bwd')
  return rows


HeadPredict = collections.namedtuple('HeadPredict', ['pred', 'logp', 'entropy', 'nll', 'lse'])
_HEAD_ABI = {'head_score': ('plm_head_score_bf16', 'plm_head_score_workspace_bytes'),
             'head_predict': ('plm_head_predict_bf16', 'plm_head_predict_workspace_bytes')}


def _head(name, y, w, targets, wants):
  """What head_score and head_predict share: the operand checks, the launch bracket, the workspace (the library is handed at least 16
  bytes) and the call plm_<name>_bf16(y, ld, w, ld, targets, outputs ..., M, V, K, workspace, bytes, stream).  wants: one
  (wanted, dtype) per output of the entry point; returns the [M] outputs, None for those not wanted."""
  try:  # the op's name is put in front only when a check fails (no string is built per call)
    _need(y, BF16, 'y', strided=True)
    _need(w, BF16, 'w', strided=True)
    if targets is not None:
      _need(targets, torch.int64, 'targets', 1)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  M, K = y.shape
  V = w.shape[0]
  if w.shape[1] != K or (targets is not None and targets.shape[0] != M):
    raise ValueError(f'{name}: y {tuple(y.shape)}, w {tuple(w.shape)}, targets {None if targets is None else tuple(targets.shape)} do not fit')
  entry, query = _HEAD_ABI[name]
  launch = _Launch('gemm_nt', 2.0 * M * V * K)
  nbytes = _ws_bytes(query, M, V, K)
  stream = _stream()
  ws = _workspace(y.device, max(nbytes, 16), stream)
  outs = [torch.empty((M,), dtype=dtype, device=y.device) if want else None for want, dtype in wants]
  with launch:
    _lib.check(getattr(_lib.load(), entry)(_p(y), y.stride(0), _p(w), w.stride(0), _p(targets), *[_p(o) for o in outs], M, V, K, _p(ws),
                                           nbytes, stream), entry)
  return outs


def head_score(y, w, targets, want_lse=False):
  """Forward-only scoring head: nll fp32[M] = logsumexp(l) - l[target] of the rows l = bf16(y[M,K] @ w[V,K]^T) - the training head's
  logits, bit for bit - without the [M, V] buffer (the NT GEMM reduces every tile to per-row (max, sum-exp) pairs).
  A target outside [0, V) is ignored (nll = 0).  want_lse: also return lse fp32[M].  No gradient."""
  _need(targets, torch.int64, 'head_score.targets', 1)
  nll, lse = _head('head_score', y, w, targets, ((True, F32), (want_lse, F32)))
  return (nll, lse) if want_lse else nll


def head_predict(y, w, targets=None, want_entropy=True, want_lse=False):
  """Prediction head: per row of l = bf16(y[M,K] @ w[V,K]^T) - the training head's logits, bit for bit, never stored -
  pred int64[M] (first index of the maximum, always in [0, V)), logp fp32[M] = log softmax(l)[pred], entropy fp32[M] in nats, and with
  ``targets`` nll fp32[M] as head_score gives it (0 where the target is outside [0, V)); want_lse: lse fp32[M].  Returns the named tuple
  (pred, logp, entropy, nll, lse) with None for the parts not asked for.  No gradient."""
  return HeadPredict(*_head('head_predict', y, w, targets,
                            ((True, torch.int64), (True, F32), (want_entropy, F32), (targets is not None, F32), (want_lse, F32))))


def mean(x):
  _need(x, F32, 'mean.x')
  out = torch.empty((), dtype=F32, device=x.device)
  _lib.check(_lib.load().plm_mean_f32(_p(x), _p(out), x.numel(), _stream()), 'plm_mean_f32')
  return out


def scale_bf16_(x, alpha):
  """x <- bf16(x * alpha) in place; alpha is a 0-d fp32 device tensor."""
  _need(x, BF16, 'scale_bf16.x')
  _need(alpha, F32, 'scale_bf16.alpha')
  _lib.check(_lib.load().plm_scale_bf16(_p(x), x.numel(), _p(alpha), _stream()), 'plm_scale_bf16')
  return x


def axpy_f32_(out, x, alpha=None, accumulate=True):
  """out <- (accumulate ? out : 0) + alpha * x; alpha a 0-d fp32 device tensor (None = 1)."""
  _need(out, F32, 'axpy.out')
  _need(x, F32, 'axpy.x')
  if out.numel() != x.numel():
    raise ValueError('axpy_f32_: sizes differ')
  if alpha is not None:
    _need(alpha, F32, 'axpy.alpha')
  _lib.check(_lib.load().plm_axpy_f32(_p(out), _p(x), x.numel(), _p(alpha), int(bool(accumulate)), _stream()), 'plm_axpy_f32')
  return out


# ---- optimizer tail ---------------------------------------------------------------------
def sumsq(x, scratch=None):
  _need(x, F32, 'sumsq.x')
  scratch = torch.empty(4096, dtype=F32, device=x.device) if scratch is None else scratch
  out = torch.empty((), dtype=F32, device=x.device)
  _lib.check(_lib.load().plm_sumsq_f32(_p(x), x.numel(), _p(scratch), _p(out), _stream()), 'plm_sumsq_f32')
  return out


_OPTIM_KINDS = {'adamw': _lib.OPTIM_ADAMW, 'nadamw': _lib.OPTIM_NADAMW, 'sgd': _lib.OPTIM_SGD, 'signSGD': _lib.OPTIM_SIGNSGD, 'sfo_adamw': _lib.OPTIM_SFO_ADAMW}


def optim_hparams(kind, lr, weight_decay=0.0, first=False, beta1=0.0, beta2=0.0, eps=0.0, momentum=0.0, dampening=0.0, bc2=1.0,
                  coef_grad=0.0, coef_avg=0.0, ckp1=0.0, bc1=1.0):
  """struct plm_optim_hparams for optim_ / optim_cast_multi_.  kind: 'adamw' | 'nadamw' | 'sgd' | 'signSGD' | 'sfo_adamw' (an int is
  passed through as is).  decay = 1 - lr * weight_decay is formed here in double and rounded once, the value torch hands to p.mul_(); for
  'sfo_adamw' (lr = the group's warmed-up scheduled_lr, ckp1 = weight / weight_sum) so is the y coefficient lr (beta1 (1 - ckp1) - 1),
  the alpha of the package's y.add_().  'adamw' takes bc1 = 1 - beta1^t and bc2 = 1 - beta2^t; the library forms its decay and step
  size itself, in fp32."""
  k = _OPTIM_KINDS[kind] if isinstance(kind, str) else int(kind)
  return _lib.OptimHparams(k, int(bool(first)), lr, weight_decay, 1.0 - lr * weight_decay, beta1, beta2, eps, momentum, dampening, bc2,
                           coef_grad, coef_avg, ckp1, lr * (beta1 * (1.0 - ckp1) - 1.0), bc1)


def sfo_scalars(group):
  """Schedule-free AdamW's per-step host scalars for one parameter group (a dict with the package's keys: lr, betas, k,
  warmup_steps, r, weight_lr_power, lr_max, weight_sum), in Python floats as the schedulefree package forms them.  Advances the
  group's k / lr_max / weight_sum / scheduled_lr and returns (scheduled lr, ckp1, bc2)."""
  k, warmup = group['k'], group['warmup_steps']
  sched = (k + 1) / warmup if k < warmup else 1.0
  lr = group['lr'] * sched
  group['scheduled_lr'] = lr
  lr_max = group['lr_max'] = max(lr, group['lr_max'])
  weight = (k + 1) ** group['r'] * lr_max ** group['weight_lr_power']
  weight_sum = group['weight_sum'] = group['weight_sum'] + weight
  ckp1 = weight / weight_sum if weight_sum != 0 else 0.0
  bc2 = 1.0 - group['betas'][1] ** (k + 1)
  group['k'] = k + 1
  return lr, ckp1, bc2


def nadam_scalars(lr, beta1, beta2, momentum_decay, step, mu_product):
  """torch.optim.NAdam's per-step host scalars for step `step` (1-based), given the product of the earlier steps' mu.
  Returns (bc2, coef_grad, coef_avg, mu_product including this step's mu)."""
  mu = beta1 * (1.0 - 0.5 * 0.96 ** (step * momentum_decay))
  mu_next = beta1 * (1.0 - 0.5 * 0.96 ** ((step + 1) * momentum_decay))
  mu_product = mu_product * mu
  return 1.0 - beta2 ** step, lr * (1.0 - mu) / (1.0 - mu_product), lr * mu_next / (1.0 - mu_product * mu_next), mu_product


def optim_(hp, p, g, m, v, clip_coef=None):
  """One optimizer step (any kind) on a flat fp32 span (hp from optim_hparams).  m / v: None where the kind has no such buffer."""
  for t, n in ((p, 'p'), (g, 'g'), (m, 'm'), (v, 'v')):
    if t is not None:
      _need(t, F32, 'optim.' + n)
      if t.numel() != p.numel():
        raise ValueError(f'optim.{n}: {t.numel()} elements, p has {p.numel()}')
  _lib.check(_lib.load().plm_optim_f32(C.byref(hp), _p(p), _p(g), _p(m), _p(v), p.numel(), _p(clip_coef), _stream()), 'plm_optim_f32')


def optim_cast_multi_(hp, items, clip_coef=None, table=None):
  """optim_ on a list of Linear weights that also writes their bf16 shadows: items = [(p, g, m, v fp32 [rows, cols], dst bf16
  [rows, cols], dst_t bf16 [cols, >= rows])], with v (and m for SGD without momentum) None where the kind has no such buffer.  Returns the ctypes item table; pass it back as `table` on later steps."""
  if table is None:
    table = (_lib.OptimItem * len(items))()
    for i, (p, g, m, v, dst, dst_t) in enumerate(items):
      for t, n in ((p, 'p'), (g, 'g'), (m, 'm'), (v, 'v')):
        if t is not None:
          _need(t, F32, 'optim_cast_multi.' + n, 2)
          if t.shape != p.shape:
            raise ValueError(f'optim_cast_multi.{n}: shape {tuple(t.shape)}, p has {tuple(p.shape)}')
      R, Cc = p.shape
      _need_shadows(dst, dst_t, R, Cc, 'optim_cast_multi.dst')
      ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
      table[i] = _lib.OptimItem(p.data_ptr(), g.data_ptr(), ptr(m), ptr(v), dst.data_ptr(), dst_t.data_ptr(), R, Cc, dst_t.stride(0))
  _lib.check(_lib.load().plm_optim_cast_multi(C.byref(hp), table, len(table), _p(clip_coef), _stream()), 'plm_optim_cast_multi')
  return table


def lerp_(p, z, w):
  """p <- torch.lerp(p, z, w) in place on a flat fp32 span: the schedule-free train / eval swap."""
  _need(p, F32, 'lerp.p')
  _need(z, F32, 'lerp.z')
  if z.numel() != p.numel():
    raise ValueError(f'lerp.z: {z.numel()} elements, p has {p.numel()}')
  _lib.check(_lib.load().plm_lerp_f32(_p(p), _p(z), p.numel(), float(w), _stream()), 'plm_lerp_f32')
  return p


# ---- probes -------------------------------------------------------------------------------
def probe_ds_read_tr16():
  out = torch.empty(256, dtype=torch.int32, device='cuda')
  _lib.check(_lib.load().plm_probe_ds_read_tr16(_p(out), _stream()), 'plm_probe_ds_read_tr16')
  return out.view(64, 4)


def probe_mfma32(A, B):
  _need(A, F32, 'probe.A', 2)
  _need(B, F32, 'probe.B', 2)
  out = torch.empty((32, 32), dtype=F32, device=A.device)
  _lib.check(_lib.load().plm_probe_mfma32(_p(A), _p(B), _p(out), _stream()), 'plm_probe_mfma32')
  return out


# ---- draft-free speculative decoding: the two wrappers live in ops_lookup.py, on this module's contract ------
from .ops_lookup import LookupDraft, lookup_draft, spec_verify_lookup  # noqa: E402,F401

# ---- the fused decode step: its wrappers live in ops_decode.py, on this module's contract ---------------------------
from .ops_decode import (DECODE_MLP_KINDS, FUSED_DECODE_MAX_ROWS, decode_gemm_residual, decode_layer, decode_layer_workspace,  # noqa: E402,F401
                         decode_norm_fc1_act, decode_norm_qkv_append)
# ---- the fused extend: chunk rows on the same kernels, same module ------------------------------------------------------
from .ops_decode import FUSED_EXTEND_MAX_ROWS, extend_layer, extend_layer_workspace, extend_norm_qkv_append  # noqa: E402,F401
# ---- the FP8 KV cache: its wrappers live in ops_kv8.py, on this module's and ops_decode.py's contract ------------------
from .ops_kv8 import (KV8_BLOCK, attn_decode_kv8, attn_extend_kv8, decode_layer_kv8, extend_layer_kv8,  # noqa: E402,F401
                      extend_norm_qkv_append_kv8, kv8_append_rope_rows, kv8_dequant_rows, kv8_quant_rows, kv8_row_bytes)
# ---- the Muon tail: batched NT GEMM, prepare / orthogonalize / apply; its wrappers live in ops_muon.py -------------------
from .ops_muon import (MUON_ADJUST_LR, MUON_EPS, MUON_NS_COEFFICIENTS, NT_BATCH_GROUP, gemm_nt_batched, muon_adjusted_lr, muon_apply,  # noqa: E402,F401
                       muon_arena, muon_blocks, muon_items, muon_layout, muon_ns_flops, muon_orthogonalize, muon_prepare, muon_set_lr,
                       muon_workspace, muon_workspace_bytes)
