"""The ops wrappers of the Muon tail: ``ops.gemm_nt_batched`` (one launch over a list of NT problems with an
``alpha * acc + beta * D`` epilogue and an optional transposed second output), ``ops.muon_workspace`` / ``ops.muon_layout`` (the shared
workspace and where each matrix's blocks lie in it), ``ops.muon_prepare`` (momentum, norm, X0), ``ops.muon_orthogonalize`` (the
Newton-Schulz steps, three batched launches each) and ``ops.muon_apply`` (the update, with the bf16 shadows written in the same pass).

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract - the operand validator (``ops._need``), the launch
bracket (``ops._Launch``), the workspace arena of the current stream, ``_lib.check`` around the one library call - and, like every wrapper
there, launch hand-written gfx950 kernels with no torch fallback.  They live in a module of their own for ops_lookup.py's reason:
tests/test_ops_trace_host.py holds every function defined in ops.py to a trace recorded on an earlier commit."""

import collections
import ctypes as C
import math

import torch

from . import _lib
from . import ops as O

NT_BATCH_GROUP = _lib.NT_BATCH_GROUP
MUON_NS_COEFFICIENTS = (3.4445, -4.7750, 2.0315)  # torch.optim._muon DEFAULT_A / B / C
MUON_EPS = 1e-7                                   # torch.optim._muon EPS
MUON_ADJUST_LR = ('match_rms_adamw', 'original')

MuonBlocks = collections.namedtuple('MuonBlocks', 'm n x xt a bm')  # bf16 element offsets; x / xt are pairs (ping, pong)


def muon_adjusted_lr(lr, adjust_lr, rows, cols):
  """torch.optim._muon._adjust_lr: the learning rate of one [rows, cols] matrix, in Python floats."""
  if adjust_lr == 'match_rms_adamw':
    return lr * (0.2 * math.sqrt(max(rows, cols)))
  if adjust_lr == 'original':
    return lr * math.sqrt(max(1, rows / cols))
  raise ValueError(f'muon_adjust_lr: {adjust_lr!r} is not one of {MUON_ADJUST_LR}')


def gemm_nt_batched(problems):
  """One library call (one launch per NT_BATCH_GROUP problems) over problems = [(A, B, C, D, Ct, alpha, beta)]:
  C[M, N] = bf16(alpha * (A[M, K] @ B[N, K]^T) + beta * float(D)), Ct = C^T when given.  Every operand is a 2-D bf16 GPU tensor with
  unit inner stride (rows any multiple of 8 apart); D and Ct may be None; D may be C.  M, N, K are multiples of 8.  Returns the Cs."""
  if not problems:
    raise ValueError('gemm_nt_batched: empty problem list')
  table = (_lib.NtBatchItem * len(problems))()
  flops = 0.0
  for i, (A, B, Cm, D, Ct, alpha, beta) in enumerate(problems):
    for t, n in ((A, 'A'), (B, 'B'), (Cm, 'C'), (D, 'D'), (Ct, 'Ct')):
      if t is not None:
        O._need(t, O.BF16, f'gemm_nt_batched[{i}].{n}', strided=True)
    M, K = A.shape
    N = B.shape[0]
    if B.shape[1] != K or tuple(Cm.shape) != (M, N) or (D is not None and tuple(D.shape) != (M, N)) or \
       (Ct is not None and tuple(Ct.shape) != (N, M)):
      raise ValueError(f'gemm_nt_batched[{i}]: A {tuple(A.shape)}, B {tuple(B.shape)}, C {tuple(Cm.shape)}, '
                       f'D {None if D is None else tuple(D.shape)}, Ct {None if Ct is None else tuple(Ct.shape)} do not fit')
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    ld = lambda t: t.stride(0) if t is not None else 0       # noqa: E731
    table[i] = _lib.NtBatchItem(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), Cm.data_ptr(), Cm.stride(0), ptr(D), ld(D), ptr(Ct), ld(Ct),
                                M, N, K, float(alpha), float(beta))
    flops += 2.0 * M * N * K
  with O._Launch('gemm_nt_batched', flops):
    _lib.check(_lib.load().plm_gemm_bf16_nt_batched(table, len(table), O._stream()), 'plm_gemm_bf16_nt_batched')
  return [p[2] for p in problems]


def _shape_arrays(shapes):
  n = len(shapes)
  return (C.c_int64 * n)(*[int(r) for r, _ in shapes]), (C.c_int64 * n)(*[int(c) for _, c in shapes]), n


def muon_workspace_bytes(shapes):
  """plm_muon_workspace_bytes for shapes = [(rows, cols)]: a function of the shapes alone.  A list the library refuses raises."""
  if not shapes:
    raise ValueError('muon_workspace_bytes: empty shape list')
  rows, cols, n = _shape_arrays(shapes)
  nbytes = int(_lib.load().plm_muon_workspace_bytes(rows, cols, n))
  if nbytes == 0:
    raise ValueError(f'muon_workspace_bytes: unsupported shapes {list(shapes)} (rows and cols are positive multiples of 8, rows * cols < 2^30)')
  return nbytes


def muon_layout(shapes):
  """Where each matrix's blocks lie in the workspace (the layout include/plainlm_hip.h states): ([MuonBlocks], bytes of the blocks,
  number of fp32 partial sums that follow them)."""
  out, el, tiles = [], 0, 0
  for rows, cols in shapes:
    m, n = min(rows, cols), max(rows, cols)
    out.append(MuonBlocks(m, n, (el, el + 2 * m * n), (el + m * n, el + 3 * m * n), el + 4 * m * n, el + 4 * m * n + m * m))
    el += 4 * m * n + 2 * m * m
    tiles += -(-rows // 64) * -(-cols // 64)
  return out, 2 * el, tiles


def muon_workspace(shapes, device):
  """A caller-owned (uint8 workspace, bytes) pair for the three muon calls over these shapes."""
  nbytes = muon_workspace_bytes(shapes)
  return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def muon_arena(shapes, device):
  """The (workspace, bytes) pair of the current stream's arena for these shapes: pass it to the three calls of one tail, which share
  its contents (nothing else may use the arena in between)."""
  nbytes = muon_workspace_bytes(shapes)
  return O._workspace(device, nbytes, O._stream()), nbytes


def muon_blocks(workspace, shapes, steps=None):
  """bf16 views into a workspace, per matrix: dict(x0, x0t, x1, x1t, a, bm) - and o, the result of ``steps`` steps in the weight's
  layout ([rows, cols]: X of a wide weight, Xt of a tall one), when steps is given."""
  ws = workspace[0] if isinstance(workspace, tuple) else workspace
  flat = ws.view(O.BF16)
  views = []
  for (rows, cols), b in zip(shapes, muon_layout(shapes)[0]):
    v = dict(x0=flat[b.x[0]:b.x[0] + b.m * b.n].view(b.m, b.n), x0t=flat[b.xt[0]:b.xt[0] + b.m * b.n].view(b.n, b.m),
             x1=flat[b.x[1]:b.x[1] + b.m * b.n].view(b.m, b.n), x1t=flat[b.xt[1]:b.xt[1] + b.m * b.n].view(b.n, b.m),
             a=flat[b.a:b.a + b.m * b.m].view(b.m, b.m), bm=flat[b.bm:b.bm + b.m * b.m].view(b.m, b.m))
    if steps is not None:
      v['o'] = v[('x%d' if rows <= cols else 'x%dt') % (steps & 1)]
    views.append(v)
  return views


def _muon_ws(name, shapes, workspace, device, stream):
  nbytes = muon_workspace_bytes(shapes)
  if workspace is None:
    return O._workspace(device, nbytes, stream), nbytes
  ws, given = workspace
  O._need(ws, torch.uint8, f'{name}.workspace', 1)
  return ws, given


def muon_items(items, lr_adj=None):
  """The ctypes table of struct plm_muon_item for items = [(p, g, buf fp32 [rows, cols], dst bf16 [rows, cols] or None, dst_t bf16
  [cols, >= rows] or None)]; lr_adj: one adjusted learning rate per item (plm_muon_apply).  Returns (table, shapes)."""
  table = (_lib.MuonItem * len(items))()
  shapes = []
  for i, (p, g, buf, dst, dst_t) in enumerate(items):
    for t, n in ((p, 'p'), (g, 'g'), (buf, 'buf')):
      if t is not None:
        O._need(t, O.F32, f'muon[{i}].{n}', 2)
    ref = p if p is not None else g
    R, Cc = ref.shape
    for t in (g, buf):
      if t is not None and tuple(t.shape) != (R, Cc):
        raise ValueError(f'muon[{i}]: shapes {tuple(t.shape)} and {(R, Cc)} differ')
    if dst_t is not None:
      O._need_shadows(dst, dst_t, R, Cc, f'muon[{i}].dst')
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    table[i] = _lib.MuonItem(ptr(p), ptr(g), ptr(buf), ptr(dst), ptr(dst_t), R, Cc, dst_t.stride(0) if dst_t is not None else R,
                             0.0 if lr_adj is None else lr_adj[i])
    shapes.append((R, Cc))
  return table, shapes


def muon_set_lr(table, lr_adj):
  for i, v in enumerate(lr_adj):
    table[i].lr_adj = v


def muon_prepare(table, shapes, momentum, nesterov, nrm, clip_coef=None, eps=MUON_EPS, workspace=None):
  """Steps 1-6 of the Muon update for a list of matrices (table, shapes from muon_items): the momentum buffers are updated in place, X0
  and X0^T go into the workspace, the per-matrix norms into nrm (fp32 [count]).  Returns nrm."""
  O._need(nrm, O.F32, 'muon_prepare.nrm', 1)
  if nrm.numel() < len(table):
    raise ValueError(f'muon_prepare.nrm: {nrm.numel()} elements for {len(table)} matrices')
  if clip_coef is not None:
    O._need(clip_coef, O.F32, 'muon_prepare.clip_coef')
  stream = O._stream()
  ws, nbytes = _muon_ws('muon_prepare', shapes, workspace, nrm.device, stream)
  with O._Launch('hbm:muon_prepare', 14.0 * sum(r * c for r, c in shapes)):
    _lib.check(_lib.load().plm_muon_prepare(table, len(table), float(momentum), int(bool(nesterov)), float(eps), O._p(clip_coef), O._p(nrm),
                                            O._p(ws), nbytes, stream), 'plm_muon_prepare')
  return nrm


def muon_ns_flops(shapes, steps):
  return float(steps) * sum(2.0 * min(r, c) ** 2 * (2 * max(r, c) + min(r, c)) for r, c in shapes)


def muon_orthogonalize(shapes, steps, device, coefficients=MUON_NS_COEFFICIENTS, workspace=None):
  """``steps`` Newton-Schulz steps on every X of the workspace from one library call (steps x 3 batched launches per NT_BATCH_GROUP
  matrices).  The result is block x{steps & 1} (and its transpose)."""
  rows, cols, n = _shape_arrays(shapes)
  a, b, c = (float(v) for v in coefficients)
  stream = O._stream()
  launch = O._Launch('muon_ns', muon_ns_flops(shapes, steps))
  ws, nbytes = _muon_ws('muon_orthogonalize', shapes, workspace, device, stream)
  with launch:
    _lib.check(_lib.load().plm_muon_orthogonalize(rows, cols, n, int(steps), a, b, c, O._p(ws), nbytes, stream), 'plm_muon_orthogonalize')


def muon_apply(table, shapes, decay, steps, device, workspace=None):
  """W = fma(-lr_adj, float(O), W * decay) for every item of the table, O the result of ``steps`` steps in the workspace; the bf16
  shadows dst / dst_t are written in the same pass."""
  stream = O._stream()
  ws, nbytes = _muon_ws('muon_apply', shapes, workspace, device, stream)
  with O._Launch('hbm:muon_apply', 14.0 * sum(r * c for r, c in shapes)):
    _lib.check(_lib.load().plm_muon_apply(table, len(table), float(decay), int(steps), O._p(ws), nbytes, stream), 'plm_muon_apply')
