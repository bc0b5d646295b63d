"""The bf16 GEMMs against oracle/parity_gemm.py's error budget on a real MI355X: every NT variant (the hybrid whole-K +
stream-K schedule included), TN whole-K and split-K, and the grouped TN launch, on four input classes and alphas that are no
powers of two, with strided operands, K tails, and C and the workspace inside guarded buffers.  References are fp64 from the
operands the kernel read (cross-checked against the host inside ``reference``); tests/test_parity_budget_gemm.py calibrates
the same budget on the CPU.  Also: a NaN or Inf in one operand row stays in its output row (the engine's NaN check relies
on it), and the hybrid, split and grouped schedules are deterministic."""

import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import parity_gemm as G  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
GUARD = 264          # guard rows above and below C: more than one tile of rows
PAD = 8              # pad columns of C
PAT = {BF16: (torch.int16, 0x5A5B), F32: (torch.int32, 0x5A5B5A5B)}
WS_GUARD = 4096      # guard bytes on each side of a workspace


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


@pytest.fixture
def plm_env(monkeypatch, ops):
  def set_(name, value):
    monkeypatch.setenv(name, value)
    ops.reload_env()
  yield set_
  monkeypatch.undo()
  ops.reload_env()


def lib():
  from plainlm_amd import _lib
  return _lib.load()


# --------------------------------------------------------------------------------------
# guarded buffers
# --------------------------------------------------------------------------------------
class GuardedC:
  """C [M, N] inside a [GUARD + M + GUARD, N + PAD] buffer of a fixed bit pattern."""

  def __init__(self, M, N, dtype, c0=None):
    it, pat = PAT[dtype]
    self.M, self.N = M, N
    self.buf = torch.full((2 * GUARD + M, N + PAD), pat, dtype=it, device='cuda')
    self.pat = pat
    self.c = self.buf.view(dtype)[GUARD:GUARD + M, :N]
    if c0 is not None:
      self.c.copy_(c0)

  def intact(self):
    b, M, N = self.buf, self.M, self.N
    return bool((b[:GUARD] == self.pat).all() and (b[GUARD + M:] == self.pat).all() and (b[GUARD:GUARD + M, N:] == self.pat).all())


class GuardedWs:
  def __init__(self, nbytes):
    self.nbytes = nbytes
    self.buf = torch.full((2 * WS_GUARD + nbytes,), 0xA5, dtype=torch.uint8, device='cuda')
    self.ws = self.buf[WS_GUARD:WS_GUARD + nbytes]

  def intact(self):
    return bool((self.buf[:WS_GUARD] == 0xA5).all() and (self.buf[WS_GUARD + self.nbytes:] == 0xA5).all())


def dev_alpha(alpha):
  return None if alpha is None else torch.tensor(alpha, dtype=F32, device='cuda')


def bits(t):
  return t.view(PAT[t.dtype][0])


# --------------------------------------------------------------------------------------
# launches: through ops, or through the C ABI when the call takes a workspace (so that it can sit between guards)
# --------------------------------------------------------------------------------------
def launch_nt(ops, A, B, alpha, variant=0, dtype=BF16, c0=None, use_ws=True):
  """-> (C view, workspace bytes used).  C and the workspace are guarded; asserts the guards."""
  from plainlm_amd import _lib
  M, K = A.shape
  N = B.shape[0]
  gc = GuardedC(M, N, dtype, c0)
  al = dev_alpha(alpha)
  nbytes = int(lib().plm_gemm_nt_workspace_bytes(M, N, K)) if (use_ws and variant == 0 and dtype == BF16) else 0
  if nbytes:
    gw = GuardedWs(nbytes)
    _lib.check(lib().plm_gemm_bf16_nt_ws(ops._p(A), A.stride(0), ops._p(B), B.stride(0), ops._p(gc.c), gc.c.stride(0), M, N, K, 0, 0,
                                         ops._p(al), 0, ops._p(gw.ws), nbytes, ops._stream()), 'plm_gemm_bf16_nt_ws')
    assert gw.intact(), 'gemm_nt wrote outside its workspace'
  elif use_ws:
    ops.gemm_nt(A, B, out=gc.c, accumulate=c0 is not None, alpha=al, variant=variant)
  else:  # the plain schedule of a shape that would take the hybrid one: no workspace given
    _lib.check(lib().plm_gemm_bf16_nt_ws(ops._p(A), A.stride(0), ops._p(B), B.stride(0), ops._p(gc.c), gc.c.stride(0), M, N, K, 0, 0,
                                         ops._p(al), 0, C.c_void_p(0), 0, ops._stream()), 'plm_gemm_bf16_nt_ws')
  assert gc.intact(), 'gemm_nt wrote outside C'
  return gc.c, nbytes


def launch_tn(ops, A, B, alpha, c0=None):
  from plainlm_amd import _lib
  K, M = A.shape
  N = B.shape[1]
  gc = GuardedC(M, N, F32, c0)
  al = dev_alpha(alpha)
  nbytes = int(lib().plm_gemm_tn_workspace_bytes(M, N, K))
  gw = GuardedWs(nbytes)
  _lib.check(lib().plm_gemm_bf16_tn(ops._p(A), A.stride(0), ops._p(B), B.stride(0), ops._p(gc.c), gc.c.stride(0), M, N, K,
                                    int(c0 is not None), ops._p(al), ops._p(gw.ws) if nbytes else C.c_void_p(0), nbytes, ops._stream()),
             'plm_gemm_bf16_tn')
  assert gw.intact(), 'gemm_tn wrote outside its workspace'
  assert gc.intact(), 'gemm_tn wrote outside C'
  return gc.c, nbytes


def launch_grouped(ops, As, Bs, alpha, c0s=None):
  from plainlm_amd import _lib
  n, K = len(As), As[0].shape[0]
  gcs = [GuardedC(a.shape[1], b.shape[1], F32, None if c0s is None else c0) for a, b, c0 in zip(As, Bs, c0s or [None] * n)]
  al = dev_alpha(alpha)
  arr = (_lib.TnProblem * n)()
  Ms, Ns = (C.c_int64 * n)(), (C.c_int64 * n)()
  for i, (a, b, gc) in enumerate(zip(As, Bs, gcs)):
    Ms[i], Ns[i] = a.shape[1], b.shape[1]
    arr[i] = _lib.TnProblem(ops._p(a), a.stride(0), ops._p(b), b.stride(0), ops._p(gc.c), gc.c.stride(0), Ms[i], Ns[i], int(c0s is not None),
                            ops._p(al))
  nbytes = int(lib().plm_gemm_tn_grouped_workspace_bytes(Ms, Ns, n, K))
  assert nbytes > 0, 'shapes cannot be grouped'
  gw = GuardedWs(nbytes)
  _lib.check(lib().plm_gemm_bf16_tn_grouped(arr, n, K, ops._p(gw.ws), nbytes, ops._stream()), 'plm_gemm_bf16_tn_grouped')
  assert gw.intact(), 'gemm_tn_grouped wrote outside its workspace'
  assert all(gc.intact() for gc in gcs), 'gemm_tn_grouped wrote outside a C'
  return [gc.c for gc in gcs], nbytes


def nt_operands(cls, M, N, K, seed, strided=False):
  """A [M, K], B [N, K]; strided: column blocks [:, 8:8+K] and [:, K+24:2K+24] of [rows, 2K+32] buffers (16-byte aligned bases
  that are not 128-byte aligned, row strides above K: the q|k|v and x|z blocks)."""
  if not strided:
    return G.operand(cls, M, K, seed, 'cuda'), G.operand(cls, N, K, seed + 1, 'cuda')
  wa, wb = G.operand(cls, M, 2 * K + 32, seed, 'cuda'), G.operand(cls, N, 2 * K + 32, seed + 1, 'cuda')
  return wa[:, 8:8 + K], wb[:, K + 24:2 * K + 24]


def tn_operands(cls, M, N, K, seed, padded=False):
  """A [K, M], B [K, N] (class structure along K, as for NT); padded: lda = M + 8, ldb = N + 16."""
  A, B = G.operand(cls, M, K, seed, 'cuda').t(), G.operand(cls, N, K, seed + 1, 'cuda').t()
  if not padded:
    return A.contiguous(), B.contiguous()
  wa = torch.zeros(K, M + 8, dtype=BF16, device='cuda')
  wb = torch.zeros(K, N + 16, dtype=BF16, device='cuda')
  wa[:, :M], wb[:, :N] = A, B
  return wa[:, :M], wb[:, :N]


def c0_like(M, N, seed):
  return torch.randn(M, N, generator=torch.Generator(device='cuda').manual_seed(seed), device='cuda')


# --------------------------------------------------------------------------------------
# NT
# --------------------------------------------------------------------------------------
# (M, N, K, class, alpha index): the step's shapes (160M: 32768 tokens, d 768, h 2048; lm_head rows; 420M: 16384 tokens, d 1024)
NT_AUTO = [(4096, 768, 2048, 'randn', 1), (1000, 2304, 768, 'wide', 2), (64, 50280, 768, 'pos', 3), (300, 768, 50304, 'pos', 3),
           (32768, 2304, 768, 'blocky', 1), (32768, 768, 2048, 'wide', 0), (16384, 3072, 1024, 'blocky', 2), (16384, 5632, 1024, 'wide', 3),
           (16384, 1024, 1024, 'pos', 1), (128, 128, 64, 'randn', 2), (256, 384, 64, 'pos', 0)]


@pytest.mark.parametrize('M,N,K,cls,ai', NT_AUTO)
def test_nt_auto_bf16(ops, M, N, K, cls, ai):
  A, B = nt_operands(cls, M, N, K, M + N + K)
  out, _ = launch_nt(ops, A, B, G.ALPHAS[ai])
  G.check(G.metrics(out, G.reference(A, B, G.ALPHAS[ai]), G.NT_TILES[0]), f'nt v0 bf16 {M}x{N}x{K} {cls} alpha={G.ALPHAS[ai]}')


# variants 0 / 1 / 2 with fp32 C, overwrite and accumulate; K tails (K % 64 != 0: the register-staged kernel) at M >= 2048
NT_F32 = [(0, 1000, 2304, 768, 'randn', 1), (1, 1000, 2304, 768, 'wide', 2), (2, 1000, 2304, 768, 'pos', 3), (0, 4096, 768, 2048, 'pos', 2),
          (1, 4096, 768, 2048, 'blocky', 3), (2, 4096, 768, 2048, 'wide', 1), (0, 2048, 392, 72, 'pos', 1), (1, 2048, 392, 72, 'randn', 2),
          (0, 2056, 264, 200, 'wide', 3), (1, 2056, 264, 200, 'pos', 0), (0, 2048, 256, 4104, 'randn', 2), (1, 2048, 256, 4104, 'pos', 1),
          (0, 16384, 1024, 1024, 'randn', 3), (2, 300, 768, 50304, 'pos', 1)]


@pytest.mark.parametrize('variant,M,N,K,cls,ai', NT_F32)
def test_nt_128_tiles_fp32_and_bf16(ops, variant, M, N, K, cls, ai):
  A, B = nt_operands(cls, M, N, K, M + N + K + variant)
  alpha = G.ALPHAS[ai]
  R = G.reference(A, B, alpha)
  tag = f'nt v{variant} {M}x{N}x{K} {cls} alpha={alpha}'
  m = G.metrics(launch_nt(ops, A, B, alpha, variant, F32)[0], R, G.NT_TILES[variant])
  if variant != 0 or K % 64 != 0:   # (variant 0 with bf16 C at K % 64 == 0 is test_nt_auto_bf16's)
    m = G.merge(m, G.metrics(launch_nt(ops, A, B, alpha, variant)[0], R, G.NT_TILES[variant]))
  c0 = c0_like(M, N, K)
  Rc = G.reference(A, B, alpha, c0=c0)
  m = G.merge(m, G.metrics(launch_nt(ops, A, B, alpha, variant, F32, c0=c0)[0], Rc, G.NT_TILES[variant]))
  G.check(m, tag)


# one ragged shape triple per tile geometry: M and N at two tile edges - 8, exactly, + 8
RAGGED = [(v, 2 * bm + d, 2 * bn + d, K, cls, ai)
          for v, bm, bn, K, cls, ai in ((2, 128, 128, 768, 'randn', 1), (3, 256, 256, 1024, 'wide', 2), (4, 256, 256, 768, 'pos', 3),
                                        (5, 256, 192, 1024, 'blocky', 1), (6, 256, 128, 768, 'wide', 2), (7, 128, 192, 1024, 'pos', 1))
          for d in (-8, 0, 8)]
BIG_VARIANTS = [(3, 32768, 768, 768, 'randn', 2), (4, 32768, 2304, 768, 'pos', 1), (5, 32768, 768, 2048, 'randn', 3), (6, 16384, 1024, 1024, 'wide', 1),
                (7, 8192, 2304, 768, 'blocky', 2), (4, 4096, 768, 4096, 'blocky', 0)]


@pytest.mark.parametrize('variant,M,N,K,cls,ai', RAGGED + BIG_VARIANTS)
def test_nt_variants(ops, variant, M, N, K, cls, ai):
  A, B = nt_operands(cls, M, N, K, M + N + K + variant)
  out, _ = launch_nt(ops, A, B, G.ALPHAS[ai], variant)
  G.check(G.metrics(out, G.reference(A, B, G.ALPHAS[ai]), G.NT_TILES[variant]), f'nt v{variant} bf16 {M}x{N}x{K} {cls} alpha={G.ALPHAS[ai]}')


HYBRID = [(32768, 768, 768, 'randn', 1, False), (32768, 768, 2048, 'pos', 2, True), (32700, 1032, 1024, 'wide', 3, False),
          (32768, 768, 4096, 'blocky', 1, False), (32768, 768, 50304, 'randn', 3, False), (32768, 768, 16384, 'pos', 3, False)]


@pytest.mark.parametrize('M,N,K,cls,ai,strided', HYBRID)
def test_nt_hybrid(ops, plm_env, M, N, K, cls, ai, strided):
  """Variant 0 with a workspace (whole-K + stream-K + nt_streamk_reduce_kernel) and without one (the plain schedule on the
  same shape), both under the budget; the hybrid run twice, bit-equal."""
  plm_env('PLM_NT_HYBRID_MIN_K', '64')
  A, B = nt_operands(cls, M, N, K, M + N + K, strided)
  alpha = G.ALPHAS[ai]
  R = G.reference(A, B, alpha)
  hyb, nbytes = launch_nt(ops, A, B, alpha)
  assert nbytes > 0, 'shape does not exercise the hybrid schedule'
  G.check(G.metrics(hyb, R, ((256, 256),)), f'nt hybrid {M}x{N}x{K} {cls} alpha={alpha} strided={strided}')
  again, _ = launch_nt(ops, A, B, alpha)
  assert torch.equal(bits(hyb), bits(again)), 'hybrid schedule is not deterministic'
  plain, nb0 = launch_nt(ops, A, B, alpha, use_ws=False)
  assert nb0 == 0
  G.check(G.metrics(plain, R, G.NT_TILES[0]), f'nt v0 no workspace {M}x{N}x{K} {cls} alpha={alpha}')


@pytest.mark.parametrize('M,N,K,cls,ai', [(32768, 768, 768, 'wide', 1), (8192, 2304, 768, 'pos', 2)])
def test_nt_strided_operands(ops, M, N, K, cls, ai):
  A, B = nt_operands(cls, M, N, K, M + N + K, strided=True)
  assert A.data_ptr() % 128 != 0 and A.data_ptr() % 16 == 0 and A.stride(0) > K and B.stride(0) > K
  alpha = G.ALPHAS[ai]
  R = G.reference(A, B, alpha)
  m = {}
  for variant in (0, 2):
    m = G.merge(m, G.metrics(launch_nt(ops, A, B, alpha, variant)[0], R, G.NT_TILES[variant]))
  G.check(m, f'nt strided {M}x{N}x{K} {cls} alpha={alpha}')


# --------------------------------------------------------------------------------------
# TN, grouped TN
# --------------------------------------------------------------------------------------
# (M, N, K, class, alpha index, padded strides): whole-K (big and 128x128 kernels), split-K, a K tail
TN_CASES = [(2304, 768, 4096, 'randn', 1, False), (768, 768, 32768, 'pos', 2, True), (50280, 768, 2048, 'wide', 3, False),
            (3072, 1024, 16384, 'blocky', 1, False), (136, 72, 200, 'pos', 2, True), (520, 264, 1024, 'wide', 1, True),
            (1024, 520, 4104, 'pos', 3, False), (128, 128, 64, 'randn', 2, False), (1024, 2816, 16384, 'randn', 3, True)]


@pytest.mark.parametrize('M,N,K,cls,ai,padded', TN_CASES)
def test_tn(ops, M, N, K, cls, ai, padded):
  A, B = tn_operands(cls, M, N, K, M + 3 * N + K, padded)
  alpha = G.ALPHAS[ai]
  out, nbytes = launch_tn(ops, A, B, alpha)
  m = G.metrics(out, G.reference(A, B, alpha, tn=True), G.TN_TILES)
  c0 = c0_like(M, N, K)
  acc, _ = launch_tn(ops, A, B, alpha, c0=c0)
  m = G.merge(m, G.metrics(acc, G.reference(A, B, alpha, tn=True, c0=c0), G.TN_TILES))
  if nbytes:
    assert torch.equal(bits(acc), bits(launch_tn(ops, A, B, alpha, c0=c0)[0])), 'split-K schedule is not deterministic'
  G.check(m, f'tn {M}x{N}x{K} {cls} alpha={alpha} padded={padded} split={nbytes > 0}')


def test_tn_shapes_cover_whole_k_and_split(ops):
  ws = [int(lib().plm_gemm_tn_workspace_bytes(M, N, K)) for M, N, K, *_ in TN_CASES]
  assert any(w > 0 for w in ws) and any(w == 0 for w in ws), ws


GROUPED = [([(1000, 1032), (520, 264), (2304, 768), (136, 72), (3000, 1544), (4096, 776)], 1024, 'wide', 1),
           ([(768, 2048), (4096, 768), (768, 768), (2304, 768)] * 6, 2048, 'pos', 2)]


@pytest.mark.parametrize('shapes,K,cls,ai', GROUPED)
def test_tn_grouped(ops, shapes, K, cls, ai):
  ops_ = [tn_operands(CLS, M, N, K, 7 * i + M + N, padded=(i % 2 == 1))
          for i, ((M, N), CLS) in enumerate(zip(shapes, [cls, 'randn', 'blocky'] * len(shapes)))]
  As, Bs = [a for a, _ in ops_], [b for _, b in ops_]
  alpha = G.ALPHAS[ai]
  outs, _ = launch_grouped(ops, As, Bs, alpha)
  c0s = [c0_like(M, N, i) for i, (M, N) in enumerate(shapes)]
  accs, _ = launch_grouped(ops, As, Bs, alpha, c0s)
  accs2, _ = launch_grouped(ops, As, Bs, alpha, c0s)
  m = {}
  for a, b, o, acc, acc2, c0 in zip(As, Bs, outs, accs, accs2, c0s):
    assert torch.equal(bits(acc), bits(acc2)), 'grouped schedule is not deterministic'
    m = G.merge(m, G.metrics(o, G.reference(a, b, alpha, tn=True), G.TN_TILES), G.metrics(acc, G.reference(a, b, alpha, tn=True, c0=c0), G.TN_TILES))
  G.check(m, f'tn grouped {len(shapes)} problems K={K} {cls} alpha={alpha}')


def test_with_cu_reserve(ops, plm_env):
  """16 CUs reserved for RCCL: the hybrid NT plan and the TN split are recomputed for 240 workgroups; same budget."""
  plm_env('PLM_NT_HYBRID_MIN_K', '64')
  try:
    ops.set_cu_reserve(16)
    M, N, K = 32768, 768, 2048
    A, B = nt_operands('randn', M, N, K, 77)
    out, nbytes = launch_nt(ops, A, B, G.ALPHAS[1])
    assert nbytes > 0, 'no hybrid plan under the reserve'
    G.check(G.metrics(out, G.reference(A, B, G.ALPHAS[1]), ((256, 256),)), f'nt hybrid reserve 16 {M}x{N}x{K}')
    M, N, K = 768, 768, 32768
    A, B = tn_operands('wide', M, N, K, 78)
    c0 = c0_like(M, N, 79)
    acc, nbytes = launch_tn(ops, A, B, G.ALPHAS[2], c0=c0)
    assert nbytes > 0, 'no TN split under the reserve'
    G.check(G.metrics(acc, G.reference(A, B, G.ALPHAS[2], tn=True, c0=c0), G.TN_TILES), f'tn split reserve 16 {M}x{N}x{K}')
  finally:
    ops.set_cu_reserve(0)


# --------------------------------------------------------------------------------------
# a NaN / Inf in one operand row stays in its output row (column); everything else keeps its bits
# --------------------------------------------------------------------------------------
def _localised(run, A, B, a_axis, b_axis, M, N, K, last_row, what):
  """run() -> C [M, N].  Plants one NaN, then one +Inf, at (i, k) of A (row axis a_axis) and (j, k) of B: i, j in {0, a tile's last
  row, the last}, k in the first and the last K tile."""
  clean = run().clone()
  assert torch.isfinite(clean.float()).all()
  for val in (float('nan'), float('inf')):
    for k in (3, K - 5):
      for X, axis, n, rows in ((A, a_axis, M, True), (B, b_axis, N, False)):
        for i in (0, min(last_row, n - 1), n - 1):
          idx = (i, k) if axis == 0 else (k, i)
          keep = X[idx].clone()
          X[idx] = val
          got = run()
          X[idx] = keep
          bad = ~torch.isfinite(got.float())
          line = bad[i] if rows else bad[:, i]
          assert line.all(), f'{what}: {val} at {"A" if rows else "B"}[{i}, {k}] did not reach its whole output {"row" if rows else "column"}'
          same = bits(got) == bits(clean)
          if rows:
            same[i] = True
          else:
            same[:, i] = True
          assert same.all(), f'{what}: {val} at {"A" if rows else "B"}[{i}, {k}] changed other elements'


@pytest.mark.parametrize('variant,bm', [(0, 256), (2, 128), (4, 256), (5, 256), (6, 256), (7, 128)])
def test_nt_nonfinite_stays_in_its_row(ops, variant, bm):
  M, N, K = 776, 520, 192
  A, B = nt_operands('randn', M, N, K, 5 + variant)
  _localised(lambda: launch_nt(ops, A, B, None, variant)[0], A, B, 0, 0, M, N, K, bm - 1, f'nt v{variant}')


def test_nt_hybrid_nonfinite_stays_in_its_row(ops, plm_env):
  plm_env('PLM_NT_HYBRID_MIN_K', '64')
  M, N, K = 32768, 768, 256
  A, B = nt_operands('randn', M, N, K, 15)
  assert launch_nt(ops, A, B, None)[1] > 0, 'shape does not exercise the hybrid schedule'
  _localised(lambda: launch_nt(ops, A, B, None)[0], A, B, 0, 0, M, N, K, 255, 'nt hybrid')


@pytest.mark.parametrize('M,N,K', [(776, 520, 192), (768, 768, 8192)])   # whole-K; split-K
def test_tn_nonfinite_stays_in_its_row(ops, M, N, K):
  A, B = tn_operands('randn', M, N, K, 25)
  _localised(lambda: launch_tn(ops, A, B, None)[0], A, B, 1, 1, M, N, K, 255, f'tn {M}x{N}x{K}')


def test_tn_grouped_nonfinite_stays_in_its_row(ops):
  shapes, K = [(1000, 1032), (520, 264), (2304, 768), (136, 72), (3000, 1544), (4096, 776)], 1024
  ops_ = [tn_operands('randn', M, N, K, 35 + i) for i, (M, N) in enumerate(shapes)]
  As, Bs = [a for a, _ in ops_], [b for _, b in ops_]
  for p in (0, 4):   # a problem in the whole-K rounds and one across the split remainder
    M, N = shapes[p]
    _localised(lambda: launch_grouped(ops, As, Bs, None)[0][p], As[p], Bs[p], 1, 1, M, N, K, 255, f'tn grouped problem {p}')
  clean = launch_grouped(ops, As, Bs, None)[0]
  As[0][7, 3] = float('nan')
  got = launch_grouped(ops, As, Bs, None)[0]
  for p in range(1, len(shapes)):
    assert torch.equal(bits(got[p]), bits(clean[p])), f'a NaN in problem 0 changed problem {p}'
