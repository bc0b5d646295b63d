"""The GEMM error budget (oracle/parity_gemm.py) against planted defects, on the CPU.

Each stand-in is one schedule of csrc/gemm.hip / csrc/gemm_big.hip restated in fp32 torch: whole-K accumulation in 64-wide
K tiles; the hybrid / stream-K NT rows (raw fp32 partials of a few K tiles each, summed, then alpha, then ONE bf16 rounding);
the TN split-K slabs plus splitk_reduce_kernel (sum, alpha, + C0); the grouped TN launch (the same per problem).  It is what an
honest kernel looks like under the budget.  Each defect is a small edit of a stand-in of the kind a rewrite of those kernels
tends to introduce.  The budget must ACCEPT every stand-in at every input class and contraction length of
tests/test_gemm_parity_gpu.py and REJECT every defect by at least 2x its bound, and at least half of the defects pass the
rel-to-max yardsticks of the older GEMM tests (asserted below).  Nothing here launches a kernel."""

import math

import pytest
import torch

from oracle import parity_gemm as G

BF16 = torch.bfloat16


def rb(x):
  return x.to(BF16).float()


def trunc_bf16(x):
  """fp32 -> bf16 by dropping the low 16 bits (what a store without the rounding increment does)."""
  return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def relmax(got, ref):
  got, ref = got.double(), ref.double()
  return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def a32(alpha):
  return torch.tensor(1.0 if alpha is None else alpha, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# stand-ins (with the defects' hooks).  A [M, K], B [N, K] bf16 in every one: TN's operands are these, transposed.
# ---------------------------------------------------------------------------------------------------------------------
def ktile_sum(A, B, k0, k1, defect=None, tile=(0, 0, 256, 256)):
  """fp32 sum over K tiles of 64 from k0 to k1 of A B^T.  Defects act on the output tile (i0, j0, bm, bn)."""
  Af, Bf = A.float(), B.float()
  acc = torch.zeros(A.shape[0], B.shape[0])
  i0, j0, bm, bn = tile
  for k in range(k0, k1, 64):
    part = Af[:, k:min(k + 64, k1)] @ Bf[:, k:min(k + 64, k1)].t()
    if defect == 'skip_last_ktile' and k + 64 >= k1:
      part[i0:i0 + bm, j0:j0 + bn] = 0.0
    acc += part
  if defect == 'drop_term':   # one k-term of one 16-column block of the tile (a lane's operand of one MFMA left out)
    k = k0 + (k1 - k0) // 2 + 5
    acc[i0:i0 + bm, j0 + 16:j0 + 32] -= Af[i0:i0 + bm, k:k + 1] * Bf[j0 + 16:j0 + 32, k][None, :]
  if defect == 'tile_scale':
    acc[i0:i0 + bm, j0:j0 + bn] *= 1 + 2.0 ** -9
  return acc


def store(acc, alpha, dtype, defect=None, c0=None):
  al = a32(alpha)
  if dtype == BF16:
    if defect == 'double_round':
      return rb(al * rb(acc)).to(BF16)
    if defect == 'truncate':
      return trunc_bf16(acc * al).to(BF16)
    return (acc * al).to(BF16)
  v = acc * al
  return v if c0 is None else c0 + v


def nt_whole(A, B, alpha, dtype, defect=None, c0=None):
  """gemm_nt_kernel / gemm_nt_dma_kernel / gemm_nt_big_kernel on the plain schedule."""
  K = A.shape[1]
  acc = ktile_sum(A, B, 0, K, defect)
  out = store(acc, alpha, dtype, defect, c0)
  if defect == 'tail_row_copy':
    out[-1] = out[-2]
  return out


def nt_hybrid(A, B, alpha, L=5, defect=None, rows0=256):
  """Hybrid NT: rows < rows0 whole-K, the rest as stream-K runs of L K-tiles whose raw fp32 partials nt_streamk_reduce_kernel
  sums, scales and rounds once."""
  K = A.shape[1]
  al = a32(alpha)
  out = torch.empty(A.shape[0], B.shape[0], dtype=BF16)
  out[:rows0] = store(ktile_sum(A[:rows0], B, 0, K), alpha, BF16)
  s = torch.zeros(A.shape[0] - rows0, B.shape[0])
  for n, k0 in enumerate(range(0, K, 64 * L)):
    part = ktile_sum(A[rows0:], B, k0, min(k0 + 64 * L, K))
    if defect == 'bf16_partials':
      part = rb(part)
    s += part
  if defect == 'alpha_twice':
    s = s * al
  out[rows0:] = (s if defect == 'alpha_missing' else s * al).to(BF16)
  return out


def tn_split(A, B, alpha, splits, c0=None, defect=None, rows0=0):
  """TN: rows < rows0 whole-K in the GEMM kernel's epilogue, the rest as ``splits`` slabs + splitk_reduce_kernel."""
  K = A.shape[1]
  al = a32(alpha)
  out = torch.empty(A.shape[0], B.shape[0])
  if rows0:
    out[:rows0] = store(ktile_sum(A[:rows0], B, 0, K), alpha, torch.float32, None, None if c0 is None else c0[:rows0])
  kchunk = -(-(-(-K // splits)) // 64) * 64
  s = torch.zeros(A.shape[0] - rows0, B.shape[0])
  for n in range(splits):
    if n * kchunk >= K:
      break
    part = ktile_sum(A[rows0:], B, n * kchunk, min((n + 1) * kchunk, K))
    if defect == 'slab_scale' and n == 1:
      part *= 1 + 2.0 ** -9
    s += part
  s = s * al
  out[rows0:] = s if (c0 is None or defect == 'accumulate_ignored') else s + c0[rows0:]
  return out


def case(cls, M, N, K, seed):
  return G.operand(cls, M, K, seed), G.operand(cls, N, K, seed + 1)


TILE = ((256, 256),)


# ---------------------------------------------------------------------------------------------------------------------
# the budget accepts every stand-in
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cls', G.CLASSES)
@pytest.mark.parametrize('K', G.KS)
def test_budget_accepts_the_standins(cls, K):
  M = N = 512 if K <= 4104 else 256
  A, B = case(cls, M, N, K, K + len(cls))
  alpha = G.ALPHAS[(G.KS.index(K) + G.CLASSES.index(cls)) % 4]
  c0 = torch.randn(M, N, generator=torch.Generator().manual_seed(K))
  R = G.reference(A, B, alpha)
  Rc = G.reference(A, B, alpha, c0=c0)
  G.check(G.metrics(nt_whole(A, B, alpha, BF16), R, TILE), f'standin nt bf16 {cls} K={K} alpha={alpha}')
  G.check(G.metrics(nt_whole(A, B, alpha, torch.float32, c0=c0), Rc, TILE), f'standin nt fp32 accumulate {cls} K={K}')
  if K % 64 == 0 and K >= 768:
    G.check(G.metrics(nt_hybrid(A, B, alpha, L=max(2, K // 64 // 5)), R, TILE), f'standin hybrid {cls} K={K}')
    for splits, rows0 in ((4, 0), (8, 256 if M > 256 else 0)):   # also the grouped launch's split remainder, per problem
      G.check(G.metrics(tn_split(A, B, alpha, splits, c0=c0, rows0=rows0), Rc, TILE), f'standin tn split {splits} {cls} K={K}')
  G.check(G.metrics(tn_split(A, B, alpha, 1), R, TILE), f'standin tn whole-K {cls} K={K}')


def test_reference_failure_is_not_a_kernel_failure(monkeypatch):
  """A device reference that disagrees with the host's rows raises ReferenceFailure, not an assertion about the kernel."""
  A, B = case('randn', 256, 128, 128, 3)
  real = G._products
  calls = []

  def skewed(A_, B_, tn, rows):
    r, s = real(A_, B_, tn, rows)
    calls.append(1)
    return (r * (1 + 1e-10), s) if len(calls) == 1 else (r, s)   # the full-tensor product, not the host's rows

  monkeypatch.setattr(G, '_products', skewed)
  with pytest.raises(G.ReferenceFailure):
    G.reference(A, B)


# ---------------------------------------------------------------------------------------------------------------------
# the budget rejects every defect by 2x; the older yardsticks pass at least half of them
# ---------------------------------------------------------------------------------------------------------------------
def _old_passes(got, A, B, alpha, c0=None):
  K = A.shape[1]
  ref = a32(alpha) * (A.float() @ B.float().t())
  if c0 is not None:
    ref = c0 + ref
  tol = 6e-3 if got.dtype == BF16 else 2e-5 * math.sqrt(K)
  return relmax(got.float(), ref) <= tol


def _defects():
  """(name, metric meant to catch it, got, R, passes the older yardstick) for every planted defect."""
  out = []
  c0 = torch.randn(512, 512, generator=torch.Generator().manual_seed(9))
  # one k-term dropped in a 16-column block: fp32 C at every class incl. the longest K, bf16 C where a term is above an ulp
  for cls, M, K in (('pos', 512, 4096), ('randn', 512, 768), ('wide', 512, 768), ('pos', 256, 50304), ('randn', 256, 50304)):
    A, B = case(cls, M, M, K, 17)
    got = nt_whole(A, B, None, torch.float32, 'drop_term')
    out.append((f'drop_term fp32 {cls} K={K}', 'cond', got, G.reference(A, B), _old_passes(got, A, B, None)))
  A, B = case('randn', 512, 512, 4096, 18)
  R = G.reference(A, B, 0.3)
  got = nt_whole(A, B, 0.3, BF16, 'drop_term')
  out.append(('drop_term bf16 randn K=4096', 'ulp', got, R, _old_passes(got, A, B, 0.3)))
  for cls in ('randn', 'pos'):
    A, B = case(cls, 512, 512, 4096, 19)
    R = G.reference(A, B, 0.3)
    for defect, metric in (('skip_last_ktile', 'ulp'), ('tile_scale', 'proj'), ('truncate', 'bias'), ('truncate', 'neq'),
                           ('double_round', 'neq'), ('tail_row_copy', 'ulp')):
      got = nt_whole(A, B, 0.3, BF16, defect)
      out.append((f'{defect} bf16 {cls}', metric, got, R, _old_passes(got, A, B, 0.3)))
    for defect, metric in (('alpha_twice', 'ulp'), ('alpha_missing', 'ulp'), ('bf16_partials', 'neq')):
      got = nt_hybrid(A, B, 0.3, L=13, defect=defect)
      out.append((f'{defect} hybrid {cls}', metric, got, R, _old_passes(got, A, B, 0.3)))
    Rc = G.reference(A, B, 0.3, c0=c0)
    got = tn_split(A, B, 0.3, 8, c0=c0, defect='slab_scale')
    out.append((f'slab_scale tn {cls}', 'proj32', got, Rc, _old_passes(got, A, B, 0.3, c0)))
    got = tn_split(A, B, 0.3, 8, c0=c0, defect='accumulate_ignored', rows0=256)
    out.append((f'accumulate_ignored tn {cls}', 'cond', got, Rc, _old_passes(got, A, B, 0.3, c0)))
    got = nt_whole(A, B, 0.3, torch.float32, 'tile_scale', c0=c0)
    out.append((f'tile_scale fp32 {cls}', 'proj32', got, Rc, _old_passes(got, A, B, 0.3, c0)))
    got = nt_whole(A, B, 0.3, torch.float32, 'tail_row_copy', c0=c0)
    out.append((f'tail_row_copy fp32 {cls}', 'cond', got, Rc, _old_passes(got, A, B, 0.3, c0)))
  return out


@pytest.fixture(scope='module')
def defects():
  return _defects()


def test_budget_rejects_every_defect_by_2x(defects):
  weak = []
  for name, metric, got, R, _ in defects:
    v = G.metrics(got, R, TILE)[metric]
    print(f'defect {name}: {metric}={v:.3e} (bound {G.BOUNDS[metric]:.1e})')
    if not v >= 2 * G.BOUNDS[metric]:
      weak.append((name, metric, v))
  assert not weak, weak


def test_older_yardsticks_pass_at_least_half_of_the_defects(defects):
  kinds = {}
  for name, _, _, _, old in defects:
    k = name.split()[0]
    kinds[k] = kinds.get(k, False) or old     # a defect kind counts as passed when the older check passes it somewhere
  passed = sorted(k for k, v in kinds.items() if v)
  print('older yardsticks pass:', passed, 'of', sorted(kinds))
  assert len(kinds) == 11
  assert 2 * len(passed) >= len(kinds), passed
