"""Error budget of the bf16 GEMMs (NT, TN, grouped TN).  TEST INFRASTRUCTURE ONLY (same rules as cpu_ref.py).

The companion of oracle/parity.py (attention) and oracle/parity_ops.py (element-wise kernels) for csrc/gemm.hip and
csrc/gemm_big.hip.  max|got - ref| / max|ref| against 6e-3 (bf16 C) or 2e-5 sqrt(K) (fp32 C) passes a dropped k-term, a
truncating store, a second rounding around a non-power-of-two alpha and a tile or split-K slab scaled by 1 + 2^-9.  This
file measures a GEMM result the ways that separate those from honest rounding:

  * ``reference``: ref = alpha * A B^T (NT) or alpha * A^T B (TN) in fp64 from the bf16 operands and the fp32 alpha the
    kernel read, WITHOUT the final rounding, and next to it S = |alpha| |A| |B|^T, the sum of the magnitudes of the terms of
    each element: the scale on which accumulation error lives (a randn element cancels to ~ S / sqrt(K)).  With
    ``accumulate`` the old C0 is added to ref and |C0| to S.  The full tensors are fp64 matmuls on the operands' device, in
    row chunks; the first and last row of every 128-row band of M are recomputed on the host in fp64 and must agree to
    1e-12 S (fp64 round-off at K <= 2^16 is ~1e-14 S), else ``ReferenceFailure`` - a broken reference, not a kernel failure;
  * ``cond`` (fp32 C): max |got - ref| / S / (sqrt(K) EPS).  fp32 accumulation of K terms in any order stays below ~1; one
    dropped term is 1 / (K sqrt(K) EPS) times its size relative to the mean term;
  * ``ulp`` / ``neq`` / ``bias`` (bf16 C): parity_ops.elementwise with the absolute allowance
    ALLOW = BOUNDS['cond'] sqrt(K) EPS S, i.e. the fp32 state before the store may be as far off as a passing fp32 C.
    ``ulp`` is the largest distance beyond ALLOW in bf16 ulps of the reference.  ``neq`` (fraction not bit-equal to the
    correctly rounded reference) and ``bias`` (|mean of sign(ref) (got - ref)| in ulps: a truncating store gives ~0.5,
    round-to-nearest ~0) are counted ONLY on elements where ALLOW is below a quarter ulp: where a result cancels (or K is
    huge) the honest fp32 error is a sizeable part of an ulp, honest kernels flip such elements, and an allowance that
    excused them would excuse a second rounding as well.  At K = 50304 almost no randn element qualifies, so ``neq`` and
    ``bias`` are carried there by the all-positive class (|ref| = S, every element qualifies); ``bias`` needs at least
    BIAS_MIN qualifying elements;
  * ``proj`` (bf16 C) / ``proj32`` (fp32 C): the projection coefficient |<err, ref>| / <ref, ref> of parity.py over row
    bands, column bands and every output tile of the kernel's tile geometry - a tile, band or split-K slab scaled by a
    few 1e-4 moves it by that much, rounding noise of relative size s by ~ s / sqrt(n).  Every group has at least PROJ_MIN
    elements (adjacent rows / columns are banded until it has; smaller edge tiles are left to the element-wise metrics), and
    both inner products are taken after dividing rows and columns by their rms (u_i v_j, one balancing pass): with
    per-row power-of-two operand scales a plain inner product is three or four elements wide.

BOUNDS.  Each is at least 2x above the larger of the honest floor (the fp32 stand-ins of tests/test_parity_budget_gemm.py)
and the worst value the MI355X kernels show (tests/test_gemm_parity_gpu.py; per case in profiles/gemm_parity_budget.md),
and at least 2x below the smallest value a planted defect of tests/test_parity_budget_gemm.py gives on the metric meant to
catch it.
"""

from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import torch

from .parity_ops import EPS, FLOOR, _exp2i, bf16_rne, elementwise, merge, ulp_of  # noqa: F401  (re-exported for the tests)

Tensor = torch.Tensor
F64 = torch.float64
BF16 = torch.bfloat16
PROJ_MIN = 4096   # elements per projection group (rounding noise 2^-9 / sqrt(4096) * 4.5 sigma ~ 1.5e-4)
BIAS_MIN = 4096   # qualifying elements ``bias`` needs (0.29 ulp / sqrt(4096) * 4.5 sigma = 0.02)
HOST_TOL = 1e-12  # device fp64 reference vs host fp64, in units of S

# worst measured: honest fp32 stand-ins (CPU) | MI355X kernels | smallest planted defect   (per case: profiles/gemm_parity_budget.md)
BOUNDS = {
    'cond': 2.0,      # 0.71 (pos, K = 72: the output roundings) | 0.52 (NT v0, pos, K = 72) | 13.5 (one k-term dropped, K = 50304)
    'ulp': 1.0,       # 0.50 | 0.50 | 5.6 (last K-tile of a tile skipped, pos K = 4096)
    'neq': 2e-2,      # 1.7e-4 | 2.3e-4 | 6.8e-2 (stream-K partials in bf16, pos); 0.25 double rounding; 0.50 truncation
    'bias': 0.1,      # 4.1e-3 | 1.7e-3 | 0.50 (truncating store)
    'proj': 6e-4,     # 1.95e-4 (wide, K = 64) | 1.86e-4 | 1.95e-3 (a tile scaled by 1 + 2^-9)
    'proj32': 3e-5,   # 2.8e-8 | 3.5e-7 | 2.5e-4 (one of 8 split-K slabs scaled by 1 + 2^-9)
}

NT_TILES = {0: ((256, 256), (256, 192), (256, 128), (128, 192), (128, 128)), 1: ((128, 128),), 2: ((128, 128),),
            3: ((256, 256),), 4: ((256, 256),), 5: ((256, 192),), 6: ((256, 128),), 7: ((128, 192),)}
TN_TILES = ((256, 256), (128, 128))


class ReferenceFailure(RuntimeError):
  """The device fp64 reference disagrees with the host's on the sampled rows: the case proves nothing about the kernel."""


# --------------------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------------------
def band_rows(M: int) -> Tensor:
  """First and last row of every 128-row band of M."""
  first = torch.arange(0, M, 128)
  return torch.unique(torch.cat([first, (first + 127).clamp_max(M - 1)]))


def _products(A: Tensor, B: Tensor, tn: bool, rows) -> Tuple[Tensor, Tensor]:
  """(A B^T, |A| |B|^T) (NT) or (A^T B, |A|^T |B|) (TN) in fp64 for the output rows ``rows`` (a slice or an index tensor)."""
  Bd = B.double()
  Ad = (A[:, rows].double().t() if tn else A[rows].double())
  Bm = Bd if tn else Bd.t()
  return Ad @ Bm, Ad.abs() @ Bm.abs()


def reference(A: Tensor, B: Tensor, alpha=None, tn: bool = False, c0: Optional[Tensor] = None, chunk: int = 4096) -> Dict:
  """{'ref', 'S' fp64 [M, N] on A's device, 'K'} for the bf16 operands A [M, K], B [N, K] (NT) or A [K, M], B [K, N] (TN),
  alpha None, a float or the fp32 tensor the kernel read, c0 the fp32 C before an accumulating call.  Cross-checked against
  the host (see the module docstring)."""
  a = 1.0 if alpha is None else float(alpha.double().item() if isinstance(alpha, Tensor) else torch.tensor(alpha, dtype=torch.float32).double().item())
  M = A.shape[1] if tn else A.shape[0]
  K = A.shape[0] if tn else A.shape[1]
  N = B.shape[1] if tn else B.shape[0]
  ref = torch.empty((M, N), dtype=F64, device=A.device)
  S = torch.empty_like(ref)
  for i0 in range(0, M, chunk):
    sl = slice(i0, min(i0 + chunk, M))
    ref[sl], S[sl] = _products(A, B, tn, sl)
  ref *= a
  S *= abs(a)
  rows = band_rows(M)
  Ah = (A[:, rows.to(A.device)] if tn else A[rows.to(A.device)]).cpu()
  href, hS = _products(Ah, B.cpu(), tn, slice(None))
  href, hS = href * a, hS * abs(a)
  dev = rows.to(A.device)
  bad = ((ref[dev].cpu() - href).abs() > HOST_TOL * hS + FLOOR) | ((S[dev].cpu() - hS).abs() > HOST_TOL * hS + FLOOR)
  if bad.any():
    raise ReferenceFailure(f'device fp64 reference differs from the host on {int(bad.sum())} of {bad.numel()} sampled elements '
                           f'(M={M} N={N} K={K} tn={tn})')
  if c0 is not None:
    ref += c0.double()
    S += c0.double().abs()
  return {'ref': ref, 'S': S, 'K': K}


# --------------------------------------------------------------------------------------
# metrics
# --------------------------------------------------------------------------------------
def _err(got: Tensor, ref: Tensor) -> Tensor:
  g = got.detach().to(ref.device).double()
  return torch.where(torch.isfinite(g), (g - ref).abs(), torch.full_like(g, float('inf')))


def cond(got: Tensor, R: Dict) -> Dict[str, float]:
  e = (_err(got, R['ref']) - FLOOR).clamp_min(0.0) / R['S'].clamp_min(FLOOR)
  return {'cond': e.max().item() / (math.sqrt(R['K']) * EPS)}


def allowance(R: Dict) -> Tensor:
  return BOUNDS['cond'] * math.sqrt(R['K']) * EPS * R['S']


def rounding(got: Tensor, R: Dict) -> Dict[str, float]:
  """{'ulp', 'neq', 'bias'} of a bf16 C (module docstring)."""
  ref, allow = R['ref'], allowance(R)
  m = {'ulp': elementwise(got, ref, allow)['ulp'], 'neq': 0.0, 'bias': 0.0}
  u = ulp_of(ref)
  q = allow < 0.25 * u
  if q.any():
    g, r = got.detach().to(ref.device)[q], ref[q]
    m['neq'] = elementwise(g, r, allow[q])['neq']
    if r.numel() >= BIAS_MIN:
      m['bias'] = abs((torch.sign(r) * (g.double() - r) / u[q]).mean().item())
  return m


def _groups(num: Tensor, den: Tensor, per: int) -> Tensor:
  """|sum num| / sum den over bands of adjacent entries holding at least PROJ_MIN elements (``per`` elements per entry)."""
  n = num.numel()
  g = -(-PROJ_MIN // per)
  ng = n // g
  if ng == 0:
    return num.new_zeros(1)
  gid = (torch.arange(n, device=num.device) // g).clamp_max(ng - 1)
  gn = torch.zeros(ng, dtype=F64, device=num.device).index_add_(0, gid, num)
  gd = torch.zeros(ng, dtype=F64, device=num.device).index_add_(0, gid, den)
  return torch.where(gd > 0, gn.abs() / gd.clamp_min(1e-300), torch.where(gn == 0, gn, gn.abs() * float('inf')))


def projection(got: Tensor, R: Dict, tiles: Sequence[Tuple[int, int]]) -> float:
  ref = R['ref']
  M, N = ref.shape
  err = got.detach().to(ref.device).double() - ref
  u = ref.pow(2).mean(1).sqrt()
  u = torch.where(u > 0, u, torch.ones_like(u))
  v = (ref / u[:, None]).pow(2).mean(0).sqrt()
  v = torch.where(v > 0, v, torch.ones_like(v))
  rn = ref / u[:, None] / v[None, :]
  p = err / u[:, None] / v[None, :] * rn
  q = rn * rn
  worst = [_groups(p.sum(1), q.sum(1), N).max(), _groups(p.sum(0), q.sum(0), M).max()]
  for bm, bn in tiles:
    tm, tn = -(-M // bm), -(-N // bn)
    pad = (0, tn * bn - N, 0, tm * bm - M)
    tp = torch.nn.functional.pad(p, pad).reshape(tm, bm, tn, bn).sum((1, 3))
    tq = torch.nn.functional.pad(q, pad).reshape(tm, bm, tn, bn).sum((1, 3))
    rows = (M - torch.arange(tm, device=ref.device) * bm).clamp_max(bm)
    cols = (N - torch.arange(tn, device=ref.device) * bn).clamp_max(bn)
    big = (rows[:, None] * cols[None, :] >= PROJ_MIN) & ((tq > 0) | (tp != 0))
    if big.any():
      worst.append((tp[big].abs() / tq[big]).max())
  w = torch.stack(worst)
  return float('nan') if torch.isnan(w).any() else w.max().item()


def metrics(got: Tensor, R: Dict, tiles: Sequence[Tuple[int, int]]) -> Dict[str, float]:
  """Every metric of one result: bf16 C -> ulp, neq, bias, proj; fp32 C -> cond, proj32."""
  if got.dtype == BF16:
    return merge(rounding(got, R), {'proj': projection(got, R, tiles)})
  return merge(cond(got, R), {'proj32': projection(got, R, tiles)})


def violations(m: Dict[str, float]) -> Dict[str, tuple]:
  return {k: (v, BOUNDS[k]) for k, v in m.items() if not v <= BOUNDS[k]}


def check(m: Dict[str, float], tag: str) -> Dict[str, float]:
  """Assert every metric within BOUNDS; prints them (one line, 'parity_gemm <tag>: ...') either way."""
  print(f'parity_gemm {tag}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  bad = violations(m)
  assert not bad, f'{tag}: ' + ', '.join(f'{k} {v:.3e} > {b:.1e}' for k, (v, b) in bad.items())
  return m


# --------------------------------------------------------------------------------------
# inputs shared by the GPU tests and the CPU calibration
# --------------------------------------------------------------------------------------
CLASSES = ('randn', 'wide', 'pos', 'blocky')
ALPHAS = (None, 0.3, -1.0 / 3.0, 1.0 / 98304)   # None, two values that are no power of two, a grad scale
KS = (64, 72, 200, 768, 1024, 2048, 4096, 4104, 16384, 32768, 50304)   # every contraction length of the GPU file


def operand(cls: str, rows: int, K: int, seed: int, device='cpu') -> Tensor:
  """bf16 [rows, K] of one input class: 'randn'; 'wide' = randn with a power-of-two scale 2^-12 .. 2^12 per row; 'pos' =
  |randn| (no cancellation: accumulation precision shows); 'blocky' = randn with whole 64-wide K tiles zeroed in a quarter
  of the rows."""
  g = torch.Generator(device=device).manual_seed(seed)
  x = torch.randn(rows, K, generator=g, device=device)
  if cls == 'wide':
    x = x * _exp2i(torch.randint(-12, 13, (rows, 1), generator=g, device=device)).float()   # exact powers of two on any device
  elif cls == 'pos':
    x = x.abs()
  elif cls == 'blocky':
    kt = -(-K // 64)
    dead = (torch.rand(rows, kt, generator=g, device=device) < 0.5) & (torch.rand(rows, 1, generator=g, device=device) < 0.25)
    x = x.masked_fill(dead.repeat_interleave(64, 1)[:, :K], 0.0)
  elif cls != 'randn':
    raise ValueError(cls)
  return x.to(BF16)
