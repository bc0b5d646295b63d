"""References for the Muon tests (tests/test_muon_host.py, tests/test_muon_gpu.py).  TEST INFRASTRUCTURE ONLY.

  ns_fp64        Newton-Schulz from a given X0 in fp64 with no intermediate rounding: the reference R.
  ns_bf16        the same iteration rounding to bf16 at A, Bm and X (products summed in fp64, the epilogue's expression in fp32 as the
                 kernel spells it): what an implementation with exact sums would give; differs from any real one by summation order only.
  x0_of          bf16(U) normalized as torch.optim._muon does (wide orientation), from torch ops.
  scalar_chain   the exact class U = v P (P a 0/1 partial permutation): every product has one non-zero term, so the whole iteration is a
                 scalar recurrence of the stated epilogue; returns the value every non-zero of O must equal, bit for bit.
"""

import numpy as np
import torch

COEFFS = (3.4445, -4.7750, 2.0315)
EPS = 1e-7
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def x0_of(u, eps=EPS):
  """(X0 bf16 [m, n] wide, nrm): torch's own normalization of bf16(u), on the transpose of a tall u."""
  x = u.bfloat16()
  if x.size(0) > x.size(1):
    x = x.T
  nrm = x.norm().clamp(min=eps)
  return (x / nrm).contiguous(), nrm


def ns_fp64(x0, steps=5, coeffs=COEFFS):
  a, b, c = coeffs
  x = x0.double()
  for _ in range(steps):
    A = x @ x.T
    Bm = b * A + c * (A @ A)
    x = a * x + Bm @ x
  return x


def _fma32(alpha, acc, addend):
  """bf16(fmaf(alpha, acc, addend)) for an fp32 scalar alpha, acc and addend fp32 tensors: the product and the sum formed in fp64 (exact for
  fp32 factors up to the final sum, which is then rounded once to fp32 - double rounding is possible only on a tie of the fp64 sum)."""
  return (float(np.float32(alpha)) * acc.double() + addend.double()).float().bfloat16()


def ns_bf16(x0, steps=5, coeffs=COEFFS):
  """Rounds where the kernels round: A = bf16(X X^T); Bm = bf16(fma(c, A A, b * A)); X = bf16(fma(1, Bm X, a * X)); sums in fp64 -> fp32."""
  a, b, c = (float(np.float32(v)) for v in coeffs)
  x = x0.bfloat16()
  for _ in range(steps):
    xd = x.double()
    A = (xd @ xd.T).float().bfloat16()
    Ad = A.double()
    Bm = _fma32(c, (Ad @ Ad).float(), (A.float() * b).float())
    x = _fma32(1.0, (Bm.double() @ xd).float(), (x.float() * a).float())
  return x


def _bf16(v):
  return float(torch.tensor(v, dtype=F32).bfloat16().float())


def _f32(v):
  return float(np.float32(v))


def scalar_chain(value, m, steps=5, coeffs=COEFFS, eps=EPS):
  """The non-zero value of O for U = value * P with m non-zeros (one per row of the wide orientation).  Every step is exact up to the
  stated roundings: ub = bf16(value); nrm = max(bf16(sqrt(fp32 sum of m ub^2)), bf16(eps)) (the sum is exact: m ub^2 needs 16 + log2 m
  bits); x = bf16(ub / nrm); then per step A = bf16(x x), Bm = bf16(fma(c, A A, b A)), x = bf16(fma(1, Bm x, a x))."""
  a, b, c = (_f32(v) for v in coeffs)
  ub = _bf16(value)
  nrm = max(_bf16(_f32(np.sqrt(np.float32(_f32(m * ub * ub))))), _bf16(eps))
  x = _bf16(_f32(np.float32(ub) / np.float32(nrm)))
  for _ in range(steps):
    A = _bf16(_f32(x * x))                        # one term: the fp32 accumulator holds the exact product
    Bm = _bf16(_f32(c * (A * A) + _f32(b * A)))   # fmaf(c, acc, b * d): the product b * d rounded to fp32, the fma once
    x = _bf16(_f32(1.0 * (Bm * x) + _f32(a * x)))
  return x


def partial_permutation(rows, cols, seed):
  """0/1 matrix with min(rows, cols) ones, one per row and column of the wide orientation, fp32."""
  g = torch.Generator().manual_seed(seed)
  m, n = min(rows, cols), max(rows, cols)
  P = torch.zeros(m, n)
  P[torch.arange(m), torch.randperm(n, generator=g)[:m]] = 1.0
  return P if rows <= cols else P.T.contiguous()


def rel_fro(x, ref):
  return ((x.double() - ref.double()).norm() / ref.double().norm()).item()
