"""Error budget and exact-input helpers for the kernels that end a training step.  TEST INFRASTRUCTURE ONLY (same rules as
cpu_ref.py and parity_ops.py).

The companion of parity_ops.py for optim.hip (AdamW, NAdamW, SGD, signSGD, schedule-free AdamW), the small reductions
(sum of squares, mean, column sums) and the embedding.  One number, max|got - ref| / max|ref| over a unit-normal tensor, sees
only the largest elements: ``eps`` moved inside the division by sqrt(bc2) reads 4.8e-7 there.  This file measures the
optimizers element by element, and gives the reductions inputs on which no tolerance is needed at all:

  * ``optim_reference``: p', m', v' in fp64 from the fp32 operands and the fp32 fields of the plm_optim_hparams struct,
    AdamW's three prepared scalars formed as optim_prepared() forms them (each rounded once to fp32); and, per output, the
    MAGNITUDE its error is measured against.  The magnitude is cancellation-free: wherever a formula adds terms of either
    sign it adds their absolute values, all the way down (m' inside p' enters as |beta1 m| + |(1 - beta1) g|, never as
    |m'|: with |m'| an honest AdamW reads 255 roundoffs on wide-range data, because m' itself cancelled);
  * ``optim_metrics``: {'p', 'm', 'v'} = max over elements of |got - ref| / (2^-24 * magnitude), i.e. the error in fp32
    roundoffs of the size of the terms that were added.  Errors below parity_ops.FLOOR are ignored, a non-finite result
    against a finite reference counts as infinite;
  * signSGD: where |m'_ref| <= BOUNDS_TAIL[signSGD, m] * 2^-24 * magnitude_m the sign of m' is not determined by the
    operands (an honest m' may land on either side of 0, or on 0).  There p' must be within the p bound of one of
    p decay - lr {-1, 0, +1}; such elements are reported as the share 'excl', capped at EXCL_MAX per case (a condition,
    not a measurement).  An m' whose magnitude is 0 (g = m = 0) is exactly 0 in any arithmetic: its sign is determined;
  * ``exact_sum_inputs`` / ``onehot_indices``: inputs on which every partial sum of a reduction is exact in fp32 (integers, or
    multiples of 2^-2, below 2^24 ulps), so that the result is the same for any order, tree or FMA contraction and is
    compared with ==;
  * ``embed_bwd_sequential``: the one summation order plm_embed_bwd_sorted's contract names (increasing token order, fp32).

BOUNDS_TAIL follows the rule at the top of parity_ops.py: each bound is at least 2x the larger of the fp32 stand-in's worst
value (tests/test_parity_budget_tail.py) and the MI355X's worst value over every input class, and at most half of the
smallest value a planted defect produces on the metric meant to catch it (profiles/tail_parity.md has every figure).
Beside each bound stands the number of fp32 roundings on the longest chain to that output in optim_elem - a first-order
ceiling of the metric (each rounding moves the result by at most one roundoff of a term no larger than the magnitude).
The measured worst values (stand-in 3.8, MI355X 4.4 at most) stay below every count but v's, whose chain squares the
rounded gi (its error enters twice); no bound is above twice its count, so none needs a reason for exceeding 4x.
"""

from __future__ import annotations

from fractions import Fraction
from typing import Dict, Optional

import numpy as np
import torch

from .parity_ops import EPS, FLOOR

Tensor = torch.Tensor
F64 = torch.float64
F32 = torch.float32

KINDS = ('adamw', 'nadamw', 'sgd', 'sgd0', 'signSGD', 'sfo_adamw')   # sgd0: SGD with momentum == 0 (no buffer)
CLASSES = ('randn', 'mixed', 'tiny_g', 'zero_g0', 'zero_g', 'large_g')
EXCL_MAX = 1e-3     # signSGD: largest share of elements whose sign may be undetermined (test_flat_kernel_matches_torch_optimizer's figure)

# (kind, output): bound in fp32 roundoffs of the magnitude.   roundings on the longest chain (optim_elem, optim.hip):
BOUNDS_TAIL = {
    ('adamw', 'p'): 10.0,      # 11: gi, (1-b1) gi, mi | (1-b2) gi, * gi, vi, sqrt, / bc2, + eps | mi / d, p decay, final fma (+ decay, coef_avg, bc2 themselves)
    ('adamw', 'm'): 5.0,       # 3: gi, (1-b1) gi, the fma
    ('adamw', 'v'): 8.0,       # 5: gi (twice: squared), (1-b2) gi, * gi, the fma
    ('nadamw', 'p'): 10.0,     # 12: as AdamW's with vi / bc2 before the sqrt, and gi / d and its fma in addition
    ('nadamw', 'm'): 5.0,      # 3
    ('nadamw', 'v'): 8.0,      # 5
    ('sgd', 'p'): 7.0,         # 5: gi, d, mom m, mi, the final fma
    ('sgd', 'm'): 6.0,         # 4: gi, d, mom m, the fma
    ('sgd0', 'p'): 5.0,        # 3: gi, d, the final fma
    ('signSGD', 'p'): 4.0,     # 2: p decay, the final fma (the sign is exact or excluded)
    ('signSGD', 'm'): 5.0,     # 3: gi, mom m0, the fma (+ 1 - dampening)
    ('sfo_adamw', 'p'): 10.0,  # 11: gi ... d (7), gi / d, gn, the lerp (2), the final fma
    ('sfo_adamw', 'm'): 10.0,  # 10: gi ... d (7), gi / d, gn, the fma
    ('sfo_adamw', 'v'): 8.0,   # 5
}


# ---------------------------------------------------------------------------------------------------------------------
# scalars
# ---------------------------------------------------------------------------------------------------------------------
def fl32(x) -> float:
  """The fp32 nearest (ties to even) to the exact rational x, rounded ONCE, as a Python float (normal range only)."""
  x = Fraction(x)
  if x == 0:
    return 0.0
  a = abs(x)
  e = a.numerator.bit_length() - a.denominator.bit_length()
  if Fraction(2) ** e > a:
    e -= 1
  assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e < 128
  n = round(a / Fraction(2) ** (e - 23))          # Python rounds a Fraction half to even
  r = float(n) * 2.0 ** (e - 23)
  return r if x > 0 else -r


def hparams_dict(hp) -> Dict[str, float]:
  """The fields of a plm_optim_hparams struct (ops.optim_hparams) as Python numbers: the fp32 values the kernels read."""
  return {name: getattr(hp, name) for name, _ in hp._fields_}


def prepared(h: Dict[str, float]) -> Dict[str, float]:
  """optim_prepared() of optim.hip for AdamW, each scalar rounded once from the fp32 fields: decay = fl32(1 - lr wd),
  coef_avg = fl32(lr / bc1), bc2 = fl32(sqrt(bc2)).  The other kinds take the struct as it is."""
  k = dict(h)
  if h['kind_name'] == 'adamw':
    k['decay'] = fl32(1 - Fraction(h['lr']) * Fraction(h['weight_decay']))
    k['coef_avg'] = fl32(Fraction(h['lr']) / Fraction(h['bc1']))
    k['bc2'] = float(np.sqrt(np.float32(h['bc2'])))   # IEEE sqrt of an fp32: correctly rounded
  return k


_KIND_IDS = {5: 'adamw', 1: 'nadamw', 2: 'sgd', 3: 'signSGD', 4: 'sfo_adamw'}   # PLM_OPTIM_* (include/plainlm_hip.h)


def fields(hp) -> Dict[str, float]:
  h = hparams_dict(hp)
  h['kind_name'] = _KIND_IDS[h['kind']]
  return prepared(h)


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------
def optim_reference(kind: str, hp, p: Tensor, g: Tensor, m: Optional[Tensor], v: Optional[Tensor], clip: Optional[float]) -> Dict:
  """One step of ``kind`` ('sgd0' = 'sgd' with hp.momentum == 0) in fp64 from the fp32 operands (before the in-place
  kernel) and the struct ``hp``; ``clip`` is the fp32 clip coefficient or None.  Returns {'p': (ref, mag), 'm': (ref, mag)
  or None, 'v': (ref, mag) or None, 'kind', and for signSGD 'pd' (p decay) and 'lr'}.  On a first step (hp.first) of SGD /
  signSGD / sfo_adamw the buffers the step creates are not read (pass anything)."""
  h = fields(hp)
  assert h['kind_name'] == ('sgd' if kind == 'sgd0' else kind), (kind, h['kind_name'])
  assert (kind == 'sgd0') == (h['kind_name'] == 'sgd' and h['momentum'] == 0.0)
  first = bool(h['first'])
  d64 = lambda t: t.detach().cpu().to(F64)  # noqa: E731
  p, g = d64(p), d64(g)
  cs = 1.0 if clip is None else float(np.float32(clip))
  gi = g * cs
  out = {'kind': kind, 'm': None, 'v': None}
  b1, b2, eps, lr, wd = h['beta1'], h['beta2'], h['eps'], h['lr'], h['weight_decay']
  if kind in ('adamw', 'nadamw'):
    m, v = d64(m), d64(v)
    mi = b1 * m + (1 - b1) * gi
    mag_m = (b1 * m).abs() + ((1 - b1) * gi).abs()
    vi = b2 * v + (1 - b2) * gi * gi
    out['m'], out['v'] = (mi, mag_m), (vi, (b2 * v).abs() + (1 - b2) * gi * gi)
    pd = p * h['decay']
    if kind == 'adamw':
      d = vi.sqrt() / h['bc2'] + eps
      out['p'] = (pd - h['coef_avg'] * mi / d, pd.abs() + abs(h['coef_avg']) * mag_m / d)
    else:
      d = (vi / h['bc2']).sqrt() + eps
      out['p'] = (pd - h['coef_grad'] * gi / d - h['coef_avg'] * mi / d,
                  pd.abs() + abs(h['coef_grad']) * gi.abs() / d + abs(h['coef_avg']) * mag_m / d)
  elif kind in ('sgd', 'sgd0'):
    d = wd * p + gi
    mag_d = (wd * p).abs() + gi.abs()
    if kind == 'sgd0':
      out['p'] = (p - lr * d, p.abs() + abs(lr) * mag_d)
    else:
      if first:
        mi, mag_m = d, mag_d
      else:
        m = d64(m)
        mi = (1 - h['dampening']) * d + h['momentum'] * m
        mag_m = abs(1 - h['dampening']) * mag_d + (h['momentum'] * m).abs()
      out['m'] = (mi, mag_m)
      out['p'] = (p - lr * mi, p.abs() + abs(lr) * mag_m)
  elif kind == 'sfo_adamw':
    z = p if first else d64(m)
    v0 = torch.zeros_like(p) if first else d64(v)
    vi = b2 * v0 + (1 - b2) * gi * gi
    out['v'] = (vi, (b2 * v0).abs() + (1 - b2) * gi * gi)
    d = (vi / h['bc2']).sqrt() + eps
    gn = wd * p + gi / d
    mag_gn = (wd * p).abs() + gi.abs() / d
    out['m'] = (z - lr * gn, z.abs() + abs(lr) * mag_gn)
    w = h['ckp1']
    # either form of the two-sided lerp subtracts p and z before it scales: its round-off is relative to |p| + |z| (0 <= w <= 1)
    out['p'] = ((1 - w) * p + w * z + h['coef_y'] * gn, p.abs() + z.abs() + abs(h['coef_y']) * mag_gn)
  else:
    assert kind == 'signSGD'
    pd = p * h['decay']
    m0 = gi if first else d64(m)
    mi = (1 - h['dampening']) * gi + h['momentum'] * m0
    out['m'] = (mi, ((1 - h['dampening']) * gi).abs() + (h['momentum'] * m0).abs())
    out['p'] = (pd - lr * torch.sign(mi), pd.abs() + abs(lr))
    out['pd'], out['lr'] = pd, lr
  return out


def _roundoffs(got: Tensor, ref: Tensor, mag: Tensor) -> Tensor:
  """|got - ref| beyond FLOOR in units of 2^-24 * mag, element by element; inf where got is not finite (the references are)."""
  g = got.detach().cpu().to(F64).reshape(ref.shape)
  err = torch.where(torch.isfinite(g), (g - ref).abs(), torch.full_like(g, float('inf')))
  return (err - FLOOR).clamp_min(0.0) / (EPS * mag).clamp_min(FLOOR)


def optim_metrics(ref: Dict, got_p: Tensor, got_m: Optional[Tensor] = None, got_v: Optional[Tensor] = None) -> Dict[str, float]:
  """{'p', 'm', 'v'} (the outputs the kind has) of a result against ``optim_reference``'s dict; signSGD adds 'excl', the
  share of elements whose sign the operands do not determine (see the top of the file)."""
  kind = ref['kind']
  out = {}
  if ref['m'] is not None:
    out['m'] = _roundoffs(got_m, *ref['m']).max().item()
  if ref['v'] is not None:
    out['v'] = _roundoffs(got_v, *ref['v']).max().item()
  rp = _roundoffs(got_p, *ref['p'])
  if kind == 'signSGD':
    mi, mag_m = ref['m']
    undet = (mi.abs() <= BOUNDS_TAIL[('signSGD', 'm')] * EPS * mag_m) & (mag_m > 0)
    mag_p = ref['p'][1]
    alt = torch.stack([_roundoffs(got_p, ref['pd'] - ref['lr'] * s, mag_p) for s in (-1.0, 0.0, 1.0)]).amin(0)
    rp = torch.where(undet, alt, rp)
    out['excl'] = undet.double().mean().item()
  out['p'] = rp.max().item()
  return out


def bound_of(kind: str, key: str) -> float:
  return EXCL_MAX if key == 'excl' else BOUNDS_TAIL[(kind, key)]


def violations(kind: str, m: Dict[str, float]) -> Dict[str, tuple]:
  """{metric: (value, bound)} for every metric above its bound (NaN counts as above)."""
  return {k: (x, bound_of(kind, k)) for k, x in m.items() if not x <= bound_of(kind, k)}


def check(kind: str, m: Dict[str, float], tag: str) -> Dict[str, float]:
  """Assert every metric within BOUNDS_TAIL; prints them (one line, 'parity_tail <tag>: ...') either way."""
  print(f'parity_tail {tag}: ' + ' '.join(f'{k}={x:.3g}' for k, x in m.items()))
  bad = violations(kind, m)
  assert not bad, f'{tag}: ' + ', '.join(f'{k} {x:.3e} > {b:.1e}' for k, (x, b) in bad.items())
  return m


# ---------------------------------------------------------------------------------------------------------------------
# inputs and hyper-parameters shared by the GPU test and the CPU calibration
# ---------------------------------------------------------------------------------------------------------------------
HP = dict(lr=1e-2, wd=0.1, b1=0.9, b2=0.95, eps=1e-8, damp=0.1)
CLIP = 0.37


def tail_hparams(kind: str, first: bool, eps: Optional[float] = None, wd: Optional[float] = None):
  """The struct for one step of ``kind``: the first step (AdamW / NAdamW: step 1, run on m = v = 0) or a steady one (step 3;
  sfo_adamw: step 2, where ckp1 = 0.8 takes the far-side branch of the lerp - its first step has ckp1 = 1, and the near side is
  lerp_'s own test)."""
  from plainlm_amd import ops
  eps = HP['eps'] if eps is None else eps
  wd = HP['wd'] if wd is None else wd
  step = 1 if first else (2 if kind == 'sfo_adamw' else 3)
  lr, b1, b2 = HP['lr'], HP['b1'], HP['b2']
  if kind == 'adamw':
    return ops.optim_hparams('adamw', lr, wd, beta1=b1, beta2=b2, eps=eps, bc1=1.0 - b1 ** step, bc2=1.0 - b2 ** step)
  if kind == 'nadamw':
    mu_product = 1.0
    for s in range(1, step + 1):
      bc2, cg, cm, mu_product = ops.nadam_scalars(lr, b1, b2, 4e-3, s, mu_product)
    return ops.optim_hparams('nadamw', lr, wd, beta1=b1, beta2=b2, eps=eps, bc2=bc2, coef_grad=cg, coef_avg=cm)
  if kind == 'sfo_adamw':
    grp = dict(lr=lr, betas=(b1, b2), k=0, warmup_steps=2, r=0.0, weight_lr_power=2.0, lr_max=-1.0, weight_sum=0.0)
    for _ in range(step):
      lr_s, ckp1, bc2 = ops.sfo_scalars(grp)
    return ops.optim_hparams('sfo_adamw', lr_s, wd, first=first, beta1=b1, beta2=b2, eps=eps, bc2=bc2, ckp1=ckp1)
  return ops.optim_hparams('sgd' if kind == 'sgd0' else kind, lr, wd, first=first, momentum=0.0 if kind == 'sgd0' else b1, dampening=HP['damp'])


def _logu(gen, n, lo, hi, signed=True):
  """n fp32 values, magnitudes log-uniform on [lo, hi], random signs."""
  mag = torch.exp(torch.rand(n, generator=gen, dtype=F64) * (np.log(hi) - np.log(lo)) + np.log(lo))
  if signed:
    mag = mag * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
  return mag.float()


def optim_inputs(cls: str, n: int, seed: int):
  """fp32 (p, g, m, v) of one input class (v >= 0; no fp32 denormals anywhere, nor in the products optim_elem forms):
  randn     unit-normal p, g; m = 0.1 randn, v = 0.01 rand (the older tests' data);
  mixed     magnitudes log-uniform over decades, random signs: p 1e-8..1e4, g and m 1e-10..1e2, v 1e-20..1e4;
  tiny_g    g, m ~ 1e-9, v ~ 1e-18: sqrt(v) is comparable to eps = 1e-8;
  zero_g0   g = 0 on m = v = 0;      zero_g   g = 0 on m, v != 0;
  large_g   |g|, |m| ~ 1e15, v ~ 1e30 (g^2 stays finite)."""
  gen = torch.Generator().manual_seed(seed)
  rn = lambda: torch.randn(n, generator=gen)  # noqa: E731
  nz = lambda t: torch.where(t.abs() < 1e-3, torch.full_like(t, 1e-3), t)  # noqa: E731  (keeps scaled values off the denormals)
  p = rn()
  if cls == 'randn':
    g, m, v = rn(), 0.1 * rn(), 0.01 * torch.rand(n, generator=gen)
  elif cls == 'mixed':
    p, g, m, v = _logu(gen, n, 1e-8, 1e4), _logu(gen, n, 1e-10, 1e2), _logu(gen, n, 1e-10, 1e2), _logu(gen, n, 1e-20, 1e4, signed=False)
  elif cls == 'tiny_g':
    g, m, v = 1e-9 * nz(rn()), 1e-9 * nz(rn()), 1e-18 * (0.01 + torch.rand(n, generator=gen))
  elif cls == 'zero_g0':
    g, m, v = torch.zeros(n), torch.zeros(n), torch.zeros(n)
  elif cls == 'zero_g':
    g, m, v = torch.zeros(n), 0.1 * nz(rn()), 0.01 * (0.01 + torch.rand(n, generator=gen))
  elif cls == 'large_g':
    g, m, v = 1e15 * nz(rn()), 1e15 * nz(rn()), 1e30 * (0.01 + torch.rand(n, generator=gen))
  else:
    raise ValueError(cls)
  tiny = torch.finfo(F32).tiny
  for t in (p, g, m, v):
    assert t.dtype == F32 and bool(((t == 0) | (t.abs() >= tiny)).all())
  return p, g, m, v


# ---------------------------------------------------------------------------------------------------------------------
# reductions: inputs whose every partial sum is exact in fp32
# ---------------------------------------------------------------------------------------------------------------------
def exact_sum_inputs(shape, seed: int, values) -> Tensor:
  """fp32 tensor of ``shape`` drawn uniformly from ``values`` (small integers or multiples of 0.5).  The caller keeps
  numel * max(v^2) (sum of squares) or numel * max|v| (plain sums) below 2^24 quanta: every partial sum, in any order and
  through any FMA, is then exact and the result must EQUAL the int64 / fp64 sum."""
  gen = torch.Generator().manual_seed(seed)
  vals = torch.tensor(list(values), dtype=F32)
  return vals[torch.randint(0, len(vals), tuple(shape) if not isinstance(shape, int) else (shape,), generator=gen)]


def onehot_indices(n: int):
  """The positions of the one-hot probes of a length-n sum of squares: both ends, the float4 / tail boundary, and the
  1024-thread x float4 block boundaries."""
  idx = {0, 3, 4, n - 1, 4 * (n // 4) - 1, 4 * (n // 4)}
  for k in (1, 2, 1023, 1024, 2047, 2048):
    idx |= {4096 * k - 1, 4096 * k, 4096 * k + 1}
  return sorted(i for i in idx if 0 <= i < n)


def embed_bwd_sequential(ids: Tensor, dout: Tensor, dW0: Optional[Tensor], V: int) -> Tensor:
  """dW[V, d] fp32 = dW0 (zeros when None) plus the rows of dout [M, d] added ONE BY ONE IN TOKEN ORDER in fp32, ids outside
  [0, V) ignored: the order plm_embed_bwd_sorted promises.  numpy.add.at is unbuffered and walks the indices in order, bit-equal to the explicit loop
  (tests/test_parity_budget_tail.py checks it)."""
  ids_n = ids.detach().cpu().numpy().reshape(-1)
  do = dout.detach().cpu().numpy().astype(np.float32)
  dW = np.zeros((V, do.shape[1]), np.float32) if dW0 is None else dW0.detach().cpu().numpy().astype(np.float32).copy()
  ok = (ids_n >= 0) & (ids_n < V)
  np.add.at(dW, ids_n[ok], do[ok])
  return torch.from_numpy(dW)
