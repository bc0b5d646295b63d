"""Error budget of the step's non-attention kernels.  TEST INFRASTRUCTURE ONLY (same rules as cpu_ref.py).

The companion of oracle/parity.py for cross-entropy, RMSNorm, SwiGLU, the plain MLP activations and the stand-alone RoPE
pass.  One global number, max|got - ref| / max|ref|, misses the defects these kernels are prone to: a register chunk of a
dlogits row 2 % off sits at ~1e-6 of the row's maximum (the target column), and a dropped or extra bf16 rounding moves a
large fraction of the elements by one ulp, well inside a per-cent tolerance.  This file measures them the ways that
separate such defects from honest rounding:

  * fp64 references from the exact operands a kernel read (bf16 tensors, fp32 inputs, the fp32 cos / sin table), rounded
    to bf16 exactly where the kernel's contract rounds (plm_device.h, elementwise.hip, ce.hip) and nowhere else; the
    final rounding of an output is left out, so ``ulp`` below sees how far the result is from the exact value;
  * bf16 element-wise outputs (``elementwise``): ``ulp`` = the largest distance from the reference in bf16 ulps of the
    reference, and ``neq`` = the fraction of elements that are not bit-equal to the correctly rounded reference.  An
    honest kernel differs from fp64 only by fp32 round-off before its bf16 roundings, so it is bit-equal almost
    everywhere; a kernel that rounds in another order is one ulp off on a large fraction of its elements;
  * cross-entropy rows (``ce``): per-row loss against lse - x_t in nats, dlogits element by element relative to
    (p_j - onehot) * grad_scale (never relative to a row's or the tensor's maximum), and exact zeros for ignored rows and
    pad columns;
  * RMSNorm (``rmsnorm_fwd`` / ``rmsnorm_bwd``): rstd relative per row, dx row-local (each row on its own scale, as
    parity.py), dw per column relative to that column's sum of |dy * x_hat| (the size of the terms it adds).

Cancellation.  Where a formula cancels, fp32 round-off before the bf16 rounding is large against the result, and an
absolute allowance derived from the formula's condition is subtracted from the error before it is measured (the
docstrings of ``silu_bwd_allow``, ``rope_reference`` and ``ce_reference`` derive theirs).  Errors below ``FLOOR`` are
ignored everywhere: an fp32 intermediate below the normal range (2^-126) that the device flushes - or keeps as a
denormal - moves a result by at most |factor| * 2^-126 with |factor| well below 2^26 here, so no bound depends on the
device's denorm mode.

BOUNDS holds every bound the GPU tests (tests/test_ops_parity_gpu.py and the budget calls in test_kernels_gpu.py /
test_bench_size_gpu.py) and tests/test_parity_budget_ops.py share.  Each is at least 2x above the larger of the honest
floor (that file's fp32 stand-ins, which round where the kernels round) and the worst value the MI355X kernels show, and
at least 2x below the smallest value a planted defect produces on the metric meant to catch it.
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import torch

Tensor = torch.Tensor
F64 = torch.float64
EPS = 2.0 ** -24      # fp32 unit round-off
FLOOR = 2.0 ** -100   # absolute errors below this are ignored (fp32 denormals times factors < 2^26; see above)
NEQ_MIN = 512         # ``neq`` of a smaller tensor is counted over this many elements (see ``elementwise``)

BOUNDS = {
    'ulp': 4.0,         # max distance from the fp64 reference in bf16 ulps, beyond the cancellation allowance
    'neq': 5e-3,        # fraction of elements not bit-equal to the correctly rounded fp64 reference
    'ce_loss': 3e-5,    # max |loss_row - (lse - x_t)|, nats
    'ce_rel': 8e-3,     # max |dlogit - (p - onehot) gs| / |(p - onehot) gs|, beyond the allowance
    'ce_zero': 0.0,     # max |value| of an ignored row's loss and gradient and of the pad columns
    'rstd': 2e-6,       # max relative error of rstd per row
    'rms_dx': 1e-5,     # row-local dx: max over rows of max|err| / rowmax|ref|
    'rms_dw': 1e-5,     # max over columns of |err| / sum_rows |dy * x_hat|
}


# --------------------------------------------------------------------------------------
# bf16 arithmetic in fp64
# --------------------------------------------------------------------------------------
def _exp2i(e: Tensor) -> Tensor:
  """2^e as fp64, assembled from its bits (|e| < 1023): exact on every device (a device's pow need not return exact powers of two)."""
  return ((e.to(torch.int64) + 1023) << 52).view(F64)


def ulp_of(v: Tensor) -> Tensor:
  """The bf16 ulp at |v| (8 significant bits; below 2^-126 the fixed spacing 2^-133 of bf16 denormals)."""
  v = v.double()
  _, e = torch.frexp(v)                     # v = m 2^e, 0.5 <= |m| < 1: the leading bit is 2^(e-1)
  e = torch.where(v == 0, torch.full_like(e, -125), e)
  return _exp2i((e - 8).clamp_min(-133))


def bf16_rne(v: Tensor) -> Tensor:
  """fp64 -> the nearest bf16 value (ties to even), as fp64: rounded once (torch's double -> bf16 goes through fp32)."""
  v = v.double()
  u = ulp_of(v)
  return torch.round(v / u) * u             # torch.round: half to even; v / u is exact (u a power of two)


def rb(v: Tensor) -> Tensor:
  """bf16 rounding of an fp64 intermediate, kept in fp64 (the contract points of the references)."""
  return bf16_rne(v)


def merge(*ms: Dict[str, float]) -> Dict[str, float]:
  """Worst of several metric dicts, key by key.  NaN wins: Python's max(prev, nan) would keep prev, and a NaN metric
  (a NaN in the result) must reach ``violations``."""
  out: Dict[str, float] = {}
  for m in ms:
    for k, v in m.items():
      prev = out.get(k, 0.0)
      out[k] = prev if math.isnan(prev) else (v if math.isnan(v) or v > prev else prev)
  return out


def elementwise(got: Tensor, ref: Tensor, allow: Optional[Tensor] = None) -> Dict[str, float]:
  """{'ulp', 'neq'} of a bf16 result against its fp64 reference (final rounding not applied), after the absolute
  allowance ``allow`` (same shape, or None) and FLOOR.  A non-finite result against a finite reference counts as infinitely
  far.  ``neq`` divides by at least NEQ_MIN elements, so a tensor smaller than that may have up to
  BOUNDS['neq'] * NEQ_MIN = 2.56, i.e. 2 mismatches (an honest kernel flips ~1e-3 of its elements; one flip among 96 is no 1 % rate).
  The budget's own cases all have at least 4096 elements; only the smallest shapes of the older tests (RMSNorm 5 x 64)
  fall under this floor.  Evaluated on ``ref``'s device (the CPU for every reference of this file; parity_gemm.py keeps its
  full-size GEMM references on the GPU)."""
  g = got.detach().to(ref.device).double()
  r = ref.double()
  slack = FLOOR if allow is None else allow.double() + FLOOR
  err = torch.where(torch.isfinite(g), (g - r).abs(), torch.full_like(g, float('inf')))
  beyond = (err - slack).clamp_min(0.0)
  n = max(g.numel(), 1)
  ulp = (beyond / ulp_of(r)).max().item() if g.numel() else 0.0
  neq = ((g != bf16_rne(r)) & (err > slack)).sum().item() / max(n, NEQ_MIN)
  return {'ulp': ulp, 'neq': neq}


# --------------------------------------------------------------------------------------
# SiLU / SwiGLU / ReLU^2 (elementwise.hip; plm_sigmoid / plm_swiglu_bf16 in plm_device.h)
# --------------------------------------------------------------------------------------
def _sig(x: Tensor) -> Tensor:
  return torch.sigmoid(x.double())


def silu_bwd_allow(x: Tensor, scale: Tensor) -> Tensor:
  """Absolute allowance for |scale| * dsilu(x), dsilu = sig (1 + x (1 - sig)), evaluated in fp32 by plm_sigmoid
  (rcp(1 + exp2(-x log2e)), each 1 ulp).  First order: e = exp2(-x log2e) carries a relative error of
  (1.5 |x| + 4) EPS (the rounded product x * log2e, exp2, the rounding of 1 + e), so sig carries an absolute
  sig (1 - sig) (1.5 |x| + 4) EPS + 2 sig EPS (rcp); dsilu = sig + x sig (1 - sig) moves by |1 + x (1 - 2 sig)| times that,
  plus three roundings of its terms.  Near the zero of dsilu at x = -2.40 the result cancels and this term dominates;
  elsewhere it is ~1e-3 ulp.  Doubled for safety."""
  x = x.double()
  s = _sig(x)
  sig_abs = s * (1 - s) * (1.5 * x.abs() + 4) * EPS + 2 * s * EPS
  d_abs = (1 + x * (1 - 2 * s)).abs() * sig_abs + (s + (x * s * (1 - s)).abs()) * 3 * EPS
  return 2.0 * scale.double().abs() * d_abs


def swiglu_fwd_reference(u: Tensor) -> Tensor:
  """out = bf16(bf16(silu(x)) * z) for u = [x | z] bf16 [M, 2h]: returns s * z in fp64 (s rounded, the product not)."""
  h = u.shape[1] // 2
  x, z = u[:, :h].double().cpu(), u[:, h:].double().cpu()
  return rb(x * _sig(x)) * z


def swiglu_bwd_reference(dout: Tensor, u: Tensor):
  """swiglu_bwd_kernel: s = bf16(silu(x)), ds = bf16(g z), dz = bf16(g s), dx = bf16(ds dsilu(x)).  Returns
  (ref [M, 2h] = [ds dsilu(x) | g s] un-rounded, allowance [M, 2h])."""
  h = u.shape[1] // 2
  x, z, g = u[:, :h].double().cpu(), u[:, h:].double().cpu(), dout.double().cpu()
  s = _sig(x)
  ds = rb(g * z)
  dx = ds * s * (1 + x * (1 - s))
  dz = g * rb(x * s)
  return torch.cat([dx, dz], 1), torch.cat([silu_bwd_allow(x, ds), torch.zeros_like(dz)], 1)


def act_fwd_reference(u: Tensor, kind: str) -> Tensor:
  """act_fwd_kernel: silu -> x sig(x); relu_sq -> r * r of the bf16 r = max(x, 0) (rounded once, by the caller's metric)."""
  x = u.double().cpu()
  if kind == 'silu':
    return x * _sig(x)
  r = x.clamp_min(0.0)
  return r * r


def act_bwd_reference(dout: Tensor, u: Tensor, kind: str):
  """act_bwd_kernel: silu -> bf16(g dsilu(x)); relu_sq -> bf16(g * 2 * max(x, 0)) (pow's backward, then relu's mask).
  Returns (ref un-rounded, allowance or None)."""
  x, g = u.double().cpu(), dout.double().cpu()
  if kind == 'silu':
    s = _sig(x)
    return g * s * (1 + x * (1 - s)), silu_bwd_allow(x, g)
  return g * 2.0 * x.clamp_min(0.0), None


# --------------------------------------------------------------------------------------
# RoPE (rope_qk_kernel, attn.hip; rope8 in plm_device.h)
# --------------------------------------------------------------------------------------
def rope_reference(qkv: Tensor, cos: Tensor, sin: Tensor, B: int, T: int, nh: int):
  """The q | k blocks of the projection qkv bf16 [B*T, 3*nh*hd] rotated in fp64 with the fp32 tables [>= T, hd/2]:
  (a c - b s, b c + a s) per interleaved pair, token row r at position r % T.  Returns (ref [B*T, 2*nh*hd], allowance):
  fp32 rounds the two products and their sum, at most 2 EPS (|a c| + |b s|) together - the whole error where the two
  terms cancel; doubled for safety."""
  d = qkv.shape[1] // 3
  hd = d // nh
  x = qkv[:, :2 * d].double().cpu().reshape(B, T, 2 * nh, hd // 2, 2)
  c = cos[:T].double().cpu().reshape(1, T, 1, hd // 2)
  s = sin[:T].double().cpu().reshape(1, T, 1, hd // 2)
  a, b = x[..., 0], x[..., 1]
  ref = torch.stack([a * c - b * s, b * c + a * s], -1).reshape(B * T, 2 * d)
  mag = (a * c).abs() + (b * s).abs()
  allow = 4.0 * EPS * torch.stack([mag, (b * c).abs() + (a * s).abs()], -1).reshape(B * T, 2 * d)
  return ref, allow


# --------------------------------------------------------------------------------------
# RMSNorm (rmsnorm_fwd_kernel / rmsnorm_bwd_kernel, elementwise.hip)
# --------------------------------------------------------------------------------------
def rmsnorm_fwd_reference(r: Tensor, w: Tensor, eps: float):
  """r fp32 [M, d] (x + bf16 branch, the kernel's xout), w fp32 [d] -> (y = r rstd w un-rounded, rstd) in fp64."""
  r, w = r.double().cpu(), w.double().cpu()
  rstd = torch.rsqrt(r.pow(2).mean(-1) + eps)
  return r * rstd[:, None] * w, rstd


def rmsnorm_bwd_reference(dy: Tensor, r: Tensor, w: Tensor, rstd: Tensor):
  """From the operands the backward reads (bf16 dy, fp32 r, w, the fp32 rstd of the forward): the norm's own
  dx = rstd dy w - r (sum(dy w r) rstd^3 / d) (without the incoming gin, see ``rmsnorm_bwd``), dw = sum_rows dy r rstd, and
  sum_rows |dy r rstd| (dw's scale)."""
  dy, r, w, rstd = (t.double().cpu() for t in (dy, r, w, rstd))
  d = r.shape[1]
  a = dy * w
  coef = (a * r).sum(-1, keepdim=True) * rstd[:, None] ** 3 / d
  dx = rstd[:, None] * a - r * coef
  t = dy * r * rstd[:, None]
  return dx, t.sum(0), t.abs().sum(0)


def rmsnorm_fwd(y: Tensor, rstd: Tensor, ref_y: Tensor, ref_rstd: Tensor) -> Dict[str, float]:
  m = elementwise(y, ref_y)
  m['rstd'] = ((rstd.detach().cpu().double() - ref_rstd).abs() / ref_rstd).nan_to_num(nan=float('inf'), posinf=float('inf')).max().item()
  return m


def rmsnorm_bwd(dx: Tensor, dw: Optional[Tensor], ref_dx: Tensor, ref_dw: Tensor, dw_scale: Tensor,
                gin: Optional[Tensor] = None) -> Dict[str, float]:
  """rms_dx judges the norm's part of dx on its own row scale: with an incoming gradient gin (the kernel returns
  fp32(dx_norm + gin)), dx - gin is compared, less the one fp32 rounding of that add (EPS |dx_norm + gin|) - a gin of
  size 1 would otherwise hide a relative error of the ~1e-3 dx_norm of a 1e3-scale row.  rms_dw is per column."""
  g = dx.detach().cpu().double()
  allow = torch.zeros_like(g)
  if gin is not None:
    gi = gin.detach().cpu().double()
    g = g - gi
    allow = EPS * (ref_dx + gi).abs()
  err = ((g - ref_dx).abs() - allow).clamp_min(0.0).nan_to_num(nan=float('inf'), posinf=float('inf'))
  m = {'rms_dx': (err.amax(-1) / ref_dx.abs().amax(-1).clamp_min(FLOOR)).max().item()}
  if dw is not None:
    m['rms_dw'] = ((dw.detach().cpu().double() - ref_dw).abs() / dw_scale.clamp_min(FLOOR)).nan_to_num(nan=float('inf'), posinf=float('inf')).max().item()
  return m


# --------------------------------------------------------------------------------------
# cross-entropy (ce.hip)
# --------------------------------------------------------------------------------------
def ce_reference(logits: Tensor, targets: Tensor, grad_scale: float, V: int):
  """bf16 logits [M, >= V] (the values BEFORE the in-place kernel), int64 targets [M] -> dict of fp64 references:
  'dl' = (p - onehot) * gs [M, V] (zeros on ignored rows: target < 0 or >= V), 'loss' = lse - x_t (0 when ignored),
  'valid' bool [M], and 'allow': the absolute allowance of each dlogit.  The kernel evaluates p_j = exp2(x_j log2e - lse
  log2e) in fp32: the rounded product, lse's own error (|lse| EPS from the add, ~30 EPS from the sum of V exponentials)
  and exp2's ulp give p_j a relative error of at most (1.5 (|x_j| + 2 |lse|) + 32) EPS.  That is ~1e-3 ulp - except at the
  target, where p_t - 1 cancels (a saturated row: p_t = 1 - 1e-17); the allowance p_j gs times that relative error covers
  it.  Doubled for safety."""
  x = logits[:, :V].double().cpu()
  t = targets.cpu().long()
  M = x.shape[0]
  valid = (t >= 0) & (t < V)
  lse = torch.logsumexp(x, -1)
  p = torch.exp(x - lse[:, None])
  dl = p * grad_scale
  rows = torch.arange(M)[valid]
  dl[rows, t[valid]] = (p[rows, t[valid]] - 1.0) * grad_scale
  dl[~valid] = 0.0
  loss = torch.where(valid, lse - x.gather(1, t.clamp(0, V - 1)[:, None])[:, 0], torch.zeros_like(lse))
  allow = 2.0 * p * abs(grad_scale) * (1.5 * (x.abs() + 2 * lse.abs()[:, None]) + 32) * EPS
  return {'dl': dl, 'loss': loss, 'valid': valid, 'allow': allow, 'V': V}


def ce(got_logits: Tensor, got_loss: Tensor, ref: Dict[str, Tensor]) -> Dict[str, float]:
  """Metrics of the kernel's in-place result got_logits bf16 [M, ld] and per-row losses [M] against ce_reference."""
  V, valid = ref['V'], ref['valid']
  g = got_logits.detach().cpu().double()
  gl = got_loss.detach().cpu().double()
  gv = g[:, :V][valid]
  rv, av = ref['dl'][valid], ref['allow'][valid]
  m = elementwise(gv, rv, av) if gv.numel() else {'ulp': 0.0, 'neq': 0.0}
  err = torch.where(torch.isfinite(gv), (gv - rv).abs(), torch.full_like(gv, float('inf')))
  m['ce_rel'] = ((err - av - FLOOR).clamp_min(0.0) / rv.abs().clamp_min(FLOOR)).max().item() if gv.numel() else 0.0
  lerr = (gl - ref['loss']).abs().nan_to_num(nan=float('inf'), posinf=float('inf'))
  m['ce_loss'] = lerr[valid].max().item() if valid.any() else 0.0
  zero = torch.cat([g[~valid].flatten(), gl[~valid], g[:, V:].flatten(), torch.zeros(1, dtype=F64)])
  m['ce_zero'] = zero.abs().nan_to_num(nan=float('inf'), posinf=float('inf')).max().item()
  return m


# --------------------------------------------------------------------------------------
def violations(m: Dict[str, float]) -> Dict[str, tuple]:
  """{metric: (value, bound)} for every metric above its bound (NaN counts as above)."""
  return {k: (v, BOUNDS[k]) for k, v in m.items() if not v <= BOUNDS[k]}


def check(m: Dict[str, float], tag: str) -> Dict[str, float]:
  """Assert every metric within BOUNDS; prints them (one line, 'parity_ops <tag>: ...') either way."""
  print(f'parity_ops {tag}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  bad = violations(m)
  assert not bad, f'{tag}: ' + ', '.join(f'{k} {v:.3e} > {b:.1e}' for k, (v, b) in bad.items())
  return m


# --------------------------------------------------------------------------------------
# inputs and shapes shared by the GPU tests and the CPU calibration (the budget is calibrated on exactly these)
# --------------------------------------------------------------------------------------
BF16 = torch.bfloat16

# one row of each class per 11 rows: ordinary, targets at both ends, a saturated row (the target 40 above the rest: p_t - 1
# cancels) and one saturated elsewhere, an all-equal row, logits over +-60, the row maximum in the last 8-element vector
# (target there too), and the three ignored targets
CE_CLASSES = ('randn', 'target_0', 'target_last', 'saturated_target', 'saturated_other', 'all_equal', 'wide', 'max_last_vec',
              'ignore_-1', 'ignore_-100', 'ignore_V')


def ce_inputs(M: int, V: int, seed: int):
  """(bf16 logits [M, V], int64 targets [M]) with row i of class CE_CLASSES[i % 11]."""
  g = torch.Generator().manual_seed(seed)
  x = 3 * torch.randn(M, V, generator=g)
  t = torch.randint(0, V, (M,), generator=g)
  wide = torch.rand(M, V, generator=g) * 120 - 60
  for i in range(M):
    k = CE_CLASSES[i % len(CE_CLASSES)]
    if k == 'target_0':
      t[i] = 0
    elif k == 'target_last':
      t[i] = V - 1
    elif k == 'saturated_target':
      x[i, t[i]] = x[i].max() + 40
    elif k == 'saturated_other':
      x[i, (t[i] + V // 2) % V] = x[i].max() + 40
    elif k == 'all_equal':
      x[i] = 1.5
    elif k == 'wide':
      x[i] = wide[i]
    elif k == 'max_last_vec':
      x[i, V - 1 - i % min(8, V)] = x[i].max() + 8
      t[i] = max(V - 3, 0)
    elif k.startswith('ignore'):
      t[i] = {'ignore_-1': -1, 'ignore_-100': -100, 'ignore_V': V}[k]
  return x.to(BF16), t


# (M, V, ld): every fast-path template (NCH 1: V 8, 8192; NCH 2: 8200, 16384; NCH 4: 16392 (chunk 3 empty), 32000, 32768;
# NCH 7: 40000 and 48000 (chunks 5-6 / 6 empty), 50280 (+ pad columns); NCH 8: 65536) and the generic kernel (V % 8 != 0,
# V > 65536, ld % 8 != 0, ld > V)
CE_CASES = [(704, 8, 8), (22, 8192, 8192), (22, 8200, 8200), (22, 16384, 16384), (22, 16392, 16392), (22, 32000, 32000),
            (22, 32768, 32768), (22, 40000, 40000), (22, 48000, 48000), (22, 50280, 50280), (22, 50280, 50304), (22, 65536, 65536),
            (22, 777, 777), (22, 777, 800), (22, 70000, 70000), (22, 1024, 1028)]


def rms_inputs(M: int, d: int, seed: int, branch: bool):
  """(x fp32, w fp32, branch bf16 or None, dy bf16, gin fp32 or None) [M, d]: rows i % 7 == 3 scaled by 1e-3 (eps matters),
  i % 7 == 5 all zero, i % 11 == 4 scaled by 1e3."""
  g = torch.Generator().manual_seed(seed)
  x = torch.randn(M, d, generator=g)
  br = 0.5 * torch.randn(M, d, generator=g)
  rows = torch.arange(M)
  sc = torch.ones(M)
  sc[rows % 7 == 3] = 1e-3
  sc[rows % 7 == 5] = 0.0
  sc[rows % 11 == 4] = 1e3
  x, br = x * sc[:, None], br * sc[:, None]
  w = 1 + 0.1 * torch.randn(d, generator=g)
  dy = torch.randn(M, d, generator=g).to(BF16)
  gin = torch.randn(M, d, generator=g)
  return x, w, (br.to(BF16) if branch else None), dy, (gin if branch else None)


# (M, d, with branch + gin): every RMSNorm template (NCH 1: d <= 256; 3: <= 768; 4: <= 1024; 8: <= 2048) with full and
# partly filled chunks, and M above 4096 (the backward's 1024-block grid then loops over rows)
RMS_CASES = [(67, d, b) for d in (4, 64, 260, 516, 768, 1020, 1028, 1280, 1536, 2044, 2048) for b in (False, True)] + \
            [(4100, 1028, True), (8200, 2048, True), (8200, 516, False)]


def act_inputs(M: int, n: int, seed: int):
  """bf16 [M, n] over the exact-bf16 range that matters to the activations: |x| log-uniform on [1e-3, 100] with both signs
  (past 88.7 exp2(-x log2e) overflows fp32), a band on [-2.9, -1.9] around the zero of dsilu (-2.40), and 2 * randn."""
  g = torch.Generator().manual_seed(seed)
  mag = torch.exp(torch.rand(M, n, generator=g) * (torch.log(torch.tensor(100.0)) - torch.log(torch.tensor(1e-3))) + torch.log(torch.tensor(1e-3)))
  sign = torch.where(torch.rand(M, n, generator=g) < 0.5, -1.0, 1.0)
  band = -2.9 + torch.rand(M, n, generator=g)
  nrm = 2 * torch.randn(M, n, generator=g)
  pick = torch.randint(0, 4, (M, n), generator=g)
  x = torch.where(pick < 2, sign * mag, torch.where(pick == 2, band, nrm))
  return x.to(BF16)


# SwiGLU (M, h) and activation (M, n) shapes: h / 8 and n / 8 not multiples of the 256-thread block (partial blocks)
# (every case has at least 4096 elements: ``neq`` is a plain fraction on all of them)
SWIGLU_CASES = [(57, 72), (5, 2072), (3, 2816), (528, 8)]
ACT_CASES = [(7, 2072), (3, 5632), (57, 72)]

# (hd, B, T, nh, table rows): head dims 32 / 64 / 128, B > 1, T off every tile, the 420M table (2048 rows) in full
ROPE_CASES = [(32, 3, 100, 2, 2048), (32, 1, 2048, 4, 2048), (64, 2, 1000, 3, 1000), (64, 1, 2048, 4, 2048),
              (128, 2, 2048, 2, 2048), (128, 3, 100, 1, 100)]
