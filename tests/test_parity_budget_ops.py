"""The error budget of the non-attention kernels (oracle/parity_ops.py) against planted defects, on the CPU.

Each stand-in below is the kernel's arithmetic restated in fp32 torch, rounding to bf16 where the kernel rounds (ce.hip,
elementwise.hip, rope_qk_kernel in attn.hip): it is what an honest kernel looks like under the budget.  Each defect is a
small edit of a stand-in of the kind a rewrite of those kernels tends to introduce: a register chunk scaled, a vector left
out of a reduction, a rounding dropped or added, a neighbour's statistic, a wrong table entry.  The budget must ACCEPT every
stand-in at every shape and input class of tests/test_ops_parity_gpu.py and REJECT every defect by at least 2x its bound -
at least half of the defects pass the rel-to-max tolerances the older tests apply (asserted below).  Nothing here launches a
kernel."""

import math

import pytest
import torch

from oracle import cpu_ref as O
from oracle import cpu_ref_bf16 as E
from oracle import parity_ops as P

BF16 = torch.bfloat16
L2E = E.LOG2E


def rb(x):
  return x.to(BF16).float()


def relmax(got, ref):
  """The older tests' yardstick: max|got - ref| / max|ref|."""
  got, ref = got.double(), ref.double()
  return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


# ---------------------------------------------------------------------------------------------------------------------
# stand-ins (with the defects' hooks)
# ---------------------------------------------------------------------------------------------------------------------
def ce_standin(x_bf, t, gs, V, ld, defect=None, at=0):
  """ce_fwd_bwd_kernel: max / sum of exp2 over the row, lse = m + log(s), p = exp2(x log2e - lse log2e), bf16(p gs), the
  target fixed up to bf16((p_t - 1) gs), ignored rows 0, pad columns 0.  Returns (logits bf16 [M, ld], loss fp32 [M])."""
  x = x_bf[:, :V].float()
  M = x.shape[0]
  valid = (t >= 0) & (t < V)
  xs = x[:, :V - 8] if defect == 'ce_skip_last_vec' else x       # the last 8-element vector left out of (max, sum)
  m = xs.max(-1).values
  s = torch.exp2(xs * L2E - (m * L2E)[:, None]).sum(-1)
  lse = m + torch.log(s)
  if defect == 'ce_lse_shift':
    lse[at] += math.log1p(2.0 ** -8)
  p = torch.exp2(x * L2E - (lse * L2E)[:, None])
  g = torch.full((M, 1), gs) if defect == 'ce_ignored_grad' else torch.where(valid, gs, 0.0)[:, None]
  dl = p * g
  if defect == 'ce_last_chunk_scale':                            # the last register chunk of row `at` 2^-6 off
    nch = -(-(V // 8) // 1024)
    dl[at, 8 * 1024 * (nch - 1):] *= 1 + 2.0 ** -6
  out = rb(rb(p) * g) if defect == 'ce_double_round' else rb(dl)
  rows = torch.arange(M)[valid]
  tt = t[valid]
  pt = p[rows, tt]
  fix = rb((pt - 1.0) * gs)
  if defect == 'ce_target_no_minus1':                            # the fix-up of a target in the final vector without the -1
    fix = torch.where(tt >= V - 8, rb(pt * gs), fix)
  out[rows, tt] = fix
  res = torch.zeros(M, ld)
  res[:, :V] = out
  loss = torch.where(valid, lse - x.gather(1, t.clamp(0, V - 1)[:, None])[:, 0], torch.zeros(M))
  return res.to(BF16), loss


def _nch_rms(d):
  return 1 if d <= 256 else 3 if d <= 768 else 4 if d <= 1024 else 8


def rms_fwd_standin(x, br, w, eps, defect=None, at=0):
  """rmsnorm_fwd_kernel: r = x + bf16 branch, rstd = rsqrt(sum r^2 / d + eps), y = bf16((r rstd) w).  -> (r, y, rstd)."""
  r = x + br.float() if br is not None else x
  d = r.shape[1]
  ss = (r * r).sum(-1)
  n = 256 * _nch_rms(d) if defect == 'rms_pad_mean' else d      # the mean over the padded chunk width
  rstd = torch.rsqrt(ss / n) + eps if defect == 'rms_eps_outside' else torch.rsqrt(ss / n + eps)
  ry = rstd.clone()
  if defect == 'rms_neighbour_rstd':
    ry[at] = rstd[at + 1]
  y = rb(rb(r * ry[:, None]) * w) if defect == 'rms_y_double_round' else rb((r * ry[:, None]) * w)
  return r, y.to(BF16), rstd


def rms_bwd_standin(dy, r, w, rstd, gin, defect=None, at=0):
  """rmsnorm_bwd_kernel (cpu_ref_bf16._rms_bwd).  -> (dx fp32, dw fp32)."""
  dx, dw = E._rms_bwd(dy.float(), r, w, rstd[:, None], gin)
  if defect == 'rms_dx_pad_width':                               # coef = dot rstd^3 / (padded chunk width) instead of / d
    a = dy.float() * w
    coef = (a * r).sum(-1, keepdim=True) * rstd[:, None] ** 3 / (256 * _nch_rms(r.shape[1]))
    dx = rstd[:, None] * a - r * coef + (gin if gin is not None else 0.0)
  if defect == 'rms_dw_block':                                   # block `at`'s partial (its 4 rows) left out of the column sum
    rows = slice(4 * at, 4 * at + 4)
    dw = dw - (dy.float()[rows] * (r[rows] * rstd[rows, None])).sum(0)
  return dx, dw


def sig32(x, round_sig=False):
  s = E._sigmoid(x)
  return rb(s) if round_sig else s


def swiglu_fwd_standin(u, defect=None):
  h = u.shape[1] // 2
  x, z = u[:, :h].float(), u[:, h:].float()
  s = x * sig32(x)
  return rb((s if defect == 'swiglu_no_silu_round' else rb(s)) * z).to(BF16)


def swiglu_bwd_standin(dout, u, defect=None):
  h = u.shape[1] // 2
  x, z, g = u[:, :h].float(), u[:, h:].float(), dout.float()
  sig = sig32(x, defect == 'swiglu_bwd_sig_round')             # an extra bf16 rounding of sig in the backward only
  s = x * sig
  ds = rb(g * z)
  dz = rb(g * (s if defect == 'swiglu_dz_unrounded_s' else rb(s)))
  dx = rb(ds * (sig * (1.0 + x * (1.0 - sig))))
  return torch.cat([dx, dz], 1).to(BF16)


def act_fwd_standin(u, kind, defect=None):
  x = u.float()
  if kind == 'silu':
    return rb(x * sig32(x, defect == 'act_fwd_sig_round')).to(BF16)
  r = x.clamp_min(0.0)
  return rb(r * r).to(BF16)


def act_bwd_standin(dout, u, kind, defect=None):
  x, g = u.float(), dout.float()
  if kind == 'silu':
    sig = sig32(x, defect == 'act_bwd_sig_round')
    return rb(g * (sig * (1.0 + x * (1.0 - sig)))).to(BF16)
  r = x.clamp_min(0.0)
  if defect == 'relu2_bwd_from_output':                          # r taken back from the stored bf16 activation
    r = torch.sqrt(rb(r * r))
  return rb(g * 2.0 * r).to(BF16)


def rope_standin(qkv, cos, sin, B, T, nh, defect=None, at=0):
  """rope_qk_kernel: interleaved pairs of the q | k blocks, row r at position r % T, fp32 math, bf16 result."""
  d = qkv.shape[1] // 3
  hd = d // nh
  pos = torch.arange(B * T) % T
  if defect == 'rope_pos_off':                                   # the first row of the second sequence one position off
    pos[T] += 1
  pair = torch.arange(hd // 2)
  if defect == 'rope_pair_mod32':
    pair = pair % 32
  c, s = cos[pos][:, pair].clone(), sin[pos][:, pair].clone()
  if defect == 'rope_sin_last':
    s[:, -1] = -s[:, -1]
  if defect == 'rope_bf16_table':
    c, s = rb(c), rb(s)
  x = qkv[:, :2 * d].float().reshape(B * T, 2 * nh, hd // 2, 2)
  a, b = x[..., 0], x[..., 1]
  c, s = c[:, None], s[:, None]
  out = torch.stack([rb(a * c - b * s), rb(b * c + a * s)], -1).reshape(B * T, 2 * d)
  return torch.cat([out, qkv[:, 2 * d:].float()], 1).to(BF16)


# ---------------------------------------------------------------------------------------------------------------------
# one measurement per family: (budget metrics, the older tests' pass / fail)
# ---------------------------------------------------------------------------------------------------------------------
def measure_ce(M, V, ld, seed=0, defect=None, at=0):
  x, t = P.ce_inputs(M, V, seed)
  gs = 1.0 / M
  got, loss = ce_standin(x, t, gs, V, ld, defect, at)
  ref = P.ce_reference(x, t, gs, V)
  m = P.ce(got, loss, ref)
  valid = ref['valid']
  mean_ok = abs(loss[valid].double().mean().item() - ref['loss'][valid].mean().item()) <= 2e-6 * abs(ref['loss'][valid].mean().item()) + 1e-6
  old = mean_ok and relmax(got[:, :V].float(), ref['dl']) <= 8e-3 and bool((got[:, V:] == 0).all())
  return m, old


def measure_rms(M, d, branch, seed=0, defect=None, at=0):
  x, w, br, dy, gin = P.rms_inputs(M, d, seed, branch)
  r, y, rstd = rms_fwd_standin(x, br, w, 1e-6, defect, at)
  dx, dw = rms_bwd_standin(dy, r, w, rstd, gin, defect, at)
  ref_y, ref_rstd = P.rmsnorm_fwd_reference(r, w, 1e-6)
  ref_dx, ref_dw, dw_scale = P.rmsnorm_bwd_reference(dy, r, w, rstd)
  m = P.merge(P.rmsnorm_fwd(y, rstd, ref_y, ref_rstd), P.rmsnorm_bwd(dx, dw, ref_dx, ref_dw, dw_scale, gin))
  ref_dx_all = ref_dx if gin is None else ref_dx + gin.double()
  old = relmax(y.float(), ref_y) <= 6e-3 and relmax(rstd, ref_rstd) <= 1e-5 and relmax(dx, ref_dx_all) <= 2e-5 and relmax(dw, ref_dw) <= 2e-5
  return m, old


def measure_swiglu(M, h, seed=0, defect=None):
  u = P.act_inputs(M, 2 * h, seed)
  dout = torch.randn(M, h, generator=torch.Generator().manual_seed(seed + 1)).to(BF16)
  out, du = swiglu_fwd_standin(u, defect), swiglu_bwd_standin(dout, u, defect)
  ref_bwd, allow = P.swiglu_bwd_reference(dout, u)
  ref_fwd = P.swiglu_fwd_reference(u)
  m = P.merge(P.elementwise(out, ref_fwd), P.elementwise(du, ref_bwd, allow))
  return m, relmax(out.float(), ref_fwd) <= 1.6e-2 and relmax(du.float(), ref_bwd) <= 1.6e-2


def measure_act(M, n, kind, seed=0, defect=None):
  u = P.act_inputs(M, n, seed)
  dout = torch.randn(M, n, generator=torch.Generator().manual_seed(seed + 1)).to(BF16)
  out, du = act_fwd_standin(u, kind, defect), act_bwd_standin(dout, u, kind, defect)
  ref_fwd = P.act_fwd_reference(u, kind)
  ref_bwd, allow = P.act_bwd_reference(dout, u, kind)
  m = P.merge(P.elementwise(out, ref_fwd), P.elementwise(du, ref_bwd, allow))
  return m, relmax(out.float(), ref_fwd) <= 1.6e-2 and relmax(du.float(), ref_bwd) <= 1.6e-2


def measure_rope(hd, B, T, nh, tab, seed=0, defect=None, at=0):
  d = nh * hd
  qkv = torch.randn(B * T, 3 * d, generator=torch.Generator().manual_seed(seed)).to(BF16)
  cos, sin = O.rope_table(hd, tab)
  got = rope_standin(qkv, cos, sin, B, T, nh, defect, at)
  ref, allow = P.rope_reference(qkv, cos, sin, B, T, nh)
  m = P.elementwise(got[:, :2 * d], ref, allow)
  assert torch.equal(got[:, 2 * d:], qkv[:, 2 * d:])
  return m, relmax(got[:, :2 * d].float(), ref) <= 8e-3


# ---------------------------------------------------------------------------------------------------------------------
# the references and the rounding helper
# ---------------------------------------------------------------------------------------------------------------------
def test_bf16_rne_is_torch_rounding_on_fp32_values():
  """bf16_rne agrees with torch's fp32 -> bf16 (RNE) on fp32 values, ties and the bf16 denormal range included."""
  g = torch.Generator().manual_seed(0)
  x = torch.cat([torch.randn(100000, generator=g) * torch.exp2(torch.randint(-140, 120, (100000,), generator=g).float()),
                 torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 2 ** -8), 2.0 ** -130, 3 * 2.0 ** -134, 0.0])])
  assert torch.equal(P.bf16_rne(x.double()), x.to(BF16).double())


def test_references_match_the_fp32_oracle():
  """The fp64 references are cpu_ref's operators (cross-entropy + autograd, rmsnorm, swiglu, mlp activations, rope_apply)
  once the contract's intermediate roundings are taken out: agreement to fp32 round-off."""
  x, t = P.ce_inputs(11, 300, 3)
  ok = (t >= 0) & (t < 300)
  leaf = x.float().requires_grad_(True)
  (O.cross_entropy(leaf[ok], t[ok]) * ok.sum()).backward()
  ref = P.ce_reference(x, t, 1.0, 300)
  assert (ref['dl'] - leaf.grad.double()).abs().max() < 1e-6
  assert (ref['loss'][ok].mean() - O.cross_entropy(x.float()[ok], t[ok]).double()).abs() < 1e-5
  xr, w, _, dy, _ = P.rms_inputs(9, 64, 1, False)
  rr, ww = xr.clone().requires_grad_(True), w.clone().requires_grad_(True)
  O.rmsnorm(rr, ww).backward(dy.float())
  ry, rstd = P.rmsnorm_fwd_reference(xr, w, 1e-6)
  dx, dw, _ = P.rmsnorm_bwd_reference(dy, xr, w, rstd)
  assert relmax(ry, O.rmsnorm(xr, w)) < 1e-6 and relmax(dx, rr.grad) < 1e-5 and relmax(dw, ww.grad) < 1e-5
  u = P.act_inputs(4, 64, 2)
  assert relmax(P.act_fwd_reference(u, 'silu'), O.mlp_act(u.float(), 0, 'mlp')) < 1e-6
  assert relmax(P.act_fwd_reference(u, 'relu_sq'), O.mlp_act(u.float(), 0, 'mlp_relu_sq')) < 1e-6
  assert relmax(P.swiglu_fwd_reference(u), O.swiglu(u.float(), 32)) < 2e-2   # one intermediate bf16 rounding apart
  qkv = torch.randn(2 * 8, 3 * 64, generator=torch.Generator().manual_seed(4)).to(BF16)
  cos, sin = O.rope_table(32, 8)
  ref, _ = P.rope_reference(qkv, cos, sin, 2, 8, 2)
  want = torch.cat([O.rope_apply(qkv[:, i * 64:(i + 1) * 64].float().reshape(2, 8, 2, 32), cos, sin).reshape(16, 64) for i in (0, 1)], 1)
  assert relmax(ref, want) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the honest stand-ins pass at every shape and input class of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def _report(name, worst, bad):
  print(f'honest floor {name}: ' + ' '.join(f'{k}={v:.2e}' for k, v in worst.items()))
  assert not bad, bad


@pytest.mark.parametrize('family', ['ce', 'rmsnorm', 'swiglu', 'act', 'rope'])
def test_honest_stand_in_within_budget(family):
  cases = {'ce': [(measure_ce, c) for c in P.CE_CASES],
           'rmsnorm': [(measure_rms, c) for c in P.RMS_CASES],
           'swiglu': [(measure_swiglu, c) for c in P.SWIGLU_CASES],
           'act': [(measure_act, c + (k,)) for c in P.ACT_CASES for k in ('silu', 'relu_sq')],
           'rope': [(measure_rope, c) for c in P.ROPE_CASES]}[family]
  worst, bad = {}, []
  for i, (fn, args) in enumerate(cases):
    m, _ = fn(*args, seed=i)
    worst = P.merge(worst, m)
    if P.violations(m):
      bad.append((args, P.violations(m)))
  _report(family, worst, bad)


# ---------------------------------------------------------------------------------------------------------------------
# every planted defect is rejected, by the metric meant to catch it
# ---------------------------------------------------------------------------------------------------------------------
DEFECTS = [
    # (id, measure, arguments, defect, where, metrics of which at least one must exceed its bound by 2x)
    ('ce_last_chunk_scale', measure_ce, (4, 16384, 16384), 'ce_last_chunk_scale', 0, ('neq',)),
    ('ce_lse_shift', measure_ce, (4, 16384, 16384), 'ce_lse_shift', 0, ('ce_loss',)),
    ('ce_skip_last_vec', measure_ce, (11, 32000, 32000), 'ce_skip_last_vec', 0, ('ce_loss', 'ce_rel')),
    ('ce_target_no_minus1', measure_ce, (11, 40000, 40000), 'ce_target_no_minus1', 0, ('ce_rel',)),
    ('ce_ignored_grad', measure_ce, (11, 8200, 8200), 'ce_ignored_grad', 0, ('ce_zero',)),
    ('ce_double_round', measure_ce, (12, 8192, 8192), 'ce_double_round', 0, ('neq',)),
    ('rms_pad_mean', measure_rms, (67, 1020, False), 'rms_pad_mean', 0, ('rstd', 'neq')),
    ('rms_eps_outside', measure_rms, (67, 768, True), 'rms_eps_outside', 0, ('rstd',)),
    ('rms_neighbour_rstd', measure_rms, (67, 1028, True), 'rms_neighbour_rstd', 0, ('ulp',)),
    ('rms_dx_pad_width', measure_rms, (67, 1020, False), 'rms_dx_pad_width', 0, ('rms_dx',)),
    ('rms_dw_block', measure_rms, (67, 516, False), 'rms_dw_block', 3, ('rms_dw',)),
    ('rms_y_double_round', measure_rms, (67, 2044, True), 'rms_y_double_round', 0, ('neq',)),
    ('swiglu_no_silu_round', measure_swiglu, (5, 2072), 'swiglu_no_silu_round', None, ('neq',)),
    ('swiglu_bwd_sig_round', measure_swiglu, (5, 2072), 'swiglu_bwd_sig_round', None, ('neq',)),
    ('swiglu_dz_unrounded_s', measure_swiglu, (5, 2072), 'swiglu_dz_unrounded_s', None, ('neq',)),
    ('act_fwd_sig_round', measure_act, (7, 2072, 'silu'), 'act_fwd_sig_round', None, ('neq',)),
    ('act_bwd_sig_round', measure_act, (7, 2072, 'silu'), 'act_bwd_sig_round', None, ('neq',)),
    ('relu2_bwd_from_output', measure_act, (7, 2072, 'relu_sq'), 'relu2_bwd_from_output', None, ('neq',)),
    ('rope_pair_mod32', measure_rope, (128, 2, 256, 2, 256), 'rope_pair_mod32', 0, ('ulp',)),
    ('rope_pos_off', measure_rope, (64, 2, 1000, 3, 1000), 'rope_pos_off', 0, ('ulp',)),
    ('rope_sin_last', measure_rope, (32, 2, 1024, 4, 2048), 'rope_sin_last', 0, ('ulp', 'neq')),
    ('rope_bf16_table', measure_rope, (64, 2, 1000, 3, 1000), 'rope_bf16_table', 0, ('neq',)),
]


def _run(fn, args, defect, at):
  kw = {'seed': 7, 'defect': defect}
  if at is not None:
    kw['at'] = at
  return fn(*args, **kw)


@pytest.mark.parametrize('name,fn,args,defect,at,caught_by', DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_is_rejected(name, fn, args, defect, at, caught_by):
  m, old = _run(fn, args, defect, at)
  print(f'{name}: passes the older tolerances: {old}; ' + ' '.join(f'{k}={v:.1e}' for k, v in m.items()))
  bad = P.violations(m)
  assert any(k in bad for k in caught_by), (name, {k: m[k] for k in caught_by})
  ratio = max((v / b if b > 0 else float('inf')) for k, (v, b) in bad.items() if k in caught_by)
  assert ratio >= 2.0, (name, {k: bad.get(k) for k in caught_by})


def test_most_defects_pass_the_older_tolerances():
  """The point of the budget: at least half of the planted defects pass the rel-to-max tolerances the older kernel tests
  apply (dlogits 8e-3 and the mean loss, RMSNorm y 6e-3 / rstd 1e-5 / dx, dw 2e-5, SwiGLU and activations 1.6e-2, RoPE 8e-3)."""
  passing = [name for name, fn, args, defect, at, _ in DEFECTS if _run(fn, args, defect, at)[1]]
  print(f'{len(passing)} of {len(DEFECTS)} defects pass the older tolerances: {passing}')
  assert 2 * len(passing) >= len(DEFECTS), passing


def test_sigmoid_error_explains_the_kernels_swiglu_ulp():
  """The MI355X SwiGLU kernels reach ulp = 1.7 where the stand-in shows 0.5: plm_sigmoid (exp2 + rcp, 1 ulp each) flips the
  intermediate rounding s = bf16(silu(x)) on ~1e-4 of the elements, and a flipped s moves out = bf16(s z) by up to
  ulp(s) |z| < 2 ulp(out).  A stand-in whose sigmoid carries that error (2 fp32 ulps) reproduces it, inside the budget."""
  M, h = 333, 2048  # test_kernels_gpu.py::test_swiglu_fwd_bwd's inputs
  g = torch.Generator().manual_seed(h)
  u = (2 * torch.randn(M, 2 * h, generator=g)).to(BF16)
  x, z = u[:, :h].float(), u[:, h:].float()
  sig = E._sigmoid(x) * (1 + 2.0 ** -22)
  out = rb(rb(x * sig) * z).to(BF16)
  m = P.elementwise(out, P.swiglu_fwd_reference(u))
  print(f'swiglu with a 2-ulp sigmoid: ulp={m["ulp"]:.2f} neq={m["neq"]:.1e}')
  assert 1.0 < m['ulp'] < P.BOUNDS['ulp'] and m['neq'] <= P.BOUNDS['neq'] / 2


def test_nan_anywhere_is_rejected():
  """A NaN in any RMSNorm output (dw, dx, rstd) survives ``merge`` - Python's max(prev, nan) would drop it - and fails the
  budget; so does a NaN in a bf16 element-wise output."""
  x, w, br, dy, gin = P.rms_inputs(67, 260, 0, True)
  r, y, rstd = rms_fwd_standin(x, br, w, 1e-6)
  dx, dw = rms_bwd_standin(dy, r, w, rstd, gin)
  ref_y, ref_rstd = P.rmsnorm_fwd_reference(r, w, 1e-6)
  ref_dx, ref_dw, dw_scale = P.rmsnorm_bwd_reference(dy, r, w, rstd)
  assert not P.violations(P.merge(P.rmsnorm_fwd(y, rstd, ref_y, ref_rstd), P.rmsnorm_bwd(dx, dw, ref_dx, ref_dw, dw_scale, gin)))
  for name in ('dw', 'dx', 'rstd', 'y'):
    t = {'dw': dw, 'dx': dx, 'rstd': rstd, 'y': y}[name].clone()
    t.view(-1)[5] = float('nan')
    a = {'dw': dw, 'dx': dx, 'rstd': rstd, 'y': y}
    a[name] = t
    for order in (0, 1):  # the NaN metric first and last in the merge
      parts = [P.rmsnorm_fwd(a['y'], a['rstd'], ref_y, ref_rstd), P.rmsnorm_bwd(a['dx'], a['dw'], ref_dx, ref_dw, dw_scale, gin)]
      m = P.merge(*(parts if order else parts[::-1]))
      assert P.violations(m), (name, order, m)
  assert P.violations(P.merge({'rms_dw': 0.0}, {'rms_dw': float('nan')}, {'rms_dw': 1e-9}))
  assert P.violations(P.merge({'ulp': float('nan')}, {'ulp': 0.5}))
