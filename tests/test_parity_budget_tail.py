"""The budget of the step's tail (oracle/parity_tail.py) against planted defects, on the CPU.

``standin`` restates optim_elem (plainlm_amd/csrc/optim.hip) in fp32 torch, rounding where the kernel rounds (an FMA is
formed in fp64 and rounded once more, which differs from a true FMA in rare double roundings: the stand-in is measured by
the budget, never compared bit for bit).  Each defect is a one-line edit of it.  The budget must ACCEPT every stand-in on
every input class, first step and steady, with and without clip, and REJECT every defect by at least 2x its bound on at
least one class; what the older criterion (max|a - ref| / max|ref| < 1e-5 on unit-normal data) says to each defect is
measured and asserted as measured.  The reductions get plain-Python models of who adds which element, with defects the
exact-sum inputs reject by != and the older tolerance accepts.  Nothing here launches a kernel."""

import numpy as np
import pytest
import torch

from oracle import parity_tail as PT

N = 4099
F32 = torch.float32


def f32(x):
  return float(np.float32(x))


def fma(a, b, c):
  """fl32(a * b + c): the product is exact in fp64, the sum rounded to fp64 and then to fp32."""
  a = a.double() if torch.is_tensor(a) else a
  b = b.double() if torch.is_tensor(b) else b
  return (a * b + c.double()).float()


def relmax(got, ref):
  """The older tests' yardstick: max|got - ref| / max|ref|."""
  got, ref = got.double(), ref.double()
  return ((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)).item()


def lerp_standin(a, b, w, defect=None):
  d = b - a
  if abs(w) < 0.5 or defect == 'one_sided_lerp':
    return fma(w, d, a)
  return fma(-d, f32(1.0 - np.float32(w)), b)


def standin(kind, hp, p, g, m, v, clip, defect=None):
  """(p', m', v') of optim_elem<kind> in fp32; None for the buffers the kind does not have."""
  h = PT.fields(hp)
  first = bool(h['first'])
  if defect == 'first_ignored':
    first = False
  cs = 1.0 if clip is None else f32(clip)
  gi = g * cs
  b1, b2, eps, lr, wd = h['beta1'], h['beta2'], h['eps'], h['lr'], h['weight_decay']
  omb1, omb2, omd = f32(np.float32(1) - np.float32(b1)), f32(np.float32(1) - np.float32(b2)), f32(np.float32(1) - np.float32(h['dampening']))
  if kind in ('adamw', 'nadamw'):
    mi = fma(b1, m, omb1 * gi)
    gv = g if defect == 'v_unclipped' else gi
    vi = fma(b2, v, (omb2 * gv) * gv)
    pd = p * h['decay']
    if kind == 'adamw':
      d = vi.sqrt() / h['bc2'] + eps
      if defect == 'eps_inside':
        d = (vi.sqrt() + eps) / h['bc2']
      if defect == 'nadam_denominator':          # NAdamW's sqrt(v / bc2) with AdamW's (already rooted) bc2
        d = (vi / h['bc2']).sqrt() + eps
      if defect == 'decay_after':
        return fma(-h['coef_avg'], mi / d, p) * h['decay'], mi, vi
      return fma(-h['coef_avg'], mi / d, pd), mi, vi
    d = (vi / h['bc2']).sqrt() + eps
    inner = pd if defect == 'coef_grad_dropped' else fma(-h['coef_grad'], gi / d, pd)
    return fma(-h['coef_avg'], mi / d, inner), mi, vi
  if kind in ('sgd', 'sgd0'):
    d = fma(wd, p, gi)
    if kind == 'sgd0':
      return fma(-lr, d, p), None, None
    mi = d if first else fma(omd, d, h['momentum'] * m)
    return fma(-lr, mi, p), mi, None
  if kind == 'sfo_adamw':
    z = p if first else m
    v0 = torch.zeros_like(p) if first else v
    vi = fma(b2, v0, (omb2 * gi) * gi)
    d = (vi / h['bc2']).sqrt() + eps
    gn = fma(wd, p, gi / d)
    return fma(h['coef_y'], gn, lerp_standin(p, z, h['ckp1'], defect)), fma(-lr, gn, z), vi
  pd = p * h['decay']
  m0 = gi if first else m
  mi = fma(omd, gi, h['momentum'] * m0)
  if defect == 'first_m_is_g' and first:
    mi = gi
  return fma(-lr, torch.sign(mi), pd), mi, None


def run(kind, cls, first, clip, defect=None, seed=0):
  """metrics of the stand-in (with ``defect``) on one case, and the fp64 reference's own tensors"""
  p, g, m, v = PT.optim_inputs(cls, N, seed + 17 * PT.CLASSES.index(cls))
  if first and kind in ('adamw', 'nadamw'):
    m, v = torch.zeros_like(m), torch.zeros_like(v)
  hp = PT.tail_hparams(kind, first)
  ref = PT.optim_reference(kind, hp, p, g, m, v, clip)
  got = standin(kind, hp, p, g, m, v, clip, defect)
  return PT.optim_metrics(ref, *got), ref, got


CASES = [(k, c, f, cl) for k in PT.KINDS for c in PT.CLASSES for f in (True, False) for cl in (None, PT.CLIP)]


def test_fl32_rounds_once():
  """optim_prepared()'s decay on the pair its comment names: fma(-lr, wd, 1) = 0.41354004, the double-rounded host value 0.41354001"""
  lr, wd = f32(0.826), f32(0.71)
  one = PT.fl32(1 - PT.Fraction(lr) * PT.Fraction(wd))
  assert one == float(np.float32(fma(torch.tensor(-lr, dtype=F32), torch.tensor(wd, dtype=F32), torch.tensor(1.0, dtype=F32)).item()))
  for x in (0.1, 1.0 / 3, 1e-8, 123456.789, 2.0 ** -24 + 2.0 ** -50):
    assert PT.fl32(PT.Fraction(x)) == f32(x) and PT.fl32(-PT.Fraction(x)) == -f32(x)


def test_standins_are_inside_the_budget():
  """every kind x class x {first, steady} x {no clip, clip}: the worst value per (kind, output) is printed (the honest floor of
  profiles/tail_parity.md) and is at most half its bound"""
  worst = {}
  for kind, cls, first, clip in CASES:
    met, _, _ = run(kind, cls, first, clip)
    assert not PT.violations(kind, met), (kind, cls, first, clip, met)
    for k, x in met.items():
      key = (kind, k, cls)
      worst[key] = max(worst.get(key, 0.0), x)
  for kind in PT.KINDS:
    for out in ('p', 'm', 'v', 'excl'):
      row = {c: worst[(kind, out, c)] for c in PT.CLASSES if (kind, out, c) in worst}
      if row:
        print(f'stand-in floor {kind:9s} {out:4s} ' + ' '.join(f'{c}={x:.3g}' for c, x in row.items()))
        top = max(row.values())
        if out == 'excl':
          assert top <= 1e-4, (kind, row)          # the fp64 reference alone leaves out at most 1e-4 on every class
        else:
          assert 2 * top <= PT.BOUNDS_TAIL[(kind, out)], (kind, out, top)


# (defect, kind, first step?, the metric meant to catch it, passes the older criterion on randn?)
DEFECTS = [
    ('eps_inside', 'adamw', False, 'p', True),
    ('decay_after', 'adamw', False, 'p', False),
    ('v_unclipped', 'adamw', False, 'v', False),
    ('nadam_denominator', 'adamw', False, 'p', False),
    ('first_ignored', 'sgd', True, 'm', False),
    ('first_ignored', 'signSGD', True, 'm', False),
    ('first_m_is_g', 'signSGD', True, 'm', False),
    ('coef_grad_dropped', 'nadamw', False, 'p', False),
]


def _old_criterion(kind, first, defect):
  """the older tests' check of this step on unit-normal data with the device clip: relmax of p, m, v against fp64"""
  _, ref, got = run(kind, 'randn', first, PT.CLIP, defect)
  vals = [relmax(x, ref[k][0]) for k, x in zip('pmv', got) if x is not None]
  return max(vals)


@pytest.mark.parametrize('defect,kind,first,metric,old_passes', DEFECTS)
def test_planted_defect_is_rejected(defect, kind, first, metric, old_passes):
  """each defect exceeds the bound of the metric meant to catch it by at least 2x on at least one class (with clip, so that
  'unclipped' means something); its value under the older criterion is measured and asserted as it falls"""
  per_class = {}
  for cls in PT.CLASSES:
    met, _, _ = run(kind, cls, first, PT.CLIP, defect)
    per_class[cls] = met[metric]
  bound = PT.BOUNDS_TAIL[(kind, metric)]
  old = _old_criterion(kind, first, defect)
  print(f'defect {defect:18s} {kind:9s} {metric}: ' + ' '.join(f'{c}={x:.3g}' for c, x in per_class.items()) +
        f' | bound {bound:g} | present relmax on randn {old:.3g} ({"passes" if old < 1e-5 else "fails"} 1e-5)')
  assert max(per_class.values()) >= 2 * bound, per_class
  assert (old < 1e-5) == old_passes, old


def test_eps_defect_in_numbers():
  """eps inside the division by sqrt(bc2) reads 1e-7 under the present criterion (100x inside 1e-5); at element level it is several
  times the honest stand-in on unit-normal data (v = 0.01 rand here: sqrt(v) >> eps) and > 1e5 roundoffs once sqrt(v) is comparable
  to eps or the magnitudes spread over decades"""
  old = _old_criterion('adamw', False, 'eps_inside')
  rn, _, _ = run('adamw', 'randn', False, PT.CLIP, 'eps_inside')
  tg, _, _ = run('adamw', 'tiny_g', False, PT.CLIP, 'eps_inside')
  print(f'eps_inside: relmax {old:.3g}, p metric randn {rn["p"]:.3g}, tiny_g {tg["p"]:.3g}')
  mx, _, _ = run('adamw', 'mixed', False, PT.CLIP, 'eps_inside')
  honest, _, _ = run('adamw', 'randn', False, PT.CLIP)
  print(f'eps_inside: honest randn {honest["p"]:.3g}, mixed {mx["p"]:.3g}')
  assert old < 1e-6 and rn['p'] > 3 * honest['p'] and tg['p'] > 1e5 and mx['p'] > 1e5


def test_one_sided_lerp_needs_the_exact_invariant():
  """torch.lerp's one-sided form a + w (b - a) for every w is off by rounding only: no budget can reject it (measured:
  inside the sfo_adamw bound on every class at ckp1 = 0.8), and the older criterion passes it.  What rejects it is the
  exact end point: lerp(p, z, 1) must return z bit for bit, which the one-sided form misses where |p| >> |z|."""
  hp = PT.tail_hparams('sfo_adamw', False)
  assert 0.5 <= hp.ckp1 < 1.0                       # the far-side branch
  worst = max(run('sfo_adamw', c, False, PT.CLIP, 'one_sided_lerp')[0]['p'] for c in PT.CLASSES)
  print(f'one_sided_lerp: worst p metric {worst:.3g} (bound {PT.BOUNDS_TAIL[("sfo_adamw", "p")]:g})')
  assert worst <= PT.BOUNDS_TAIL[('sfo_adamw', 'p')]
  p, _, z, _ = PT.optim_inputs('mixed', N, 5)
  assert torch.equal(lerp_standin(p, z, 1.0), z) and torch.equal(lerp_standin(p, z, 0.0), p)
  assert not torch.equal(lerp_standin(p, z, 1.0, 'one_sided_lerp'), z)


def test_clip_and_scaling_invariants_hold_on_the_standin():
  """the exact invariants the GPU test asserts, confirmed bit for bit on the stand-in: clip folded into g; and power-of-two
  scaling of (g, m, v) with eps = 0"""
  p, g, m, v = PT.optim_inputs('randn', N, 3)
  for kind in PT.KINDS:
    hp = PT.tail_hparams(kind, False)
    a = standin(kind, hp, p, g, m, v, 0.37)
    b = standin(kind, hp, p, g * f32(0.37), m, v, None)
    assert all(x is None or torch.equal(x, y) for x, y in zip(a, b)), kind
  for kind in ('adamw', 'nadamw'):
    hp = PT.tail_hparams(kind, False, eps=0.0)
    a = standin(kind, hp, p, g, m, v, None)
    b = standin(kind, hp, p, 4 * g, 4 * m, 16 * v, None)
    assert torch.equal(a[0], b[0]) and torch.equal(4 * a[1], b[1]) and torch.equal(16 * a[2], b[2]), kind
  hp = PT.tail_hparams('sfo_adamw', False, eps=0.0, wd=0.0)
  a = standin('sfo_adamw', hp, p, g, m, v, None)
  b = standin('sfo_adamw', hp, p, 4 * g, m, 16 * v, None)
  assert all(torch.equal(x, y) for x, y in zip(a[:2], b[:2])) and torch.equal(16 * a[2], b[2])
  hp = PT.tail_hparams('signSGD', False)
  assert torch.equal(standin('signSGD', hp, p, g, m, None, None)[0], standin('signSGD', hp, p, 8 * g, 8 * m, None, None)[0])


def test_nan_in_any_output_fails_every_metric():
  for kind in PT.KINDS:
    met0, ref, got = run(kind, 'randn', False, None)
    for i, key in enumerate('pmv'):
      if got[i] is None:
        continue
      bad = [None if x is None else x.clone() for x in got]
      bad[i][7] = float('nan')
      met = PT.optim_metrics(ref, *bad)
      assert met[key] == float('inf') and PT.violations(kind, met), (kind, key, met)
      bad[i][7] = float('inf')
      assert PT.optim_metrics(ref, *bad)[key] == float('inf')


# ---------------------------------------------------------------------------------------------------------------------
# reductions: who adds which element
# ---------------------------------------------------------------------------------------------------------------------
def sumsq_model(n, defect=None):
  """count[i] = how often plm_sumsq_f32 adds x[i]^2: stage 1 (float4 body over min(2048, ceil(n / 4096)) blocks of 1024
  threads with a stride loop, the n % 4 tail in block 0) and stage 2 (one partial per block)."""
  nvec = n >> 2
  blocks = min(max(-(-(-(-n // 4)) // 1024), 1), 2048)
  count = np.zeros(n, np.int64)
  owner = np.zeros(n, np.int64)
  vec = np.arange(nvec)
  count[:4 * nvec] = 1
  owner[:4 * nvec] = np.repeat((vec % (blocks * 1024)) // 1024, 4)
  if defect != 'tail_dropped':
    count[4 * nvec:] = 1            # block 0, threads 0 .. n % 4 - 1
  if defect == 'last_partial_dropped':
    count[owner == blocks - 1] = 0
  return count


def colsum_model(rows, defect=None):
  """count[r] = how often one column's sum adds row r: 16 row groups, a 64-row main loop (r + 48 < rows), a 16-row remainder"""
  count = np.zeros(rows, np.int64)
  for gi in range(16):
    r = gi
    while r + 48 < rows:
      for k in (0, 16, 32, 48):
        count[r + k] += 1
      r += 64
    if defect == 'remainder_late':
      r += 16
    while r < rows:
      count[r] += 1
      r += 16
  return count


def mean_model(n, defect=None):
  """count[i] for plm_mean_f32: thread t of one 1024-thread block adds t, t + 1024, ..."""
  count = np.ones(n, np.int64)
  if defect == 'single_trip':
    count[1024:] = 0
  return count


SUMSQ_N = [1, 3, 4, 5, 4095, 4096, 4097, 4 * 1024 * 2048 - 1, 4 * 1024 * 2048, 4 * 1024 * 2048 + 5]
COLSUM_ROWS = [1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 1024]
MEAN_N = [1, 63, 64, 65, 1023, 1024, 1025, 32768, 65537]


def test_reduction_models_add_every_element_once():
  for n in SUMSQ_N:
    assert (sumsq_model(n) == 1).all(), n
  for rows in COLSUM_ROWS:
    assert (colsum_model(rows) == 1).all(), rows
  for n in MEAN_N:
    assert (mean_model(n) == 1).all()


def test_exact_sum_inputs_reject_the_reduction_defects():
  """every defect changes the exact result on the inputs of tests/test_tail_parity_gpu.py (!=), and the older test's allowance
  (1e-4 n on n = 1 000 003 unit-normal values) accepts the dropped tail"""
  for n in SUMSQ_N:
    x = PT.exact_sum_inputs(n, n, (-1.0, 0.0, 1.0)).double().numpy()
    assert (x * x).sum() < 2 ** 24
    for defect in ('tail_dropped', 'last_partial_dropped'):
      c = sumsq_model(n, defect)
      changed = (c != 1).any()
      # n = 4097: 1025 float4 slots make two blocks, but the 1024 whole vectors all sit in block 0 (and so does the tail): block 1 adds nothing
      assert changed == (n % 4 != 0 if defect == 'tail_dropped' else n != 4097), (n, defect)
      if changed:
        hit = [(c[i] != 1) for i in PT.onehot_indices(n)]   # a one-hot probe at a dropped index reads 0, not 1
        assert any(hit), (n, defect)
        if (x[c != 1] != 0).any():
          assert (c * x * x).sum() != (x * x).sum()
  for rows in COLSUM_ROWS:
    c = colsum_model(rows, 'remainder_late')
    changed = (c != 1).any()
    assert changed == (rows % 64 != 0), rows          # the first 16-row group of a non-empty remainder is lost
    if changed:
      # the probe: a single 1 per column at row col % rows; the widest case (768 columns) visits every row of all but the 1024-row case
      assert any(c[col % rows] != 1 for col in range(768)), rows
  assert any((mean_model(n, 'single_trip') != 1).any() for n in MEAN_N)
  # the older sumsq test: n = 1 000 003 unit-normal values, |got - ref| < 1e-4 n = 100
  g = torch.Generator().manual_seed(1)
  n = 1_000_003
  x = torch.randn(n, generator=g).double().numpy()
  c = sumsq_model(n, 'tail_dropped')
  assert (c == 0).sum() == 3 and abs((c * x * x).sum() - (x * x).sum()) < 1e-4 * n


def test_embedding_order_is_seen_bit_for_bit():
  """embed_bwd_sequential is the explicit fp32 loop; a swap of two tokens of one id changes its bits and stays inside the older
  tolerance (1e-6 max|ref| sqrt(M / 4)); against the rounded fp64 sum most elements differ, so the order really matters"""
  g = torch.Generator().manual_seed(11)
  M, V, d = 1025, 7, 8
  ids = torch.randint(-1, V + 1, (M,), generator=g)
  dout = torch.randn(M, d, generator=g)
  dW0 = torch.randn(V, d, generator=g)
  seq = PT.embed_bwd_sequential(ids, dout, dW0, V)
  loop = dW0.clone().numpy()
  for t in range(M):
    if 0 <= ids[t] < V:
      loop[ids[t]] = loop[ids[t]] + dout[t].numpy()
  assert np.array_equal(loop, seq.numpy())
  ok = (ids >= 0) & (ids < V)
  ref64 = dW0.double().index_add_(0, ids[ok], dout[ok].double())
  frac = (ref64.float() != seq).float().mean().item()
  print(f'sequential fp32 vs rounded fp64 sum: {frac:.2%} of the elements differ')
  assert frac > 0.5
  same = torch.nonzero(ids == 3).flatten()
  a, b = same[0].item(), same[-1].item()
  perm = torch.arange(M)
  perm[a], perm[b] = b, a
  swapped = PT.embed_bwd_sequential(ids[perm], dout[perm], dW0, V)
  assert not torch.equal(swapped, seq)
  err = (swapped.double() - ref64).abs().max().item()
  assert err <= 1e-6 * max(1.0, ref64.abs().max().item()) * max(1, M // 4) ** 0.5
