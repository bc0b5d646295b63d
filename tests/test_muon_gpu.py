"""Muon on a real MI355X (plainlm_amd/csrc/muon.hip): the batched NT GEMM against fp64 under oracle/parity_gemm's
allowance; prepare against torch; orthogonalize against an fp64 Newton-Schulz from the same X0, with torch's own bf16 iteration on the
device as the control that is held to the same assertion; the exact class of scaled partial permutations; FlatMuon against optim.Muon on
the small golden model; and the engine with optim: muon against its fused_optim: False twin, checkpoint included."""

import copy
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import muon_ref as MR  # noqa: E402
from oracle import parity_gemm as G  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope='module')
def P():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  import plainlm_amd
  return plainlm_amd


def relmax(a, ref):
  a, ref = a.double().cpu(), ref.double().cpu()
  return ((a - ref).abs().max() / ref.abs().max()).item()


# ---- the batched GEMM ------------------------------------------------------------------------------------------------------------------
MNK = ((64, 64, 64), (72, 136, 40), (200, 8, 24), (128, 128, 768))
PADLD = 8


def _padded(rows, cols, seed=None, cls='randn'):
  """bf16 [rows, cols] view of a [rows, cols + 8] buffer (every ld padded by 8); the pad holds NaN."""
  buf = torch.full((rows, cols + PADLD), float('nan'), dtype=BF16, device='cuda')
  v = buf[:, :cols]
  if seed is not None:
    v.copy_(G.operand(cls, rows, cols, seed, device='cuda'))
  return v


def _problems(mnk, with_d, with_ct, alpha, beta, seed):
  out = []
  for i, (M, N, K) in enumerate(mnk):
    A, B = _padded(M, K, seed + 3 * i), _padded(N, K, seed + 3 * i + 1)
    D = _padded(M, N, seed + 3 * i + 2) if with_d else None
    out.append((A, B, _padded(M, N), D, _padded(N, M) if with_ct else None, alpha, beta))
  return out


@pytest.mark.parametrize('with_d,alpha,beta', [(False, 1.0, 0.0), (False, 0.3, 0.0), (True, 2.0315, -4.775), (True, 1.0, 3.4445)])
def test_batched_gemm_against_fp64(P, with_d, alpha, beta):
  """One list mixing the four shapes, every ld padded by 8: each C under parity_gemm's budget against fp64 (the beta * D term enters the
  reference as the old C of an accumulating call does), Ct bit-equal to C^T, pads untouched, a second run bit-equal."""
  ops = P.ops
  probs = _problems(MNK, with_d, True, alpha, beta, 10)
  ops.gemm_nt_batched(probs)
  first = [(p[2].clone(), p[4].clone()) for p in probs]
  for (A, B, Cm, D, Ct, al, be), (M, N, K) in zip(probs, MNK):
    c0 = None if D is None else float(np.float32(be)) * D.double()
    R = G.reference(A, B, alpha=al, c0=c0)
    G.check(G.metrics(Cm, R, ((128, 128),)), f'nt_batched M{M} N{N} K{K} d={with_d} alpha={al} beta={be}')
    assert torch.equal(Ct, Cm.t()), (M, N, K)
    for t in (Cm, Ct):  # the pad columns behind the payload still hold their NaN
      pad = torch.as_strided(t, (t.shape[0], PADLD), (t.stride(0), 1), t.storage_offset() + t.shape[1])
      assert torch.isnan(pad).all(), (M, N, K)
  for p in probs:
    p[2].zero_()
    p[4].zero_()
  ops.gemm_nt_batched(probs)
  for p, (c, ct) in zip(probs, first):
    assert torch.equal(p[2], c) and torch.equal(p[4], ct)


@pytest.mark.parametrize('count', [1, 33])
def test_batched_gemm_list_lengths(P, count):
  """A list of one problem and one of NT_BATCH_GROUP + 1 (the group boundary is crossed: two launches): every problem bit-equal to
  the same problem run alone, with and without the optional operands in one list."""
  ops = P.ops
  assert ops.NT_BATCH_GROUP == 32
  mnk = [MNK[i % 3] for i in range(count)]
  probs = _problems(mnk, True, True, 0.7, -1.3, 50)
  probs = [(A, B, Cm, D if i % 2 == 0 else None, Ct if i % 3 != 1 else None, al, be) for i, (A, B, Cm, D, Ct, al, be) in enumerate(probs)]
  ops.gemm_nt_batched(probs)
  for i in (0, count - 1, count // 2):
    A, B, Cm, D, Ct, al, be = probs[i]
    alone = torch.empty_like(Cm)
    ops.gemm_nt_batched([(A, B, alone, D, None, al, be)])
    assert torch.equal(alone, Cm), i
    assert Ct is None or torch.equal(Ct, Cm.t()), i
    ref = al * (A.double() @ B.double().t()) + (0 if D is None else float(np.float32(be)) * D.double())
    assert relmax(Cm, ref) < 1e-2, i


# ---- prepare ---------------------------------------------------------------------------------------------------------------------------
def _prepare(ops, grads, bufs, momentum, nesterov, clip=None):
  table, shapes = ops.muon_items([(None, g, b, None, None) for g, b in zip(grads, bufs)])
  ws = ops.muon_workspace(shapes, 'cuda')
  nrm = torch.zeros(len(grads), device='cuda')
  ops.muon_prepare(table, shapes, momentum, nesterov, nrm, clip, workspace=ws)
  return ws, shapes, nrm


@pytest.mark.parametrize('nesterov', [True, False])
def test_prepare_against_torch(P, nesterov):
  """Two steps of the momentum update with a clip coefficient != 1 on a wide, a tall and a square matrix with ragged 64-tiles: the
  buffer against torch.lerp (relmax < 1e-6, as test_optim_gpu.py holds momentum buffers), nrm within one bf16 ulp of Ub.norm(), X0
  and X0^T bit-equal to bf16(float(Ub) / nrm) formed by torch from the kernel's own nrm; a second run from the same state bit-equal."""
  ops = P.ops
  gen = torch.Generator(device='cuda').manual_seed(3)
  shapes = [(72, 200), (200, 72), (128, 128)]
  bufs = [torch.zeros(s, device='cuda') for s in shapes]
  refs = [b.clone() for b in bufs]
  clip = torch.tensor([0.37], device='cuda')
  mu = 0.95
  for step in range(2):
    grads = [torch.randn(s, device='cuda', generator=gen) for s in shapes]
    before = [b.clone() for b in bufs]
    ws, shp, nrm = _prepare(ops, grads, bufs, mu, nesterov, clip)
    again = [b.clone() for b in before]
    ws2, _, nrm2 = _prepare(ops, grads, again, mu, nesterov, clip)
    assert torch.equal(nrm, nrm2) and all(torch.equal(a, b) for a, b in zip(again, bufs))
    for b1, b2 in zip(ops.muon_blocks(ws, shp), ops.muon_blocks(ws2, shp)):   # the blocks prepare writes (the others are uninitialised)
      assert torch.equal(b1['x0'], b2['x0']) and torch.equal(b1['x0t'], b2['x0t'])
    for i, (g, b, r, blk) in enumerate(zip(grads, bufs, refs, ops.muon_blocks(ws, shp))):
      gc = g * clip
      r.lerp_(gc, 1 - mu)
      assert relmax(b, r) < 1e-6, (step, i)
      u = gc.lerp(b, mu) if nesterov else b   # from the kernel's own buffer: the roundings below are then the kernel's alone
      ub = u.bfloat16()
      want = ub.norm().float().item()
      assert abs(nrm[i].item() - want) <= want * 2.0 ** -7, (step, i, nrm[i].item(), want)
      assert nrm[i].item() == nrm[i].bfloat16().float().item()
      x0 = (ub.float() / nrm[i]).bfloat16()
      wide = x0 if ub.shape[0] <= ub.shape[1] else x0.t()
      same = (blk['x0'] == wide)
      # u is re-formed here by torch from the kernel's buffer: where torch's lerp and the kernel's round u differently by one fp32 ulp
      # bf16(u) may flip, rarely; everything else is bit-equal
      assert same.float().mean().item() > 0.999, (step, i)
      assert torch.equal(blk['x0t'], blk['x0'].t()), (step, i)


def test_prepare_x0_is_bit_exact_from_its_own_ub(P):
  """momentum = 0 without Nesterov makes U the gradient itself (lerp(B, g, 1) = g exactly), so Ub is known bit for bit: X0 and X0^T are
  bit-equal to bf16(float(Ub) / nrm) formed by torch from the kernel's own nrm, on all three orientations."""
  ops = P.ops
  gen = torch.Generator(device='cuda').manual_seed(4)
  shapes = [(72, 200), (200, 72), (128, 128)]
  grads = [torch.randn(s, device='cuda', generator=gen) for s in shapes]
  bufs = [torch.randn(s, device='cuda', generator=gen) for s in shapes]
  ws, shp, nrm = _prepare(ops, grads, bufs, 0.0, False)
  for g, b, blk, nr in zip(grads, bufs, ops.muon_blocks(ws, shp), nrm):
    assert torch.equal(b, g)
    ub = g.bfloat16()
    x0 = (ub.float() / nr).bfloat16()
    wide = x0 if g.shape[0] <= g.shape[1] else x0.t()
    assert torch.equal(blk['x0'], wide) and torch.equal(blk['x0t'], wide.t())
    want = ub.norm().float().item()
    assert abs(nr.item() - want) <= want * 2.0 ** -7


def test_zero_gradient_on_a_zero_buffer(P):
  """X0 = 0, O = 0, no NaN anywhere, and W only decays (its shadows follow)."""
  ops = P.ops
  shapes = [(64, 96), (96, 64)]
  ps = [torch.randn(s, device='cuda') for s in shapes]
  p0 = [p.clone() for p in ps]
  items = [(p, torch.zeros_like(p), torch.zeros_like(p), torch.empty(s, dtype=BF16, device='cuda'),
            torch.empty((s[1], s[0]), dtype=BF16, device='cuda')) for p, s in zip(ps, shapes)]
  table, shp = ops.muon_items(items, lr_adj=[0.05, 0.05])
  ws = ops.muon_workspace(shp, 'cuda')
  nrm = torch.zeros(2, device='cuda')
  ops.muon_prepare(table, shp, 0.95, True, nrm, workspace=ws)
  ops.muon_orthogonalize(shp, 5, 'cuda', workspace=ws)
  ops.muon_apply(table, shp, 0.999, 5, 'cuda', workspace=ws)
  for blk, (p, g, b, dst, dst_t), q in zip(ops.muon_blocks(ws, shp, steps=5), items, p0):
    assert not blk['x0'].any() and not blk['o'].any() and not b.any()
    assert torch.equal(p, q * 0.999) and torch.isfinite(p).all()
    assert torch.equal(dst, p.bfloat16()) and torch.equal(dst_t, p.bfloat16().t())
  assert torch.equal(nrm, torch.full_like(nrm, 1e-7).bfloat16().float())


# ---- orthogonalize ---------------------------------------------------------------------------------------------------------------------
NS_SHAPES = ((64, 96), (96, 64), (128, 128), (96, 320), (768, 768))
MEASURED = {}  # tag -> (ours vs R, control vs R, ours vs control), relative Frobenius; printed by the test


def _ns_inputs():
  gen = torch.Generator(device='cuda').manual_seed(7)
  us = [torch.randn(s, device='cuda', generator=gen) for s in NS_SHAPES]
  scaled = torch.randn(96, 320, device='cuda', generator=gen) * torch.exp2(-torch.arange(96, device='cuda') % 9).float()[:, None]
  return us + [scaled], [f'{r}x{c}' for r, c in NS_SHAPES] + ['96x320 rows 2^(-8..0)']


def _orthogonalize(ops, us, steps=5):
  """O of every u through prepare (momentum 0, no Nesterov: U = u exactly) and orthogonalize, and each matrix's X0."""
  bufs = [torch.zeros_like(u) for u in us]
  ws, shp, _ = _prepare(ops, us, bufs, 0.0, False)
  x0 = [b['x0'].clone() for b in ops.muon_blocks(ws, shp)]
  ops.muon_orthogonalize(shp, steps, 'cuda', workspace=ws)
  blocks = ops.muon_blocks(ws, shp, steps=steps)
  return [b['o'].clone() for b in blocks], x0, blocks


def _held(ours, control, R, tag):
  """The one assertion both sides are held to: relative Frobenius error against R at most 1.5 x the control's own, measured in this
  run; and ours no farther from the control than the control is from R."""
  eo, ec, d = MR.rel_fro(ours, R), MR.rel_fro(control, R), ((ours.double() - control.double()).norm() / R.norm()).item()
  MEASURED[tag] = (eo, ec, d)
  print(f'muon_ns {tag}: ours-R {eo:.3e} control-R {ec:.3e} ours-control {d:.3e}')
  bound = 1.5 * ec
  assert ec <= bound and eo <= bound, (tag, eo, ec)
  assert d <= ec, (tag, d, ec)


def test_orthogonalize_against_fp64_with_torch_as_control(P):
  """Five Newton-Schulz steps on six matrices in one call (wide, tall, square, 768 x 768; unit-normal, and one with rows scaled by
  2^(-8..0)).  R = fp64 iteration from the kernel's X0; control C = torch.optim._muon._zeropower_via_newtonschulz on the device from
  the same matrix.  Bound: 1.5 x the control's error of this run (never our own); and |ours - C| <= |C - R|.  Two runs bit-equal;
  the tall result is stored in the weight's layout.
  Measured on MI355X: MEASURED_ON_MI355X below (worst ours / control 1.02, worst |ours - C| / |C - R| 0.88)."""
  from torch.optim._muon import _zeropower_via_newtonschulz
  ops = P.ops
  us, tags = _ns_inputs()
  outs, x0s, _ = _orthogonalize(ops, us)
  again, _, _ = _orthogonalize(ops, us)
  for u, o, o2, x0, tag in zip(us, outs, again, x0s, tags):
    assert torch.equal(o, o2), tag
    assert o.shape == u.shape and torch.isfinite(o.float()).all(), tag
    R = MR.ns_fp64(x0)
    R = R.t() if u.shape[0] > u.shape[1] else R
    control = _zeropower_via_newtonschulz(u, MR.COEFFS, 5, MR.EPS)
    _held(o, control, R, tag)


MEASURED_ON_MI355X = """relative Frobenius norms against R, five steps (ours - R, control - R, |ours - control| / |R|):
  64 x 96 1.406e-2 1.390e-2 2.5e-3 | 96 x 64 1.361e-2 1.361e-2 0 | 128 x 128 1.114e-2 1.131e-2 3.0e-3 | 96 x 320 1.157e-2 1.154e-2 1.4e-3 |
  768 x 768 0.985e-2 0.989e-2 5.8e-3 | 96 x 320 with rows scaled by 2^(-8..0) 0.999e-2 0.999e-2 0;
  FlatMuon's implied updates (8 weights x 3 steps): ours 1.01e-2 .. 1.27e-2, control 1.02e-2 .. 1.24e-2, |ours - control| 0.7e-3 .. 9.7e-3;
  the engine: |flat - twin| 3.8e-4 under the control-derived bound 2.7e-3."""


@pytest.mark.parametrize('rows,cols', [(64, 64), (64, 128), (128, 64)])
def test_exact_class_of_scaled_partial_permutations(P, rows, cols):
  """U = 0.37 P, P a 0/1 partial permutation: every product has one non-zero term, nothing depends on summation order.  Where P is 0,
  O is exactly 0 (a stray accumulation shows here); all non-zeros are bit-equal to one another, equal the scalar recurrence of the
  stated epilogue (muon_ref.scalar_chain) and lie within one bf16 ulp of 0.69140625; the tall result is the transpose of the wide one."""
  ops = P.ops
  Pm = MR.partial_permutation(rows, cols, seed=rows + cols).cuda()
  (o,), _, _ = _orthogonalize(ops, [0.37 * Pm])
  assert not o[Pm == 0].any()
  nz = o[Pm != 0].float()
  assert (nz == nz[0]).all()
  want = MR.scalar_chain(0.37, min(rows, cols))
  assert nz[0].item() == want, (nz[0].item(), want)
  assert abs(want - 0.69140625) <= 2.0 ** -8   # one bf16 ulp in [0.5, 1)
  if rows > cols:
    (wide,), _, _ = _orthogonalize(ops, [0.37 * Pm.t().contiguous()])
    assert torch.equal(o, wide.t())


# ---- FlatMuon against optim.Muon on the small model ---------------------------------------------------------------------------------------
def _small(P, mdl, main_grad=False):
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  m.load_state_dict({k[2:]: v for k, v in mdl.items() if k.startswith('w:')})
  m = m.cuda()
  if main_grad:
    m.enable_main_grad()
  return m


@pytest.fixture(scope='module')
def mdl(golden_dir):
  z = np.load(os.path.join(golden_dir, 'model.npz'))
  return {k: torch.from_numpy(z[k]) for k in z.files}


KW = dict(lr=3e-3, betas=[0.9, 0.95], eps=1e-8, weight_decay=0.1)


def _grads(gen, model, step):
  return [torch.randn(p.shape, device='cuda', generator=gen) * (5.0 if step == 0 else 0.01) for p in model.parameters()]


def _flat_run(P, mdl, steps=3):
  from plainlm_amd import optim
  m = _small(P, mdl, main_grad=True)
  opt = optim.FlatMuon(m, optim.muon_param_groups(m, P.get_param_groups(m, 0.1)), **KW)
  gen = torch.Generator(device='cuda').manual_seed(0)
  trail = []
  for step in range(steps):
    for p, grad in zip(m.parameters(), _grads(gen, m, step)):
      p.main_grad.copy_(grad)
    for grp in opt.param_groups:
      grp['lr'] = KW['lr'] * (step + 1) / 3
    old = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt.clip_and_step(1.0)
    trail.append((old, {n: p.detach().clone() for n, p in m.named_parameters()}))
  return m, opt, trail


def test_flat_muon_matches_the_torch_twin(P, mdl):
  """clip_and_step(1.0) against clip_grad_norm_ + optim.Muon over 3 steps with a changing lr (step 0 clips).  AdamW-part parameters
  and moments: relmax < 1e-5; momentum buffers < 1e-6; for every Muon weight and step the implied update (W_new - W_old decay) /
  (-lr_adj) of both sides is held to the orthogonalize assertion against an fp64 iteration from torch's X0 of the twin's U; the
  shadows equal bf16(W) and its transpose bit for bit; a second flat run gives the same bits; the state_dict has torch's keys."""
  from plainlm_amd import optim, ops
  m, opt, trail = _flat_run(P, mdl)
  ref = _small(P, mdl)
  ropt = optim.Muon(optim.muon_param_groups(ref, P.get_param_groups(ref, 0.1)), **KW)
  muon_names = {n for n, p in m.named_parameters() if any(p is q for q in opt.param_groups[0]['params'])}
  assert len(muon_names) == 8 and all(n.startswith('layers.') for n in muon_names)
  gen = torch.Generator(device='cuda').manual_seed(0)
  names = [n for n, _ in ref.named_parameters()]
  for step in range(3):
    for q, grad in zip(ref.parameters(), _grads(gen, ref, step)):
      q.grad = grad.clone()
    lr = KW['lr'] * (step + 1) / 3
    for grp in ropt.param_groups:
      grp['lr'] = lr
    torch.nn.utils.clip_grad_norm_(list(ref.parameters()), 1.0)
    told = {n: q.detach().clone() for n, q in ref.named_parameters()}
    ropt.step()
    old, new = trail[step]
    decay = 1 - lr * 0.1
    for n, q in ref.named_parameters():
      if n not in muon_names:
        continue
      st = ropt.state[q]
      u = q.grad.lerp(st['momentum_buffer'], 0.95)
      x0, _ = MR.x0_of(u)
      R = MR.ns_fp64(x0)
      R = R.t() if q.shape[0] > q.shape[1] else R
      lr_adj = ops.muon_adjusted_lr(lr, 'match_rms_adamw', *q.shape)
      ours = (new[n].double() - old[n].double() * decay) / -lr_adj
      control = (q.detach().double() - told[n].double() * decay) / -lr_adj
      _held(ours, control, R, f'flat step {step} {n}')
  for (n, p), q in zip(m.named_parameters(), ref.parameters()):
    mom, v = opt._views[id(p)]
    st = ropt.state[q]
    if n in muon_names:
      assert relmax(mom, st['momentum_buffer']) < 1e-6, n
    else:
      assert relmax(p.detach(), q.detach()) < 1e-5, n
      assert relmax(mom, st['exp_avg']) < 1e-5 and relmax(v, st['exp_avg_sq']) < 1e-5, n
  for lin in m.linear_modules():
    assert lin.stale_item() is None
    assert torch.equal(lin._shadow[0], lin.weight.detach().bfloat16())
    assert torch.equal(lin._shadow[1][:, :lin.out_features], lin.weight.detach().bfloat16().t())
  m2, opt2, _ = _flat_run(P, mdl)
  for (n, p), p2 in zip(m.named_parameters(), m2.parameters()):
    assert torch.equal(p.detach(), p2.detach()), n
  assert torch.equal(opt.flat_m, opt2.flat_m) and torch.equal(opt.flat_v, opt2.flat_v)
  sd = opt.state_dict()
  assert [g['use_muon'] for g in sd['param_groups']] == [True, False, False]
  keys = [set(sd['state'][i]) for g in sd['param_groups'] for i in g['params']]
  n_muon = len(sd['param_groups'][0]['params'])
  assert all(k == {'momentum_buffer'} for k in keys[:n_muon]) and all(k == {'step', 'exp_avg', 'exp_avg_sq'} for k in keys[n_muon:])
  assert names  # the twin saw the same parameter list


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
def _engine_cfg(**over):
  EC = dict(model='transformer', vocab_size=256, seq_len=64, d_model=128, expand='8/3', n_layers=2, n_heads=2,
            mlp_class='glu', tie_embeddings=False, torch_compile=False, micro_batch_size=1, grad_accumulation_steps=1,
            dtype='bfloat16', optim='muon', fused_optim=True, lr=3e-3, weight_decay=0.1, beta1=0.9, beta2=0.95, dampening=0.0,
            grad_clip=1.0, scheduler='warmup_cosine', warmup_steps=2, cooldown_steps=None, lr_start=0.0, lr_end=1e-5,
            lr_end_pct=None, steps_budget=8, resume=False, seed=100)
  EC.update(over)
  return namedtuple('Config', EC.keys())(**EC)


def _engine(P, mdl, cfg, ckpt=None):
  model, _ = P.construct_model(cfg)
  if ckpt is None:
    model.load_state_dict({k[2:]: v for k, v in mdl.items() if k.startswith('w:')})
  return P.TorchEngine(model, cfg, 'cuda', None, ckpt)


def test_engine_with_muon(P, mdl, golden_dir, monkeypatch):
  """HipEngine with optim: muon over 8 steps of the small model on one repeated batch: FlatMuon against its fused_optim: False twin (optim.Muon, torch's bf16
  matmuls on the device).  The loss falls on both.  The bound on their loss difference comes from two CONTROL runs that differ only in
  the Newton-Schulz summation order - the twin as it is, and the twin with muon_ref.ns_bf16 (exact sums, the same rounding points) in
  place of its matmuls - times 2.  A checkpoint after step 4 resumed by the flat engine continues bit-equal to the uninterrupted run."""
  from plainlm_amd import optim as O
  tokens = torch.from_numpy(np.load(os.path.join(golden_dir, 'engine.npz'))['tokens'])
  batch = lambda i: {'input_ids': tokens[0]}  # noqa: E731  (one batch, seen eight times: the loss must fall)
  eng = _engine(P, mdl, _engine_cfg())
  assert isinstance(eng.optimizer, O.FlatMuon)
  flat = [float(eng.step(batch(i))) for i in range(4)]
  ckpt = copy.deepcopy({'step': 4, 'state_dict': eng.model.state_dict(), 'optimizer': eng.optimizer.state_dict(),
                        'scheduler': eng.scheduler.state_dict(), 'scaler': eng.scaler.state_dict()})
  flat += [float(eng.step(batch(i))) for i in range(4, 8)]
  twin_eng = _engine(P, mdl, _engine_cfg(fused_optim=False))
  assert type(twin_eng.optimizer) is O.Muon
  twin = [float(twin_eng.step(batch(i))) for i in range(8)]

  def emulated(u, steps=5, coefficients=MR.COEFFS, eps=MR.EPS):
    x0, _ = MR.x0_of(u, eps)
    x = MR.ns_bf16(x0, steps, coefficients)
    return x.t() if u.size(0) > u.size(1) else x
  monkeypatch.setattr(O, 'newton_schulz', emulated)
  emu_eng = _engine(P, mdl, _engine_cfg(fused_optim=False))
  emu = [float(emu_eng.step(batch(i))) for i in range(8)]
  monkeypatch.undo()
  bound = 2.0 * max(abs(a - b) for a, b in zip(twin, emu))
  diff = max(abs(a - b) for a, b in zip(flat, twin))
  print(f'muon engine: flat {flat}\nmuon engine: twin {twin}\nmuon engine: emulated {emu}\nmuon engine: |flat - twin| {diff:.3e} bound {bound:.3e}')
  assert flat[-1] < flat[0] and twin[-1] < twin[0]
  assert diff <= bound, (diff, bound)
  eng2 = _engine(P, mdl, _engine_cfg(resume=True), ckpt=copy.deepcopy(ckpt))
  resumed = [float(eng2.step(batch(i))) for i in range(4, 8)]
  assert resumed == flat[4:], (resumed, flat[4:])
