"""The AdamW / NAdamW / SGD / signSGD tails on MI355X (plainlm_amd/csrc/optim.hip): the flat kernel against the torch optimizers, the
shadow-emitting multi-tensor form against the flat kernel bit for bit, AdamW's bits against those of its former kernels, the argument
checks (all items of a list before its first launch), the flat optimizers on the small model
(clip, shadows, torch-layout state both ways) and the engine with each optimizer against its torch-side twin (fused_optim False),
checkpoints included."""

import copy
import importlib.util
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from plainlm_amd.optim import SignSGD  # noqa: E402

KINDS = ['adamw', 'nadamw', 'sgd', 'sgd0', 'signSGD']  # sgd0: SGD without momentum (no buffer)
HP = dict(lr=1e-2, wd=0.1, b1=0.9, b2=0.95, eps=1e-8, damp=0.1)


@pytest.fixture(scope='module')
def P():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  import plainlm_amd
  return plainlm_amd


def relmax(a, ref):
  a, ref = a.double().cpu(), ref.double().cpu()
  return ((a - ref).abs().max() / ref.abs().max()).item()


def _torch_opt(kind, params, lr=HP['lr'], wd=HP['wd']):
  if kind == 'adamw':
    return torch.optim.AdamW(params, lr=lr, betas=(HP['b1'], HP['b2']), eps=HP['eps'], weight_decay=wd)
  if kind == 'nadamw':
    return torch.optim.NAdam(params, lr=lr, betas=(HP['b1'], HP['b2']), eps=HP['eps'], weight_decay=wd, decoupled_weight_decay=True)
  if kind in ('sgd', 'sgd0'):
    return torch.optim.SGD(params, lr=lr, momentum=0.0 if kind == 'sgd0' else HP['b1'], dampening=HP['damp'], weight_decay=wd)
  return SignSGD(params, lr=lr, momentum=HP['b1'], dampening=HP['damp'], weight_decay=wd)


class _Kernel:
  """host side of one kernel trajectory: hyper-parameters per step as the flat optimizers form them"""

  def __init__(self, ops, kind):
    self.ops, self.kind, self.step, self.mu_product = ops, kind, 0, 1.0

  def hparams(self, lr, wd=HP['wd']):
    self.step += 1
    if self.kind == 'adamw':
      return self.ops.optim_hparams('adamw', lr, wd, beta1=HP['b1'], beta2=HP['b2'], eps=HP['eps'], bc1=1.0 - HP['b1'] ** self.step,
                                    bc2=1.0 - HP['b2'] ** self.step)
    if self.kind == 'nadamw':
      bc2, cg, cm, self.mu_product = self.ops.nadam_scalars(lr, HP['b1'], HP['b2'], 4e-3, self.step, self.mu_product)
      return self.ops.optim_hparams('nadamw', lr, wd, beta1=HP['b1'], beta2=HP['b2'], eps=HP['eps'], bc2=bc2, coef_grad=cg, coef_avg=cm)
    mom = 0.0 if self.kind == 'sgd0' else HP['b1']
    return self.ops.optim_hparams(self.kind.rstrip('0'), lr, wd, first=self.step == 1, momentum=mom, dampening=HP['damp'])

  def buffers(self, like):
    m = None if self.kind == 'sgd0' else torch.zeros_like(like)
    v = torch.zeros_like(like) if self.kind in ('adamw', 'nadamw') else None
    return m, v


@pytest.mark.parametrize('kind', KINDS)
def test_flat_kernel_matches_torch_optimizer(P, kind):
  """plm_optim_f32 on an odd length from the first step on, with a device clip coefficient != 1, against the torch optimizer on the
  same (clipped) gradients over 4 steps with a changing learning rate.  signSGD is exact but where |m| is within rounding of 0; there
  the two may disagree on the sign, i.e. by 2 lr, or by lr where one side's m is exactly 0 (each step re-starts from torch's state, so
  such elements do not accumulate)."""
  from plainlm_amd import ops
  n = 1_000_003
  gen = torch.Generator(device='cuda').manual_seed(1)
  p0 = torch.randn(n, device='cuda', generator=gen)
  ref = torch.nn.Parameter(p0.clone())
  topt = _torch_opt(kind, [ref])
  p = p0.clone()
  k = _Kernel(ops, kind)
  m, v = k.buffers(p)
  clip = torch.tensor([0.37], device='cuda')
  for s in range(4):
    lr = HP['lr'] * (1.0 + 0.5 * s)
    g = torch.randn(n, device='cuda', generator=gen)
    ops.optim_(k.hparams(lr), p, g, m, v, clip)
    ref.grad = g * clip
    for grp in topt.param_groups:
      grp['lr'] = lr
    topt.step()
    st = topt.state[ref]
    if kind == 'signSGD':
      off = p != ref.detach()
      frac = off.float().mean().item()
      assert frac < 1e-3, (s, frac)
      if off.any():
        d = (p - ref.detach())[off].abs()  # opposite signs: 2 lr; an m that rounded to exactly 0 on one side (sign 0): lr
        near = lambda x: (x - d).abs() <= 1e-4 * x  # noqa: E731
        assert (near(2 * lr) | near(lr)).all(), (s, d.min().item(), d.max().item())
        mr = st['m'][off].abs()
        assert (mr <= 1e-5 * st['m'].abs().max()).all(), (s, mr.max().item())
      assert relmax(m, st['m']) < 1e-6
      p.copy_(ref.detach())
      m.copy_(st['m'])
    else:
      assert relmax(p, ref.detach()) < 1e-5, s
      if kind in ('adamw', 'nadamw'):
        assert relmax(m, st['exp_avg']) < 1e-5 and relmax(v, st['exp_avg_sq']) < 1e-5, s
      elif kind == 'sgd':
        assert relmax(m, st['momentum_buffer']) < 1e-5, s
      else:
        assert 'momentum_buffer' not in st or st['momentum_buffer'] is None


def _items(shapes, kind, gen):
  """(p, g, m, v, dst, dst_t) per [rows, cols]; dst_t is [cols, ld_t] with padding columns set to a sentinel"""
  out = []
  for rows, cols, ld_t in shapes:
    p = torch.randn(rows, cols, device='cuda', generator=gen)
    g = torch.randn(rows, cols, device='cuda', generator=gen)
    m = None if kind == 'sgd0' else torch.randn(rows, cols, device='cuda', generator=gen) * 0.1
    v = torch.rand(rows, cols, device='cuda', generator=gen) * 0.01 if kind in ('adamw', 'nadamw') else None
    dst = torch.empty(rows, cols, dtype=torch.bfloat16, device='cuda')
    dst_t = torch.full((cols, ld_t), 7.0, dtype=torch.bfloat16, device='cuda')
    out.append((p, g, m, v, dst, dst_t))
  return out


@pytest.mark.parametrize('kind', KINDS)
def test_multi_tensor_form_equals_flat_kernel_and_writes_shadows(P, kind):
  """plm_optim_cast_multi over 60 items (two launches of at most 56), square and non-square, partial 64 x 64 tiles, ld_t > rows:
  p / m / v bit for bit as plm_optim_f32 leaves them, dst = bf16(p), dst_t[:, :rows] = bf16(p)^T, the padding columns untouched.
  Two steps: the first-step path and the steady one."""
  from plainlm_amd import ops
  gen = torch.Generator(device='cuda').manual_seed(2)
  base = [(64, 64, 64), (128, 72, 136), (40, 200, 48), (8, 8, 8), (200, 40, 256), (72, 128, 72)]
  shapes = [base[i % len(base)] for i in range(60)]
  items = _items(shapes, kind, gen)
  flat = [tuple(t.clone() if t is not None else None for t in it[:4]) for it in items]
  clip = torch.tensor([0.61], device='cuda')
  km, kf = _Kernel(ops, kind), _Kernel(ops, kind)
  table = None
  for s in range(2):
    lr = 3e-3 * (s + 1)
    table = ops.optim_cast_multi_(km.hparams(lr), items, clip, table)
    hf = kf.hparams(lr)
    for p, g, m, v in flat:
      ops.optim_(hf, p, g, m, v, clip)
    torch.cuda.synchronize()
    for i, ((p, g, m, v, dst, dst_t), (fp, _, fm, fv)) in enumerate(zip(items, flat)):
      rows = p.shape[0]
      assert torch.equal(p, fp), (s, i)
      if m is not None:
        assert torch.equal(m, fm), (s, i)
      if v is not None:
        assert torch.equal(v, fv), (s, i)
      assert torch.equal(dst, p.bfloat16()), (s, i)
      assert torch.equal(dst_t[:, :rows], p.bfloat16().t()), (s, i)
      assert (dst_t[:, rows:] == 7.0).all(), (s, i)


def test_bad_arguments_are_refused_before_any_launch(P):
  from plainlm_amd import ops
  gen = torch.Generator(device='cuda').manual_seed(3)
  hn = ops.optim_hparams('nadamw', 1e-3, 0.1, beta1=0.9, beta2=0.95, eps=1e-8, bc2=0.05, coef_grad=1e-3, coef_avg=1e-3)
  hs = ops.optim_hparams('sgd', 1e-3, 0.1, first=True, momentum=0.9)
  good = _items([(64, 64, 64)], 'nadamw', gen)[0]
  before = good[0].clone()
  bad_v = good[:3] + (None,) + good[4:]
  with pytest.raises(RuntimeError, match='item 1: nadamw needs v'):
    ops.optim_cast_multi_(hn, [good, bad_v])
  with pytest.raises(RuntimeError, match='sgd takes no v'):
    ops.optim_cast_multi_(hs, [good])
  with pytest.raises(RuntimeError, match='signSGD needs the momentum buffer m'):
    ops.optim_cast_multi_(ops.optim_hparams('signSGD', 1e-3), [good[:2] + (None, None) + good[4:]])
  buf = torch.zeros(64 * 64 + 1, device='cuda')
  mis = buf[1:].view(64, 64)  # 4 bytes off 16-byte alignment
  with pytest.raises(RuntimeError, match='item 1: pointers must be 16-byte aligned'):
    ops.optim_cast_multi_(hn, [good, (mis,) + good[1:]])
  ha = ops.optim_hparams('adamw', 1e-3, 0.1, beta1=0.9, beta2=0.95, eps=1e-8, bc1=0.1, bc2=0.05)
  with pytest.raises(RuntimeError, match='item 1: adamw needs v'):
    ops.optim_cast_multi_(ha, [good, bad_v])
  with pytest.raises(RuntimeError, match='item 1: adamw needs the momentum buffer m'):
    ops.optim_cast_multi_(ha, [good, good[:2] + (None,) + good[3:]])
  with pytest.raises(RuntimeError, match='adamw needs v'):
    ops.optim_(ha, good[0].view(-1), good[1].view(-1), good[2].view(-1), None)
  with pytest.raises(RuntimeError, match='adamw needs the momentum buffer m'):
    ops.optim_(ha, good[0].view(-1), good[1].view(-1), None, good[3].view(-1))
  with pytest.raises(RuntimeError, match='unknown optimizer kind 9'):
    ops.optim_cast_multi_(ops.optim_hparams(9, 1e-3), [good])
  with pytest.raises(RuntimeError, match='unknown optimizer kind 0'):
    ops.optim_(ops.optim_hparams(0, 1e-3), good[0].view(-1), good[1].view(-1), None, None)
  with pytest.raises(RuntimeError, match='nadamw needs v'):
    ops.optim_(hn, good[0].view(-1), good[1].view(-1), good[2].view(-1), None)
  torch.cuda.synchronize()
  assert torch.equal(good[0], before)  # the valid first item of each refused list was not updated


def test_bad_item_beyond_the_56th_leaves_the_first_56_untouched(P):
  """The C side launches once per 56 items; it validates the WHOLE list first.  Item 57 has 12 rows (not a multiple of 8): the call is
  refused on the host and the 56 valid items in front of it - a full first launch - keep their parameters, state and shadows, for
  plm_optim_cast_multi (AdamW) and for plm_cast_f32_bf16_t_multi."""
  from plainlm_amd import ops
  gen = torch.Generator(device='cuda').manual_seed(4)
  items = _items([(64, 64, 64)] * 56 + [(12, 8, 16)] + [(8, 8, 8)], 'adamw', gen)
  before = [tuple(t.clone() for t in it[:4]) for it in items]
  for it in items:
    it[4].fill_(3.0)
  ha = ops.optim_hparams('adamw', 1e-2, 0.1, beta1=0.9, beta2=0.95, eps=1e-8, bc1=0.1, bc2=0.05)
  with pytest.raises(RuntimeError, match='plm_optim_cast_multi: item 56: rows=12 cols=8 must be positive multiples of 8'):
    ops.optim_cast_multi_(ha, items)
  with pytest.raises(RuntimeError, match='plm_cast_f32_bf16_t_multi: item 56: rows=12 cols=8 must be positive multiples of 8'):
    ops.cast_bf16_t_multi([(it[0], it[4], it[5]) for it in items])
  torch.cuda.synchronize()
  for i, (it, old) in enumerate(zip(items, before)):
    for t, o in zip(it[:4], old):
      assert torch.equal(t, o), i
    assert (it[4] == 3.0).all() and (it[5] == 7.0).all(), i


def test_adamw_bits_are_those_of_the_separate_adamw_kernels(P, golden_dir):
  """AdamW as a kind of the plm_optim_* family against tests/golden/adamw_bits.npz, what plm_adamw_f32 / plm_adamw_cast_multi of the
  tree before (ABI 111) left on an MI355X (make_adamw_bits.py, whose seeded CPU inputs are rebuilt here): p, m, v and the shadows
  bit for bit - the flat form on 4099 elements over 3 steps, the multi-tensor form on three matrices with partial tiles and
  ld_t > rows over 2, with a device clip coefficient and a changing lr, at an ordinary hyper-parameter set and at lr = 0.826,
  wd = 0.71, where decay = fma(-lr, wd, 1) and lr / bc1 formed in fp32 differ from their double-then-round values."""
  from plainlm_amd import ops
  spec = importlib.util.spec_from_file_location('make_adamw_bits', os.path.join(golden_dir, 'make_adamw_bits.py'))
  G = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(G)
  z = np.load(os.path.join(golden_dir, 'adamw_bits.npz'))
  want = lambda key: torch.from_numpy(z[key])  # noqa: E731
  bits = lambda t: t.view(torch.int16).cpu()  # noqa: E731

  def hparams(hp, t):
    return ops.optim_hparams('adamw', G.step_lr(hp, t), hp['wd'], beta1=hp['b1'], beta2=hp['b2'], eps=hp['eps'], bc1=1.0 - hp['b1'] ** t,
                             bc2=1.0 - hp['b2'] ** t)

  for name, hp in G.SETS.items():
    p0, gs = G.flat_inputs()
    p, m, v = p0.cuda(), torch.zeros(G.FLAT_N, device='cuda'), torch.zeros(G.FLAT_N, device='cuda')
    clip = torch.tensor([G.FLAT_CLIP], device='cuda')
    for t in range(1, G.FLAT_STEPS + 1):
      ops.optim_(hparams(hp, t), p, gs[t - 1].cuda(), m, v, clip)
    for k, x in (('p', p), ('m', m), ('v', v)):
      assert torch.equal(x.cpu(), want(f'{name}/flat/{k}')), (name, 'flat', k)
    mats = [(p.cuda(), [g.cuda() for g in gs], m.cuda(), v.cuda(), torch.empty(p.shape, dtype=torch.bfloat16, device='cuda'),
             torch.full((p.shape[1], ld_t), 7.0, dtype=torch.bfloat16, device='cuda'))
            for (p, gs, m, v), (_, _, ld_t) in zip(G.multi_inputs(), G.MULTI_SHAPES)]
    clip = torch.tensor([G.MULTI_CLIP], device='cuda')
    for t in range(1, G.MULTI_STEPS + 1):
      ops.optim_cast_multi_(hparams(hp, t), [(p, gs[t - 1], m, v, dst, dst_t) for p, gs, m, v, dst, dst_t in mats], clip)
    for i, (p, _, m, v, dst, dst_t) in enumerate(mats):
      for k, x in (('p', p), ('m', m), ('v', v)):
        assert torch.equal(x.cpu(), want(f'{name}/multi/{i}/{k}')), (name, 'multi', i, k)
      assert torch.equal(bits(dst), want(f'{name}/multi/{i}/dst').view(torch.int16)), (name, i, 'dst')
      assert torch.equal(bits(dst_t), want(f'{name}/multi/{i}/dst_t').view(torch.int16)), (name, i, 'dst_t')


# ---- the flat optimizers on the small model ------------------------------------------------------------------------------------------
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


FLAT = {'nadamw': ('FlatNAdamW', dict(lr=3e-3, betas=[0.9, 0.95], eps=1e-8, weight_decay=0.1), {'step', 'mu_product', 'exp_avg', 'exp_avg_sq'}),
        'sgd': ('FlatSGD', dict(lr=3e-2, momentum=0.9, dampening=0.1, weight_decay=0.1), {'momentum_buffer'}),
        'signSGD': ('FlatSignSGD', dict(lr=1e-3, momentum=0.9, dampening=0.1, weight_decay=0.1), {'m'})}


def _torch_twin(name, params, kw):
  if name == 'nadamw':
    return torch.optim.NAdam(params, lr=kw['lr'], betas=tuple(kw['betas']), eps=kw['eps'], weight_decay=kw['weight_decay'],
                             decoupled_weight_decay=True)
  cls = torch.optim.SGD if name == 'sgd' else SignSGD
  return cls(params, lr=kw['lr'], momentum=kw['momentum'], dampening=kw['dampening'], weight_decay=kw['weight_decay'])


def _params_close(name, a, b, lr, what):
  if name == 'signSGD':  # sign flips of a near-zero momentum move ONE element by 2 lr
    frac = ((a.detach() - b.detach()).abs() > 0.5 * lr).float().mean().item()
    assert frac < 1e-3, (what, frac)
    assert (a.detach() - b.detach()).abs().max().item() <= 2 * lr * 5 + 1e-6, what
  else:
    assert relmax(a.detach(), b.detach()) < 2e-6, what


def _grads(gen, model, step):
  return [torch.randn(p.shape, device='cuda', generator=gen) * (5.0 if step == 0 else 0.01) for p in model.parameters()]


@pytest.mark.parametrize('name', list(FLAT))
def test_flat_optimizer_matches_torch_and_clip(P, mdl, name):
  """clip_and_step(1.0) against clip_grad_norm_ + the torch optimizer over 3 steps (step 0 clips), the shadows written by the
  update, PLM_ADAMW_SHADOWS=0 bit for bit, and the torch-layout state_dict: loaded into the torch optimizer and back, each side
  continues the other's trajectory."""
  from plainlm_amd import optim
  cls_name, kw, keys = FLAT[name]
  cls = getattr(optim, cls_name)
  lr = kw['lr']
  m = _small(P, mdl, main_grad=True)
  ref = _small(P, mdl)
  opt = cls(m, P.get_param_groups(m, 0.1), **kw)
  ropt = _torch_twin(name, P.get_param_groups(ref, 0.1), kw)
  gen = torch.Generator(device='cuda').manual_seed(0)
  for step in range(3):
    for p, q, grad in zip(m.parameters(), ref.parameters(), _grads(gen, m, step)):
      p.main_grad.copy_(grad)
      q.grad = grad.clone()
    for grp in opt.param_groups + ropt.param_groups:
      grp['lr'] = lr * (step + 1) / 3
    opt.clip_and_step(1.0)
    norm = torch.nn.utils.clip_grad_norm_(list(ref.parameters()), 1.0)
    ropt.step()
    assert abs(opt.last_grad_norm.item() - norm.item()) <= 1e-5 * norm.item()
  for (n, p), q in zip(m.named_parameters(), ref.parameters()):
    _params_close(name, p, q, lr, n)
  assert opt.emits_shadows
  for lin in m.linear_modules():
    assert lin.stale_item() is None
    assert torch.equal(lin._shadow[0], lin.weight.detach().bfloat16())
    assert torch.equal(lin._shadow[1][:, :lin.out_features], lin.weight.detach().bfloat16().t())
  # the flat kernel alone (no shadow emission): the same parameters bit for bit
  m2 = _small(P, mdl, main_grad=True)
  os.environ['PLM_ADAMW_SHADOWS'] = '0'
  try:
    opt2 = cls(m2, P.get_param_groups(m2, 0.1), **kw)
  finally:
    del os.environ['PLM_ADAMW_SHADOWS']
  assert not opt2.emits_shadows
  gen2 = torch.Generator(device='cuda').manual_seed(0)
  for step in range(3):
    for p, grad in zip(m2.parameters(), _grads(gen2, m2, step)):
      p.main_grad.copy_(grad)
    for grp in opt2.param_groups:
      grp['lr'] = lr * (step + 1) / 3
    opt2.clip_and_step(1.0)
  for (n, p), p2 in zip(m.named_parameters(), m2.parameters()):
    assert torch.equal(p.detach(), p2.detach()), n
  assert all(lin.stale_item() is not None for lin in m2.linear_modules())
  # torch's layout; flat -> torch, one step on each side from the same state
  sd = opt.state_dict()
  assert len(sd['state']) == 15 and all(set(st) == keys for st in sd['state'].values())
  ref2 = _small(P, mdl)
  with torch.no_grad():
    for q, p in zip(ref2.parameters(), m.parameters()):
      q.copy_(p)
  topt = _torch_twin(name, P.get_param_groups(ref2, 0.1), kw)
  topt.load_state_dict(copy.deepcopy(sd))  # a checkpoint file's copy, not views of the flat buffers
  for p, q, grad in zip(m.parameters(), ref2.parameters(), _grads(gen, m, 3)):
    p.main_grad.copy_(grad)
    q.grad = grad.clone()
  opt.clip_and_step(1.0)
  torch.nn.utils.clip_grad_norm_(list(ref2.parameters()), 1.0)
  topt.step()
  for (n, p), q in zip(m.named_parameters(), ref2.parameters()):
    _params_close(name, p, q, lr, 'flat->torch ' + n)
  # torch -> flat: a fresh flat optimizer on torch's parameters and state continues like torch
  m3 = _small(P, mdl, main_grad=True)
  with torch.no_grad():
    for p3, q in zip(m3.parameters(), ref2.parameters()):
      p3.copy_(q)
  opt3 = cls(m3, P.get_param_groups(m3, 0.1), **kw)
  opt3.load_state_dict(copy.deepcopy(topt.state_dict()))
  if name == 'nadamw':
    assert opt3._step_count == 4 and abs(opt3._mu_product[0] - opt._mu_product[0]) <= 1e-6
  for p3, q, grad in zip(m3.parameters(), ref2.parameters(), _grads(gen, m3, 4)):
    p3.main_grad.copy_(grad)
    q.grad = grad.clone()
  opt3.clip_and_step(1.0)
  torch.nn.utils.clip_grad_norm_(list(ref2.parameters()), 1.0)
  topt.step()
  for (n, p3), q in zip(m3.named_parameters(), ref2.parameters()):
    _params_close(name, p3, q, lr, 'torch->flat ' + n)


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
ENGINE = {'nadamw': dict(optim='nadamw', lr=3e-3), 'sgd': dict(optim='sgd', lr=5e-2, dampening=0.1),
          'signSGD': dict(optim='signSGD', lr=1e-3, dampening=0.1)}


def _engine_cfg(**over):
  EC = dict(model='transformer', vocab_size=256, seq_len=64, d_model=128, expand='8/3', n_layers=2, n_heads=2,
            mlp_class='glu', tie_embeddings=False, torch_compile=False, micro_batch_size=1, grad_accumulation_steps=2,
            dtype='bfloat16', optim='adamw', fused_optim=True, lr=3e-3, weight_decay=0.1, beta1=0.9, beta2=0.95, dampening=0.0,
            grad_clip=1.0, scheduler='warmup_cosine', warmup_steps=2, cooldown_steps=None, lr_start=0.0, lr_end=1e-5,
            lr_end_pct=None, steps_budget=8, resume=False, seed=100)
  EC.update(over)
  return namedtuple('Config', EC.keys())(**EC)


@pytest.mark.parametrize('name', list(ENGINE))
def test_engine_with_each_optimizer(P, mdl, golden_dir, name):
  """HipEngine with optim nadamw / sgd / signSGD, accumulation 2, clip 1.0, warmup-cosine: the fused tail (flat optimizer) against
  the torch one (fused_optim False) over 5 optimizer steps - identical losses in the first window, within 2e-4 afterwards (the
  tolerance argued in test_engine_options_fused_optimizer_equals_torch_adamw), parameters within an lr-scaled bound - and a
  checkpoint after step 3 that resumes under the same engine and under the torch optimizer."""
  tokens = torch.from_numpy(np.load(os.path.join(golden_dir, 'engine.npz'))['tokens'])
  batch = lambda i: {'input_ids': tokens[i % tokens.shape[0]]}  # noqa: E731
  opts = ENGINE[name]
  from plainlm_amd import optim as O
  expect = {'nadamw': O.FlatNAdamW, 'sgd': O.FlatSGD, 'signSGD': O.FlatSignSGD}[name]
  ckpt_at = 6  # micro-steps: after 3 optimizer steps
  runs = {}
  for fused in (True, False):
    cfg = _engine_cfg(fused_optim=fused, **opts)
    model, _ = P.construct_model(cfg)
    model.load_state_dict({k[2:]: v for k, v in mdl.items() if k.startswith('w:')})
    eng = P.TorchEngine(model, cfg, 'cuda', None, None)
    assert isinstance(eng.optimizer, expect) == fused
    losses = [float(eng.step(batch(i))) for i in range(10)]
    runs[fused] = (losses, {n: p.detach().float().cpu() for n, p in eng.model.named_parameters()})
  (lf, pf), (lt, pt) = runs[True], runs[False]
  assert lf[:2] == lt[:2], (lf[:2], lt[:2])
  np.testing.assert_allclose(lf, lt, rtol=2e-4)
  lr = opts['lr']
  for n in pf:
    frac_off = ((pf[n] - pt[n]).abs() > 0.5 * lr).float().mean().item()
    assert frac_off < 0.02, (n, frac_off)
  # checkpoint after 3 optimizer steps (the reference's recipe), resumed by the fused engine and by the torch one
  cfg = _engine_cfg(**opts)
  model, _ = P.construct_model(cfg)
  model.load_state_dict({k[2:]: v for k, v in mdl.items() if k.startswith('w:')})
  eng = P.TorchEngine(model, cfg, 'cuda', None, None)
  head = [float(eng.step(batch(i))) for i in range(ckpt_at)]
  assert head == lf[:ckpt_at]
  ckpt = copy.deepcopy({'step': ckpt_at // 2, 'state_dict': eng.model.state_dict(), 'optimizer': eng.optimizer.state_dict(),
                        'scheduler': eng.scheduler.state_dict(), 'scaler': eng.scaler.state_dict()})
  tail = [float(eng.step(batch(i))) for i in range(ckpt_at, 10)]
  for fused in (True, False):
    cfg = _engine_cfg(fused_optim=fused, resume=True, **opts)
    model, _ = P.construct_model(cfg)
    eng2 = P.TorchEngine(model, cfg, 'cuda', None, copy.deepcopy(ckpt))
    assert isinstance(eng2.optimizer, expect) == fused
    resumed = [float(eng2.step(batch(i))) for i in range(ckpt_at, 10)]
    if fused and name != 'nadamw':
      assert resumed == tail, (resumed, tail)
    elif fused:  # mu_product travels as torch's fp32 scalar, the flat optimizer keeps it in fp64
      np.testing.assert_allclose(resumed, tail, rtol=1e-6)
    else:
      np.testing.assert_allclose(resumed, tail, rtol=2e-4)
