"""Schedule-free AdamW on the CPU: optim.AdamWScheduleFree (the y-only form the kernels also use) against an fp64 numpy oracle written
here in the paper's x / z form (Defazio et al. 2024, "The Road Less Scheduled"), the running-mean property of x, the train / eval
swaps, the state_dict round trip and the engine's optimizer selection.  When the schedulefree package happens to be importable, the
restatement is also compared with it."""

import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from plainlm_amd import optim as O
from plainlm_amd.engine import intialize_optimizer

B1, B2, EPS = 0.9, 0.95, 1e-8


class Oracle:
  """x / z form, one parameter group per entry of `groups`, everything in fp64:
  z <- z - lr (g_hat + wd y),  x <- (1 - c) x + c z,  y = (1 - b1) z + b1 x,  g_hat = g / (sqrt(v / bc2) + eps)."""

  def __init__(self, params, wds, warmup, r=0.0, power=2.0):
    self.x = [np.array(p, dtype=np.float64) for p in params]
    self.z = [x.copy() for x in self.x]
    self.v = [np.zeros_like(x) for x in self.x]
    self.wds, self.warmup, self.r, self.power = wds, warmup, r, power
    n = len(params)
    self.t, self.lr_max, self.wsum = [0] * n, [-1.0] * n, [0.0] * n

  def y(self, i):
    return (1 - B1) * self.z[i] + B1 * self.x[i]

  def step(self, grads, lrs):
    for i, (g, lr) in enumerate(zip(grads, lrs)):
      t = self.t[i] + 1  # 1-based step of this group
      lr_t = lr * min(1.0, t / self.warmup) if self.warmup else lr
      self.lr_max[i] = max(self.lr_max[i], lr_t)
      w = t ** self.r * self.lr_max[i] ** self.power
      self.wsum[i] += w
      c = w / self.wsum[i] if self.wsum[i] else 0.0
      y = self.y(i)
      self.v[i] = B2 * self.v[i] + (1 - B2) * g * g
      g_hat = g / (np.sqrt(self.v[i] / (1 - B2 ** t)) + EPS)
      self.z[i] = self.z[i] - lr_t * (g_hat + self.wds[i] * y)
      self.x[i] = (1 - c) * self.x[i] + c * self.z[i]
      self.t[i] = t


def _run(warmup, wds, clip, steps=24, seed=0):
  """the torch restatement (fp64 parameters) and the oracle on the same clipped gradients, two groups, lr set by a schedule each step,
  0 on step 0 (ckp1 = 0)"""
  rng = np.random.default_rng(seed)
  shapes = [(7, 5), (13,)]
  p0 = [rng.standard_normal(s) for s in shapes]
  params = [torch.nn.Parameter(torch.from_numpy(p.copy())) for p in p0]
  opt = O.AdamWScheduleFree([{'params': [params[0]], 'weight_decay': wds[0]}, {'params': [params[1]], 'weight_decay': wds[1]}],
                            lr=1e-2, betas=(B1, B2), eps=EPS, warmup_steps=warmup)
  ora = Oracle(p0, wds, warmup)
  for s in range(steps):
    lr = 0.0 if s == 0 else 1e-2 * (1.0 + 0.5 * np.sin(s))
    for grp in opt.param_groups:
      grp['lr'] = lr
    gs = [rng.standard_normal(sh) * (3.0 if s % 5 == 0 else 0.1) for sh in shapes]
    for p, g in zip(params, gs):
      p.grad = torch.from_numpy(g.copy())
    if clip:  # clip_grad_norm_ scales .grad in place, the oracle gets the same scaled gradients
      torch.nn.utils.clip_grad_norm_(params, clip)
      norm = np.sqrt(sum((g * g).sum() for g in gs))
      gs = [g * min(1.0, clip / (norm + 1e-6)) for g in gs]
    opt.step()
    ora.step(gs, [lr, lr])
    for i, p in enumerate(params):
      y = ora.y(i)
      err = np.abs(p.detach().numpy() - y).max() / np.abs(y).max()
      assert err < 1e-12, (s, i, err)
      zerr = np.abs(opt.state[p]['z'].numpy() - ora.z[i]).max() / np.abs(ora.z[i]).max()
      assert zerr < 1e-12, (s, i, zerr)
  return opt, params, ora


@pytest.mark.parametrize('warmup,wds,clip', [(0, (0.0, 0.0), None), (5, (0.1, 0.0), None), (5, (0.1, 0.3), 1.0), (3, (0.1, 0.0), 0.5)])
def test_restatement_matches_xz_oracle(warmup, wds, clip):
  opt, _, ora = _run(warmup, wds, clip)
  g = opt.param_groups[0]
  assert g['k'] == 24 and g['k'] == ora.t[0]
  assert g['weight_sum'] == pytest.approx(ora.wsum[0], rel=1e-12) and g['lr_max'] == pytest.approx(ora.lr_max[0], rel=1e-12)


def test_lr_zero_first_step_leaves_y_and_z():
  """lr = 0 on step 0: lr_max = 0, weight_sum = 0, ckp1 = 0 - y and z stay put, only exp_avg_sq moves"""
  p = torch.nn.Parameter(torch.randn(9, dtype=torch.float64))
  p0 = p.detach().clone()
  opt = O.AdamWScheduleFree([p], lr=0.0, betas=(B1, B2), weight_decay=0.1)
  p.grad = torch.randn(9, dtype=torch.float64)
  opt.step()
  g = opt.param_groups[0]
  assert g['weight_sum'] == 0.0 and g['lr_max'] == 0.0 and g['k'] == 1
  assert torch.equal(p.detach(), p0) and torch.equal(opt.state[p]['z'], p0)
  assert (opt.state[p]['exp_avg_sq'] > 0).all()


def test_x_is_running_mean_of_z():
  """warmup 0, constant lr, r = 0: every step has the same weight, so x = (y - (1 - b1) z) / b1 is the mean of z_1 .. z_t"""
  torch.manual_seed(0)
  p = torch.nn.Parameter(torch.randn(31, dtype=torch.float64))
  opt = O.AdamWScheduleFree([p], lr=3e-2, betas=(B1, B2), weight_decay=0.05)
  zs = []
  for _ in range(20):
    p.grad = torch.randn(31, dtype=torch.float64)
    opt.step()
    z = opt.state[p]['z']
    zs.append(z.clone())
    x = (p.detach() - (1 - B1) * z) / B1
    mean = torch.stack(zs).mean(0)
    assert (x - mean).abs().max().item() < 1e-12 * mean.abs().max().item() + 1e-14


def test_eval_train_swaps_and_step_in_eval_mode():
  torch.manual_seed(1)
  p = torch.nn.Parameter(torch.randn(1000))
  opt = O.AdamWScheduleFree([p], lr=1e-2, betas=(B1, B2), weight_decay=0.1, warmup_steps=2)
  p0 = p.detach().clone()
  opt.eval()  # before the first step: no state, nothing moves
  assert torch.equal(p.detach(), p0) and not opt.param_groups[0]['train_mode']
  with pytest.raises(RuntimeError, match='eval mode'):
    p.grad = torch.randn(1000)
    opt.step()
  opt.train()
  for _ in range(5):
    p.grad = torch.randn(1000)
    opt.step()
  y = p.detach().clone()
  z = opt.state[p]['z'].clone()
  opt.eval()
  x64 = (y.double() - (1 - B1) * z.double()) / B1
  assert (p.detach().double() - x64).abs().max().item() < 1e-6 * x64.abs().max().item()
  x = p.detach().clone()
  opt.eval()  # already in eval mode: a no-op
  assert torch.equal(p.detach(), x)
  with pytest.raises(RuntimeError, match='eval mode'):
    opt.step()
  opt.train()
  assert (p.detach() - y).abs().max().item() < 4e-7 * y.abs().max().item()
  opt.train()
  assert opt.param_groups[0]['train_mode']


def test_state_dict_round_trip():
  """state_dict carries the group keys and per-parameter z / exp_avg_sq; a fresh optimizer that loads it (from a checkpoint's
  copy, in eval mode) continues bit for bit"""
  opt, params, _ = _run(5, (0.1, 0.0), 1.0, steps=10, seed=3)
  opt.eval()
  sd = copy.deepcopy(opt.state_dict())
  for g in sd['param_groups']:
    assert {'k', 'weight_sum', 'lr_max', 'scheduled_lr', 'train_mode', 'warmup_steps', 'r', 'weight_lr_power'} <= set(g)
    assert g['train_mode'] is False and g['k'] == 10
  assert all(set(st) == {'z', 'exp_avg_sq'} for st in sd['state'].values())
  twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
  opt2 = O.AdamWScheduleFree([{'params': [twins[0]], 'weight_decay': 0.1}, {'params': [twins[1]], 'weight_decay': 0.0}], lr=1.0,
                             betas=(B1, B2), eps=EPS, warmup_steps=5)
  opt2.load_state_dict(sd)
  opt.train()
  opt2.train()
  rng = np.random.default_rng(9)
  for s in range(5):
    for p, q in zip(params, twins):
      g = torch.from_numpy(rng.standard_normal(tuple(p.shape)))
      p.grad, q.grad = g.clone(), g.clone()
    opt.step()
    opt2.step()
  for p, q in zip(params, twins):
    assert torch.equal(p.detach(), q.detach())
  assert opt.param_groups[1]['weight_sum'] == opt2.param_groups[1]['weight_sum']


def test_against_schedulefree_package_if_installed():
  sf = pytest.importorskip('schedulefree')
  torch.manual_seed(4)
  a = torch.nn.Parameter(torch.randn(64, dtype=torch.float64))
  b = torch.nn.Parameter(a.detach().clone())
  oa = O.AdamWScheduleFree([a], lr=1e-2, betas=(B1, B2), weight_decay=0.1, warmup_steps=3)
  ob = sf.AdamWScheduleFree([b], lr=1e-2, betas=(B1, B2), weight_decay=0.1, warmup_steps=3)
  ob.train()
  for _ in range(10):
    g = torch.randn(64, dtype=torch.float64)
    a.grad, b.grad = g.clone(), g.clone()
    oa.step()
    ob.step()
  assert torch.allclose(a.detach(), b.detach(), rtol=1e-12, atol=1e-14)
  oa.eval()
  ob.eval()
  assert torch.allclose(a.detach(), b.detach(), rtol=1e-12, atol=1e-14)


def _cfg(**over):
  c = dict(optim='sfo_adamw', fused_optim=False, lr=1e-3, beta1=0.9, beta2=0.95, weight_decay=0.1, warmup_steps=0.25, steps_budget=8)
  c.update(over)
  return SimpleNamespace(**c)


def test_engine_builds_sfo_adamw_and_names_missing_warmup_steps():
  params = [{'params': [torch.nn.Parameter(torch.zeros(4))], 'weight_decay': 0.1}]
  opt = intialize_optimizer(params, _cfg())
  assert type(opt) is O.AdamWScheduleFree and opt.param_groups[0]['warmup_steps'] == 2  # int(0.25 * 8), as the reference
  assert opt.param_groups[0]['eps'] == 1e-8 and opt.param_groups[0]['betas'] == (0.9, 0.95)
  params = [{'params': [torch.nn.Parameter(torch.zeros(4))], 'weight_decay': 0.1}]
  assert intialize_optimizer(params, _cfg(warmup_steps=3)).param_groups[0]['warmup_steps'] == 3
  cfg = _cfg()
  del cfg.warmup_steps
  with pytest.raises(ValueError, match="'warmup_steps'") as err:
    intialize_optimizer(params, cfg)
  assert isinstance(err.value, NotImplementedError) and 'sfo_adamw' in str(err.value)  # what such a config has always raised

