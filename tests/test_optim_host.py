"""The reference's other optimizers (optim/init_optim.py:7-70) on the host: engine.intialize_optimizer's torch-side choices
(fused_optim False) against the reference's own trajectories (tests/golden/optimizers.npz, make_optimizers.py), the refusals,
and the per-element update the gfx950 kernels implement (plainlm_amd/csrc/optim.hip), restated in fp64 with the host scalars
of ops.nadam_scalars / ops.optim_hparams, against the same trajectories."""

import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from plainlm_amd import engine, ops
from plainlm_amd.optim import SignSGD

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'optimizers.npz')
N_DECAY = 3


@pytest.fixture(scope='module')
def gold():
  z = np.load(GOLDEN)
  return {k: z[k] for k in z.files}


def _cases(gold):
  return json.loads(str(gold['cases']))


def _inputs(gold):
  n = len([k for k in gold if k.startswith('init/')])
  init = [torch.from_numpy(gold[f'init/{k}']) for k in range(n)]
  grads = [[torch.from_numpy(gold[f'grad/{s}/{k}']) for k in range(n)] for s in range(len(gold['lrs']))]
  return init, grads


def _groups(params, wd):
  return [{'params': params[:N_DECAY], 'weight_decay': wd}, {'params': params[N_DECAY:], 'weight_decay': 0.0}]


def _ulps(a, b):
  """distance in units in the last place between two fp32 arrays"""
  ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
  ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
  ia = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia)
  ib = np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
  return np.abs(ia - ib)


def _check(case, got, want):
  if case['optim'] == 'nadamw':
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-9)
  else:
    assert _ulps(got, want).max() <= 1, (case['name'], np.abs(got - want).max())


def test_torch_side_optimizers_reproduce_the_reference(gold):
  init, grads = _inputs(gold)
  types = {'sgd': torch.optim.SGD, 'signSGD': SignSGD, 'nadamw': torch.optim.NAdam}
  for case in _cases(gold):
    cfg = SimpleNamespace(**{k: v for k, v in case.items() if k != 'name'})
    params = [torch.nn.Parameter(t.clone()) for t in init]
    opt = engine.intialize_optimizer(_groups(params, cfg.weight_decay), cfg, model=None)
    assert type(opt) is types[case['optim']], case['name']
    if case['optim'] == 'nadamw':
      assert opt.param_groups[0]['decoupled_weight_decay'] and opt.param_groups[0]['momentum_decay'] == 4e-3
    else:
      assert opt.param_groups[0]['momentum'] == cfg.beta1 and opt.param_groups[0]['dampening'] == cfg.dampening
    for s, step in enumerate(grads):
      for p, g in zip(params, step):
        p.grad = g.clone()
      torch.nn.utils.clip_grad_norm_(params, 1.0)
      for grp in opt.param_groups:
        grp['lr'] = float(gold['lrs'][s])
      opt.step()
      pre = f"{case['name']}/{s}"
      for k, p in enumerate(params):
        _check(case, p.detach().numpy(), gold[f'{pre}/p/{k}'])
      state = opt.state_dict()['state']
      want_keys = {key.split('/')[-1] for key in gold if key.startswith(f'{pre}/state/0/')}
      for k in range(len(params)):
        got = {n: v for n, v in state.get(k, {}).items() if torch.is_tensor(v)}
        assert set(got) == want_keys, (case['name'], k, set(got), want_keys)
        for n, v in got.items():
          _check(case, v.numpy(), gold[f'{pre}/state/{k}/{n}'])
    if case['name'] == 'sgd_plain':
      assert not opt.state_dict()['state'] and not want_keys  # torch keeps no momentum_buffer without momentum


def test_kernel_update_rule_reproduces_the_reference(gold):
  """optim.hip's per-element update with the host scalars it is launched with (ops.optim_hparams, ops.nadam_scalars), in fp64: the
  arithmetic the GPU tests then hold the kernels to, checked against the reference's trajectories on a machine without a GPU."""
  init, grads = _inputs(gold)
  for case in _cases(gold):
    ps = [t.double().clone() for t in init]
    ms = [None] * len(ps)
    vs = [torch.zeros_like(p) for p in ps]
    mu_product = [1.0, 1.0]
    for s, step in enumerate(grads):
      norm = torch.cat([g.double().reshape(-1) for g in step]).norm()
      clip = min(1.0, 1.0 / (float(norm) + 1e-6))
      lr = float(gold['lrs'][s])
      scal = {}
      if case['optim'] == 'nadamw':  # per group and step, as FlatNAdamW forms them
        for gi in (0, 1):
          *scal[gi], mu_product[gi] = ops.nadam_scalars(lr, case['beta1'], case['beta2'], 4e-3, s + 1, mu_product[gi])
      for k, (p, g) in enumerate(zip(ps, step)):
        gi = int(k >= N_DECAY)
        wd = case['weight_decay'] if gi == 0 else 0.0
        g = g.double() * clip
        if case['optim'] == 'nadamw':
          b1, b2 = case['beta1'], case['beta2']
          bc2, cg, cm = scal[gi]
          h = ops.optim_hparams('nadamw', lr, wd, beta1=b1, beta2=b2, eps=case['eps'], bc2=bc2, coef_grad=cg, coef_avg=cm)
          m = (ms[k] if ms[k] is not None else torch.zeros_like(p)) * h.beta1 + (1 - h.beta1) * g
          vs[k] = vs[k] * h.beta2 + (1 - h.beta2) * g * g
          d = (vs[k] / h.bc2).sqrt() + h.eps
          ps[k] = p * h.decay - h.coef_grad * g / d - h.coef_avg * m / d
        else:
          h = ops.optim_hparams(case['optim'], lr, wd, first=ms[k] is None, momentum=case['beta1'], dampening=case['dampening'])
          if case['optim'] == 'sgd':
            d = g + h.weight_decay * p
            if h.momentum == 0:
              ps[k] = p - h.lr * d
              continue
            m = d if h.first else h.momentum * ms[k] + (1 - h.dampening) * d
            ps[k] = p - h.lr * m
          else:
            m = h.momentum * (g if h.first else ms[k]) + (1 - h.dampening) * g
            ps[k] = p * h.decay - h.lr * torch.sign(m)
        ms[k] = m
      for k, p in enumerate(ps):
        want = torch.from_numpy(gold[f"{case['name']}/{s}/p/{k}"]).double()
        tol = 1e-5 * want.abs().max().item()  # fp64 against the reference's fp32: a few fp32 roundings per step
        assert (p - want).abs().max().item() <= tol, (case['name'], s, k)


def _cfg(**over):
  c = dict(optim='sgd', lr=1e-2, beta1=0.9, beta2=0.95, weight_decay=0.1, dampening=0.0, fused_optim=False)
  c.update(over)
  return SimpleNamespace(**c)


def test_refusals_name_the_problem():
  params = [torch.nn.Parameter(torch.zeros(4))]
  with pytest.raises(NotImplementedError, match='sfo_adamw'):
    engine.intialize_optimizer([{'params': params}], _cfg(optim='sfo_adamw'))
  with pytest.raises(NotImplementedError, match='lion'):
    engine.intialize_optimizer([{'params': params}], _cfg(optim='lion'))
  for name in ('sgd', 'signSGD'):
    cfg = _cfg(optim=name)
    del cfg.dampening
    with pytest.raises(ValueError, match='dampening'):
      engine.intialize_optimizer([{'params': params}], cfg)
  with pytest.raises(KeyError):
    ops.optim_hparams('lion', 1e-3)
