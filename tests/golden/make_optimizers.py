"""Trajectories of the reference's non-AdamW optimizers (optim/init_optim.py:7-70), frozen as data for tests/test_optim_host.py.

Small fp32 parameters in the reference's two weight-decay groups (0.1: a matrix, a vector and an odd-length vector; 0.0: two
vectors), 5 steps of fixed gradients (step 2 large enough that clip_grad_norm_(1.0) clips), a learning rate that changes between
steps.  Per step: p.grad = the step's gradient, clip_grad_norm_(params, 1.0), every group's lr set, optimizer.step(); then the
parameters and every tensor of the optimizer's state_dict are recorded.

sgd and signSGD come from the REFERENCE's own intialize_optimizer (imported in the build container).  Its nadamw branch passes
fused= to torch.optim.NAdam, which torch 2.10 refuses, so for nadamw the script builds torch.optim.NAdam with exactly the
reference's other arguments (lr, betas=[beta1, beta2], weight_decay, decoupled_weight_decay=True, eps).

Keys of optimizers.npz: 'cases' (JSON list of the configs), 'lrs' [5], 'init/<k>', 'grad/<t>/<k>' (k = parameter index in
param_groups order), '<case>/<t>/p/<k>' and '<case>/<t>/state/<k>/<name>' after step t (0-based).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_optimizers.py      (writes tests/golden/optimizers.npz)
"""
import json
import os
import sys
from types import SimpleNamespace

os.environ.setdefault('PYTHONDONTWRITEBYTECODE', '1')
sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _install_stubs  # noqa: E402

SHAPES = [(6, 5), (7,), (13,), (5,), (3,)]  # the first three decay (0.1), the last two do not
N_DECAY = 3
LRS = [1e-2, 2e-2, 1.5e-2, 5e-3, 1e-2]
CLIPPED_STEP = 2
COMMON = dict(lr=1e-2, beta2=0.95, weight_decay=0.1, eps=1e-8, fused_optim=False)
CASES = [
  dict(name='sgd_mom', optim='sgd', beta1=0.9, dampening=0.0),
  dict(name='sgd_mom_damp', optim='sgd', beta1=0.9, dampening=0.1),
  dict(name='sgd_plain', optim='sgd', beta1=0.0, dampening=0.0),
  dict(name='signsgd_mom', optim='signSGD', beta1=0.9, dampening=0.0),
  dict(name='signsgd_mom_damp', optim='signSGD', beta1=0.9, dampening=0.1),
  dict(name='nadamw', optim='nadamw', beta1=0.9, dampening=0.0),
]


def inputs():
  g = torch.Generator().manual_seed(2024)
  init = [torch.randn(s, generator=g) for s in SHAPES]
  grads = []
  for t in range(len(LRS)):
    scale = 5.0 if t == CLIPPED_STEP else 0.1
    step = [torch.randn(s, generator=g) * scale for s in SHAPES]
    step[1][3] = 0.0  # an exact zero gradient: sign(0) on signSGD's first step
    grads.append(step)
  return init, grads


def main():
  _install_stubs()
  sys.path.insert(0, REF)
  from optim import intialize_optimizer
  init, grads = inputs()
  out = {'cases': np.array(json.dumps([dict(COMMON, **c) for c in CASES])), 'lrs': np.array(LRS)}
  for k, t in enumerate(init):
    out[f'init/{k}'] = t.numpy()
  for s, step in enumerate(grads):
    for k, t in enumerate(step):
      out[f'grad/{s}/{k}'] = t.numpy()
  for case in CASES:
    cfg = SimpleNamespace(**COMMON, **{k: v for k, v in case.items() if k != 'name'})
    params = [torch.nn.Parameter(t.clone()) for t in init]
    groups = [{'params': params[:N_DECAY], 'weight_decay': cfg.weight_decay}, {'params': params[N_DECAY:], 'weight_decay': 0.0}]
    if cfg.optim == 'nadamw':
      opt = torch.optim.NAdam(groups, lr=cfg.lr, betas=[cfg.beta1, cfg.beta2], weight_decay=cfg.weight_decay,
                              decoupled_weight_decay=True, eps=getattr(cfg, 'eps', 1e-8))
    else:
      opt = intialize_optimizer(groups, cfg)
    for s, step in enumerate(grads):
      for p, g in zip(params, step):
        p.grad = g.clone()
      torch.nn.utils.clip_grad_norm_(params, 1.0)
      for grp in opt.param_groups:
        grp['lr'] = LRS[s]
      opt.step()
      for k, p in enumerate(params):
        out[f"{case['name']}/{s}/p/{k}"] = p.detach().numpy().copy()
      for k, st in opt.state_dict()['state'].items():
        for name, val in st.items():
          if torch.is_tensor(val):
            out[f"{case['name']}/{s}/state/{k}/{name}"] = val.detach().numpy().copy()
  np.savez_compressed(os.path.join(HERE, 'optimizers.npz'), **out)
  print('wrote', len(CASES), 'cases,', len(out), 'arrays')


if __name__ == '__main__':
  main()
