"""Two ranks on ONE GPU with FlatSignSGD: the flat re-layout of a non-AdamW optimizer feeds ddp.GradReducer (model._grad_spans)
exactly as FlatAdamW's does.  As in tests/test_ddp_gpu.py the data plane is torch.distributed's gloo backend on the CUDA tensors
(RCCL refuses two ranks on one device, comm_backend='torch'); everything else is the production path.  signSGD is the strictest
optimizer for this check: a rank whose reduced gradient differed in one bit could move an element by 2 lr instead of not at all.
Two processes hold the GPU at a time."""

import os
import socket
from collections import namedtuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _free_port():
  with socket.socket() as s:
    s.bind(('127.0.0.1', 0))
    return s.getsockname()[1]


def _cfg():
  EC = dict(model='transformer', vocab_size=256, seq_len=64, d_model=128, expand='8/3', n_layers=2, n_heads=2,
            mlp_class='glu', tie_embeddings=False, torch_compile=False, micro_batch_size=1, grad_accumulation_steps=2,
            dtype='bfloat16', optim='signSGD', fused_optim=True, lr=1e-3, weight_decay=0.1, beta1=0.9, beta2=0.95, dampening=0.1,
            grad_clip=1.0, scheduler='warmup_cosine', warmup_steps=2, cooldown_steps=None, lr_start=1e-4, lr_end=1e-5,
            lr_end_pct=None, steps_budget=8, resume=False, seed=100)
  return namedtuple('Config', EC.keys())(**EC)


def _worker(rank, world, port, out_dir):
  import torch.distributed as dist
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
  dist.init_process_group('gloo', rank=rank, world_size=world)
  torch.cuda.set_device(0)
  import plainlm_amd as P
  from plainlm_amd.optim import FlatSignSGD
  z = np.load(os.path.join(GOLDEN, 'model.npz'))
  w = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')}
  if rank != 0:  # the constructor's broadcast must overwrite whatever the other ranks start from
    w = {k: v + 0.01 for k, v in w.items()}
  model, _ = P.construct_model(_cfg())
  model.load_state_dict(w)
  eng = P.TorchEngine(model, _cfg(), 'cuda:0', 0, None, comm_backend='torch', bucket_cap_mb=0.2)
  assert isinstance(eng.optimizer, FlatSignSGD) and len(eng.reducer.buckets) > 4
  tok = torch.from_numpy(np.load(os.path.join(GOLDEN, 'engine.npz'))['tokens'])
  losses = [eng.step({'input_ids': tok[k * world + rank]}).item() for k in range(6)]  # 3 optimizer windows of 2 micro-steps
  torch.cuda.synchronize()
  torch.save({'params': {n: p.detach().cpu().clone() for n, p in eng.model.named_parameters()}, 'losses': losses},
             os.path.join(out_dir, f'r{rank}.pt'))
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_flat_signsgd_keeps_ranks_identical(tmp_path):
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  import torch.multiprocessing as mp
  mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
  r0, r1 = (torch.load(tmp_path / f'r{r}.pt') for r in range(2))
  z = np.load(os.path.join(GOLDEN, 'model.npz'))
  moved = 0
  for n, p in r0['params'].items():
    assert torch.equal(p, r1['params'][n]), n
    moved += int(not torch.equal(p, torch.from_numpy(z['w:' + n])))
  assert moved == len(r0['params'])  # every tensor took its signSGD steps
  assert all(np.isfinite(r0['losses'] + r1['losses']))
