"""Schedule-free AdamW on MI355X (PLM_OPTIM_SFO_ADAMW and plm_lerp_f32 in plainlm_amd/csrc/optim.hip): the flat kernel against the torch
restatement optim.AdamWScheduleFree, the shadow-emitting multi-tensor form against the flat kernel bit for bit, the train / eval swap
against torch.lerp, the argument checks, FlatAdamWScheduleFree on the small model (clip, shadows, swaps, state both ways), the engine with
optim sfo_adamw (fused against torch, eval at x, checkpoints both ways) and two data-parallel ranks."""

import copy
import ctypes as C
import os
import socket
from collections import namedtuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from plainlm_amd.optim import AdamWScheduleFree  # noqa: E402

B1, B2, EPS, WD = 0.9, 0.95, 1e-8, 0.1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def P():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  import plainlm_amd
  return plainlm_amd


def relmax(a, ref):
  a, ref = a.double().cpu(), ref.double().cpu()
  return ((a - ref).abs().max() / ref.abs().max()).item()


def _group(lr, warmup=2):
  """the host side of one kernel trajectory: a parameter group dict with the package's keys, advanced by ops.sfo_scalars"""
  return dict(lr=lr, betas=(B1, B2), k=0, warmup_steps=warmup, r=0.0, weight_lr_power=2.0, lr_max=-1.0, weight_sum=0.0)


def _hparams(ops, grp, lr, first):
  grp['lr'] = lr
  lr_s, ckp1, bc2 = ops.sfo_scalars(grp)
  return ops.optim_hparams('sfo_adamw', lr_s, WD, first=first, beta1=B1, beta2=B2, eps=EPS, bc2=bc2, ckp1=ckp1)


@pytest.mark.parametrize('clip', [None, 0.37])
def test_flat_kernel_matches_torch_restatement(P, clip):
  """plm_optim_f32 (sfo_adamw) on an odd length from the first step on (z created inside the launch), warm-up over the first two steps,
  a changing learning rate, with and without a device clip coefficient, against AdamWScheduleFree on the same gradients over 5 steps:
  y, z and exp_avg_sq at NAdamW's tolerance"""
  from plainlm_amd import ops
  n = 1_000_003
  gen = torch.Generator(device='cuda').manual_seed(1)
  p0 = torch.randn(n, device='cuda', generator=gen)
  ref = torch.nn.Parameter(p0.clone())
  topt = AdamWScheduleFree([ref], lr=1e-2, betas=(B1, B2), eps=EPS, weight_decay=WD, warmup_steps=2)
  p = p0.clone()
  z = torch.full_like(p, float('nan'))  # the first step must not read z or v
  v = torch.full_like(p, float('nan'))
  grp = _group(1e-2)
  cl = torch.tensor([clip], device='cuda') if clip else None
  for s in range(5):
    lr = 1e-2 * (1.0 + 0.5 * s)
    g = torch.randn(n, device='cuda', generator=gen)
    ops.optim_(_hparams(ops, grp, lr, s == 0), p, g, z, v, cl)
    ref.grad = g * cl if clip else g.clone()
    topt.param_groups[0]['lr'] = lr
    topt.step()
    st = topt.state[ref]
    assert relmax(p, ref.detach()) < 1e-5, s
    assert relmax(z, st['z']) < 1e-5 and relmax(v, st['exp_avg_sq']) < 1e-5, s
  assert grp['k'] == topt.param_groups[0]['k'] == 5 and grp['weight_sum'] == topt.param_groups[0]['weight_sum']


def _items(shapes, gen):
  out = []
  for rows, cols, ld_t in shapes:
    p = torch.randn(rows, cols, device='cuda', generator=gen)
    g = torch.randn(rows, cols, device='cuda', generator=gen)
    z = torch.randn(rows, cols, device='cuda', generator=gen)
    v = torch.rand(rows, cols, device='cuda', generator=gen) * 0.01
    dst = torch.empty(rows, cols, dtype=torch.bfloat16, device='cuda')
    dst_t = torch.full((cols, ld_t), 7.0, dtype=torch.bfloat16, device='cuda')
    out.append((p, g, z, v, dst, dst_t))
  return out


def test_multi_tensor_form_equals_flat_kernel_and_writes_shadows(P):
  """plm_optim_cast_multi (sfo_adamw) over 60 items (two launches), partial tiles, ld_t > rows: y / z / v bit for bit as plm_optim_f32
  leaves them, dst = bf16(y), dst_t[:, :rows] = bf16(y)^T, padding columns untouched.  Three steps: the first (z = copy of y, ckp1 = 1:
  the far side of the lerp) and two steady ones."""
  from plainlm_amd import ops
  gen = torch.Generator(device='cuda').manual_seed(2)
  base = [(64, 64, 64), (128, 72, 136), (40, 200, 48), (8, 8, 8), (200, 40, 256), (72, 128, 72)]
  items = _items([base[i % len(base)] for i in range(60)], gen)
  flat = [tuple(t.clone() for t in it[:4]) for it in items]
  clip = torch.tensor([0.61], device='cuda')
  gm, gf = _group(3e-3, warmup=0), _group(3e-3, warmup=0)
  table = None
  for s in range(3):
    lr = 3e-3 * (s + 1)
    table = ops.optim_cast_multi_(_hparams(ops, gm, lr, s == 0), items, clip, table)
    hf = _hparams(ops, gf, lr, s == 0)
    for p, g, z, v in flat:
      ops.optim_(hf, p, g, z, v, clip)
    torch.cuda.synchronize()
    for i, ((p, g, z, v, dst, dst_t), (fp, _, fz, fv)) in enumerate(zip(items, flat)):
      rows = p.shape[0]
      assert torch.equal(p, fp) and torch.equal(z, fz) and torch.equal(v, fv), (s, i)
      assert torch.equal(dst, p.bfloat16()), (s, i)
      assert torch.equal(dst_t[:, :rows], p.bfloat16().t()), (s, i)
      assert (dst_t[:, rows:] == 7.0).all(), (s, i)
    if s == 0:  # ckp1 = 1, coef_y = -lr: y = y - lr gn = z, the same bits through both lerp branches
      assert all(torch.equal(it[0], it[2]) for it in items)


def test_swap_kernel_matches_torch_lerp(P):
  """plm_lerp_f32 against torch.lerp on an odd length, for the eval / train weights of several beta1 and both sides of |w| = 0.5;
  w = 0 and w = 1 are exact, and eval then train returns y to rounding"""
  from plainlm_amd import ops
  n = 1_000_003
  gen = torch.Generator(device='cuda').manual_seed(4)
  p0 = torch.randn(n, device='cuda', generator=gen)
  z = torch.randn(n, device='cuda', generator=gen)
  for w in (1 - 1 / 0.9, 1 - 0.9, 1 - 1 / 0.5, 1 - 0.5, 0.3, 0.7, -0.2, 0.0, 1.0):
    got = ops.lerp_(p0.clone(), z, w)
    ref = torch.lerp(p0, z, w)
    tol = 8 * torch.finfo(torch.float32).eps * torch.maximum(p0.abs(), z.abs()).clamp(min=1.0) * (1.0 + abs(w))
    assert ((got - ref).abs() <= tol).all(), (w, (got - ref).abs().max().item())
    if w == 0.0:
      assert torch.equal(got, p0)
    if w == 1.0:
      assert torch.equal(got, z)
  y = ops.lerp_(ops.lerp_(p0.clone(), z, 1 - 1 / 0.9), z, 1 - 0.9)
  assert relmax(y, p0) < 1e-6


def test_bad_arguments_are_refused_before_any_launch(P):
  from plainlm_amd import _lib, ops
  gen = torch.Generator(device='cuda').manual_seed(3)
  hp = ops.optim_hparams('sfo_adamw', 1e-3, WD, beta1=B1, beta2=B2, eps=EPS, bc2=0.05, ckp1=0.1)
  good = _items([(64, 64, 64)], gen)[0]
  before = good[0].clone()
  with pytest.raises(RuntimeError, match='item 1: sfo_adamw needs v'):
    ops.optim_cast_multi_(hp, [good, good[:3] + (None,) + good[4:]])
  with pytest.raises(RuntimeError, match='item 1: sfo_adamw needs the momentum buffer m'):
    ops.optim_cast_multi_(hp, [good, good[:2] + (None,) + good[3:]])
  with pytest.raises(RuntimeError, match='sfo_adamw needs v'):
    ops.optim_(hp, good[0].view(-1), good[1].view(-1), good[2].view(-1), None)
  with pytest.raises(RuntimeError, match='sfo_adamw needs the momentum buffer m'):
    ops.optim_(hp, good[0].view(-1), good[1].view(-1), None, good[3].view(-1))
  lib = _lib.load()
  with pytest.raises(RuntimeError, match='null p or z'):
    _lib.check(lib.plm_lerp_f32(ops._p(good[0]), C.c_void_p(0), good[0].numel(), 0.5, ops._stream()), 'plm_lerp_f32')
  with pytest.raises(RuntimeError, match='must be positive'):
    _lib.check(lib.plm_lerp_f32(ops._p(good[0]), ops._p(good[2]), 0, 0.5, ops._stream()), 'plm_lerp_f32')
  with pytest.raises(ValueError, match='lerp.z'):
    ops.lerp_(good[0].view(-1), good[2].view(-1)[:-8], 0.5)
  torch.cuda.synchronize()
  assert torch.equal(good[0], before)


# ---- FlatAdamWScheduleFree on the small model ----------------------------------------------------------------------------------------
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


KW = dict(lr=3e-3, betas=[B1, B2], weight_decay=WD, warmup_steps=2)


def _grads(gen, model, step):
  return [torch.randn(p.shape, device='cuda', generator=gen) * (5.0 if step == 0 else 0.01) for p in model.parameters()]


def _close(a, b, what, tol=2e-6):
  assert relmax(a.detach(), b.detach()) < tol, (what, relmax(a.detach(), b.detach()))


def _both_step(opt, topt, m, ref, grads, lr=None):
  for p, q, grad in zip(m.parameters(), ref.parameters(), grads):
    p.main_grad.copy_(grad)
    q.grad = grad.clone()
  if lr is not None:
    for grp in opt.param_groups + topt.param_groups:
      grp['lr'] = lr
  opt.clip_and_step(1.0)
  torch.nn.utils.clip_grad_norm_(list(ref.parameters()), 1.0)
  topt.step()


def test_flat_optimizer_matches_torch_swaps_and_state(P, mdl):
  """clip_and_step(1.0) against clip_grad_norm_ + AdamWScheduleFree over 4 steps (warm-up, step 0 clips), the shadows written by the
  update, PLM_ADAMW_SHADOWS=0 bit for bit, eval() / train() on both sides (x, invalidated shadows, step refused in eval mode), and the
  package's state layout loaded into the torch optimizer (in eval mode) and back, each side continuing the other's trajectory"""
  from plainlm_amd import optim
  m = _small(P, mdl, main_grad=True)
  ref = _small(P, mdl)
  opt = optim.FlatAdamWScheduleFree(m, P.get_param_groups(m, WD), **KW)
  topt = AdamWScheduleFree(P.get_param_groups(ref, WD), **KW)
  assert opt.state_dict()['state'] == {}  # the package creates z / exp_avg_sq at the first step
  gen = torch.Generator(device='cuda').manual_seed(0)
  for step in range(4):
    _both_step(opt, topt, m, ref, _grads(gen, m, step), KW['lr'] * (step + 1) / 4)
  for (n, p), q in zip(m.named_parameters(), ref.parameters()):
    _close(p, q, n)
  assert opt.emits_shadows
  for lin in m.linear_modules():
    assert lin.stale_item() is None
    assert torch.equal(lin._shadow[0], lin.weight.detach().bfloat16())
  # the flat kernel alone: the same parameters bit for bit
  m2 = _small(P, mdl, main_grad=True)
  os.environ['PLM_ADAMW_SHADOWS'] = '0'
  try:
    opt2 = optim.FlatAdamWScheduleFree(m2, P.get_param_groups(m2, WD), **KW)
  finally:
    del os.environ['PLM_ADAMW_SHADOWS']
  gen2 = torch.Generator(device='cuda').manual_seed(0)
  for step in range(4):
    for p, grad in zip(m2.parameters(), _grads(gen2, m2, step)):
      p.main_grad.copy_(grad)
    for grp in opt2.param_groups:
      grp['lr'] = KW['lr'] * (step + 1) / 4
    opt2.clip_and_step(1.0)
  for (n, p), p2 in zip(m.named_parameters(), m2.parameters()):
    assert torch.equal(p.detach(), p2.detach()), n
  # eval: x on both sides, the shadows re-cast from x; a step is refused until train()
  ys = [p.detach().clone() for p in m.parameters()]
  zs = [opt.state[p]['z'].clone() for p in m.parameters()]
  opt.eval()
  topt.eval()
  assert all(not g['train_mode'] for g in opt.param_groups)
  for (n, p), q, y, z in zip(m.named_parameters(), ref.parameters(), ys, zs):
    x = ((y.double() - (1 - B1) * z.double()) / B1).float()
    _close(p, x, 'x ' + n, 1e-6)
    _close(p, q, 'eval ' + n)
  assert all(lin.stale_item() is not None for lin in m.linear_modules())
  with pytest.raises(RuntimeError, match='eval mode'):
    opt.clip_and_step(1.0)
  # flat -> torch from eval mode (a checkpoint's copy); both sides train() and step
  sd = opt.state_dict()
  assert len(sd['state']) == 15 and all(set(st) == {'z', 'exp_avg_sq'} for st in sd['state'].values())
  assert sd['param_groups'][0]['k'] == 4 and sd['param_groups'][0]['train_mode'] is False
  ref2 = _small(P, mdl)
  with torch.no_grad():
    for q, p in zip(ref2.parameters(), m.parameters()):
      q.copy_(p)
  topt2 = AdamWScheduleFree(P.get_param_groups(ref2, WD), **KW)
  topt2.load_state_dict(copy.deepcopy(sd))
  opt.train()
  topt2.train()
  for (n, p), y in zip(m.named_parameters(), ys):
    _close(p, y, 'train ' + n, 1e-6)
  _both_step(opt, topt2, m, ref2, _grads(gen, m, 4))
  for (n, p), q in zip(m.named_parameters(), ref2.parameters()):
    _close(p, q, 'flat->torch ' + n)
  # torch -> flat: a fresh flat optimizer on torch's parameters and state (in eval mode) continues like torch
  topt2.eval()
  m3 = _small(P, mdl, main_grad=True)
  with torch.no_grad():
    for p3, q in zip(m3.parameters(), ref2.parameters()):
      p3.copy_(q)
  opt3 = optim.FlatAdamWScheduleFree(m3, P.get_param_groups(m3, WD), **KW)
  opt3.load_state_dict(copy.deepcopy(topt2.state_dict()))
  assert opt3.param_groups[0]['k'] == 5 and not opt3.param_groups[0]['train_mode'] and all(opt3._primed)
  assert opt3.param_groups[0]['weight_sum'] == topt2.param_groups[0]['weight_sum']
  opt3.train()
  topt2.train()
  _both_step(opt3, topt2, m3, ref2, _grads(gen, m3, 5))
  for (n, p3), q in zip(m3.named_parameters(), ref2.parameters()):
    _close(p3, q, 'torch->flat ' + n)


# ---- the engine ------------------------------------------------------------------------------------------------------------------------
def _engine_cfg(**over):
  EC = dict(model='transformer', vocab_size=256, seq_len=64, d_model=128, expand='8/3', n_layers=2, n_heads=2,
            mlp_class='glu', tie_embeddings=False, torch_compile=False, micro_batch_size=1, grad_accumulation_steps=2,
            dtype='bfloat16', optim='sfo_adamw', fused_optim=True, lr=3e-3, weight_decay=0.1, beta1=0.9, beta2=0.95,
            grad_clip=1.0, scheduler='warmup_cosine', warmup_steps=2, cooldown_steps=None, lr_start=0.0, lr_end=1e-5,
            lr_end_pct=None, steps_budget=8, resume=False, seed=100)
  EC.update(over)
  return namedtuple('Config', EC.keys())(**EC)


def _tokens():
  return torch.from_numpy(np.load(os.path.join(GOLDEN, 'engine.npz'))['tokens'])


def _engine(P, mdl, cfg, ckpt=None):
  model, _ = P.construct_model(cfg)
  if ckpt is None:
    model.load_state_dict({k[2:]: v for k, v in mdl.items() if k.startswith('w:')})
  return P.TorchEngine(model, cfg, 'cuda', None, ckpt)


def _ckpt(eng, micro):
  return copy.deepcopy({'step': micro // 2, 'state_dict': eng.model.state_dict(), 'optimizer': eng.optimizer.state_dict(),
                        'scheduler': eng.scheduler.state_dict(), 'scaler': eng.scaler.state_dict()})


def test_engine_fused_equals_torch_and_eval_at_x(P, mdl):
  """HipEngine with optim sfo_adamw, accumulation 2, clip 1.0, warmup-cosine on top of the optimizer's own warm-up: the flat tail against
  AdamWScheduleFree (fused_optim False) over 5 optimizer steps; eval() after 3 steps gives the loss of a model loaded with the host-computed
  x = (y - (1 - b1) z) / b1, and training afterwards follows the run that did not evaluate to within the swap's rounding"""
  tok = _tokens()
  batch = lambda i: {'input_ids': tok[i % tok.shape[0]]}  # noqa: E731
  val_batches = [batch(12), batch(13)]
  from plainlm_amd import optim as O
  runs = {}
  for fused in (True, False):
    eng = _engine(P, mdl, _engine_cfg(fused_optim=fused))
    assert isinstance(eng.optimizer, O.FlatAdamWScheduleFree) == fused and isinstance(eng.optimizer, AdamWScheduleFree)
    assert eng.optimizer.param_groups[0]['warmup_steps'] == 2
    runs[fused] = [float(eng.step(batch(i))) for i in range(10)]
  lf, lt = runs[True], runs[False]
  assert lf[:2] == lt[:2], (lf[:2], lt[:2])
  np.testing.assert_allclose(lf, lt, rtol=2e-4)
  # eval after 3 optimizer steps, at x
  eng = _engine(P, mdl, _engine_cfg())
  head = [float(eng.step(batch(i))) for i in range(6)]
  assert head == lf[:6]
  ys = {n: p.detach().double().clone() for n, p in eng.model.named_parameters()}
  zs = {n: eng.optimizer.state[p]['z'].detach().double().clone() for n, p in eng.model.named_parameters()}
  val = eng.eval(val_batches)
  assert all(not g['train_mode'] for g in eng.optimizer.param_groups)
  xs = {n: ((ys[n] - (1 - B1) * zs[n]) / B1).float().cpu() for n in ys}
  assert max(relmax(p, xs[n]) for n, p in eng.model.named_parameters()) < 1e-6
  ref = _engine(P, mdl, _engine_cfg(optim='adamw'))
  ref.model.load_state_dict(xs)
  val_x = ref.eval(val_batches)
  assert abs(val - val_x) <= 1e-4 * abs(val_x), (val, val_x)
  y_val = _engine(P, mdl, _engine_cfg(optim='adamw'))
  y_val.model.load_state_dict({n: t.float().cpu() for n, t in ys.items()})
  assert y_val.eval(val_batches) != val  # x is not y: the swap happened
  # training resumes at y: the same trajectory as without the eval
  tail = [float(eng.step(batch(i))) for i in range(6, 10)]
  assert all(g['train_mode'] for g in eng.optimizer.param_groups)
  np.testing.assert_allclose(tail, lf[6:], rtol=1e-4)


def test_engine_checkpoint_both_ways(P, mdl):
  """A checkpoint written after an eval (model at x, train_mode False) resumes bit for bit under the fused engine; loaded by the torch
  engine it continues within the fused / torch tolerance, and the torch engine's own checkpoint resumes under the fused engine"""
  tok = _tokens()
  batch = lambda i: {'input_ids': tok[i % tok.shape[0]]}  # noqa: E731
  eng = _engine(P, mdl, _engine_cfg())
  for i in range(6):
    eng.step(batch(i))
  eng.eval([batch(12)])
  ckpt = _ckpt(eng, 6)
  assert ckpt['optimizer']['param_groups'][0]['train_mode'] is False
  tail = [float(eng.step(batch(i))) for i in range(6, 12)]
  fused = _engine(P, mdl, _engine_cfg(resume=True), copy.deepcopy(ckpt))
  assert [float(fused.step(batch(i))) for i in range(6, 12)] == tail
  torch_eng = _engine(P, mdl, _engine_cfg(resume=True, fused_optim=False), copy.deepcopy(ckpt))
  assert type(torch_eng.optimizer) is AdamWScheduleFree
  mid = [float(torch_eng.step(batch(i))) for i in range(6, 8)]
  np.testing.assert_allclose(mid, tail[:2], rtol=2e-4)
  torch_eng.eval([batch(12)])
  back = _ckpt(torch_eng, 8)
  again = _engine(P, mdl, _engine_cfg(resume=True), back)
  assert again.optimizer.param_groups[0]['k'] == 4 and all(again.optimizer._primed)
  np.testing.assert_allclose([float(again.step(batch(i))) for i in range(8, 12)], tail[2:], rtol=2e-4)


# ---- two ranks through the reducer ---------------------------------------------------------------------------------------------------
def _free_port():
  with socket.socket() as s:
    s.bind(('127.0.0.1', 0))
    return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
  import torch.distributed as dist
  os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
  dist.init_process_group('gloo', rank=rank, world_size=world)
  torch.cuda.set_device(0)
  import plainlm_amd as P
  from plainlm_amd.optim import FlatAdamWScheduleFree
  z = np.load(os.path.join(GOLDEN, 'model.npz'))
  w = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')}
  if rank != 0:  # the constructor's broadcast overwrites this; z must be created from the broadcast weights
    w = {k: v + 0.01 for k, v in w.items()}
  cfg = _engine_cfg(lr_start=1e-4)
  model, _ = P.construct_model(cfg)
  model.load_state_dict(w)
  eng = P.TorchEngine(model, cfg, 'cuda:0', 0, None, comm_backend='torch', bucket_cap_mb=0.2)
  assert isinstance(eng.optimizer, FlatAdamWScheduleFree) and len(eng.reducer.buckets) > 4
  tok = _tokens()
  losses = [eng.step({'input_ids': tok[k * world + rank]}).item() for k in range(4)]
  val = eng.eval([{'input_ids': tok[12 + rank]}])
  losses += [eng.step({'input_ids': tok[k * world + rank]}).item() for k in range(4, 6)]
  torch.cuda.synchronize()
  torch.save({'params': {n: p.detach().cpu().clone() for n, p in eng.model.named_parameters()},
              'z': {n: eng.optimizer.state[p]['z'].cpu().clone() for n, p in eng.model.named_parameters()},
              'losses': losses, 'val': val}, os.path.join(out_dir, f'r{rank}.pt'))
  dist.barrier()
  dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_rank_flat_sfo_adamw_keeps_ranks_identical(P, tmp_path):
  """two ranks on one GPU (gloo data plane on the CUDA tensors, as tests/test_optim_ddp_gpu.py), 3 optimizer windows with an eval
  between the second and the third: y, z and the reduced validation loss identical on both ranks, every tensor moved"""
  import torch.multiprocessing as mp
  mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
  r0, r1 = (torch.load(tmp_path / f'r{r}.pt') for r in range(2))
  z = np.load(os.path.join(GOLDEN, 'model.npz'))
  for n, p in r0['params'].items():
    assert torch.equal(p, r1['params'][n]) and torch.equal(r0['z'][n], r1['z'][n]), n
    assert not torch.equal(p, torch.from_numpy(z['w:' + n])), n
  assert r0['val'] == r1['val'] and np.isfinite(r0['val'])
  assert all(np.isfinite(r0['losses'] + r1['losses']))
