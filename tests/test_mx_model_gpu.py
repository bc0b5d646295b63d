"""linear_precision 'mxfp8' on a real MI355X: each MX autograd Function against a CPU emulation of the contract (tests/mx_ref.py
quantizer, fp64 matmul, bf16 rounding where the kernels round; the stand-alone RoPE / SwiGLU / activation kernels, which are checked
against the oracle elsewhere, applied to the emulated intermediates), through the GradSink and the autograd path; the whole model
against the same weights in bf16; the engine over a few hundred steps and a checkpoint that moves from mxfp8 to bf16."""
import copy
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_ref  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TOL = 2.0 ** -7  # |got - ref| <= TOL * max |ref|: two bf16 roundings (2^-8 relative each) along the chain


@pytest.fixture(scope='module')
def P():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  import plainlm_amd
  return plainlm_amd


def _q(x):
  """fp64 value of an MX operand blocked along the last dim of x (a CPU bf16 / float tensor)."""
  return mx_ref.qdq(x.cpu())


def _bf(t):
  return t.float().to(BF).double()


def _close(got, ref, what):
  got, ref = got.detach().double().cpu(), ref.double().cpu()
  err = float((got - ref).abs().max())
  assert err <= TOL * float(ref.abs().max()), (what, err, float(ref.abs().max()))


def _emul_linear(x, w, dy):
  """(y, dx, dw) of y = x W^T on MX operands: x [M, K], w [N, K], dy [M, N], all bf16 on the CPU."""
  y = _bf(_q(x) @ _q(w).t())
  dx = _bf(_q(dy) @ _q(w.t()).t())
  dw = _q(dy.t()) @ _q(x.t()).t()
  return y, dx, dw


def _model(P, prec, mlp='glu', d=128, layers=2, heads=2, T=64):
  torch.manual_seed(0)
  return P.Transformer(P.ModelConfig(vocab_size=256, seq_len=T, dim=d, expand=8 / 3, n_layers=layers, n_heads=heads, mlp=mlp,
                                     linear_precision=prec)).cuda()


def _run_linear(lin, x, dy, sink):
  lin.weight.grad = None
  xx = x.cuda().requires_grad_(True)
  if sink:
    lin.sink.enabled = True
    lin.weight.main_grad = torch.full_like(lin.weight, float('nan'))
    lin.sink.begin_window()
  y = lin(xx)
  y.backward(dy.cuda())
  if sink:
    lin.sink.flush_dw()
    dw = lin.weight.main_grad
    lin.sink.enabled = False
    del lin.weight.main_grad
  else:
    dw = lin.weight.grad
  return y, xx.grad, dw


@pytest.mark.parametrize('sink', [False, True])
def test_mx_linear_fn_against_emulation(P, sink):
  """LinearFn on an mx linear (w_out of block 0) with ragged M = 1000: y and dx within two bf16 roundings of the emulation, dW (fp32) too; the sink path
  (deferred MX dW GEMM storing into main_grad) and the autograd path give the same bits."""
  m = _model(P, 'mxfp8')
  lin = m.layers[0].attn.w_out
  assert lin.mx
  g = torch.Generator().manual_seed(1)
  x = torch.randn(1000, 128, generator=g).to(BF)
  dy = (torch.randn(1000, 128, generator=g) * 1e-3).to(BF)
  y, dx, dw = _run_linear(lin, x, dy, sink)
  w = lin.weight.detach().cpu().to(BF)
  ry, rdx, rdw = _emul_linear(x, w, dy)
  _close(y, ry, 'y')
  _close(dx, rdx, 'dx')
  _close(dw, rdw, 'dw')
  assert y.dtype == BF and dw.dtype == torch.float32
  if sink:  # same bits as autograd mode
    _, dx2, dw2 = _run_linear(lin, x, dy, False)
    assert torch.equal(dx2, dx) and torch.equal(dw2, dw)


@pytest.mark.parametrize('mlp', ['glu', 'mlp', 'mlp_relu_sq'])
@pytest.mark.parametrize('sink', [False, True])
def test_mx_mlp_fns_against_emulation(P, mlp, sink):
  from plainlm_amd import ops
  m = _model(P, 'mxfp8', mlp=mlp)
  blk = m.layers[0].mlp
  g = torch.Generator().manual_seed(2)
  x = torch.randn(512, 128, generator=g).to(BF)
  dy = (torch.randn(512, 128, generator=g) * 1e-3).to(BF)
  xx = x.cuda().requires_grad_(True)
  for lin in (blk.fc1, blk.fc2):
    lin.weight.grad = None
    if sink:
      lin.weight.main_grad = torch.full_like(lin.weight, float('nan'))
  if sink:
    m.sink.enabled = True
    m.sink.begin_window()
  y = blk.apply_fn(xx)
  y.backward(dy.cuda())
  if sink:
    m.sink.flush_dw()
    m.sink.enabled = False
  dw1, dw2 = ((blk.fc1.weight.main_grad, blk.fc2.weight.main_grad) if sink else (blk.fc1.weight.grad, blk.fc2.weight.grad))
  w1, w2 = blk.fc1.weight.detach().cpu().to(BF), blk.fc2.weight.detach().cpu().to(BF)
  act_f = ops.swiglu_fwd if mlp == 'glu' else (lambda u: ops.act_fwd(u, blk.kind))
  act_b = ops.swiglu_bwd if mlp == 'glu' else (lambda d, u: ops.act_bwd(d, u, blk.kind))
  # stage by stage: each GEMM's emulation starts from the kernels' own bf16 intermediate (a one-ulp difference upstream would move an
  # e4m3 rounding of the next operand, which is not what a stage-level check is after); the intermediates are the Function's bits
  u = ops.gemm_mx_nt(ops.mx_quant(xx.detach(), cols=False)[0], blk.fc1.mx_weights()[0])
  _close(u, _bf(_q(x) @ _q(w1).t()), 'u')
  act = act_f(u)
  _close(y, _bf(_q(act.cpu()) @ _q(w2).t()), 'y')
  dact = ops.gemm_mx_nt(ops.mx_quant(dy.cuda(), cols=False)[0], blk.fc2.mx_weights()[1])
  _close(dact, _bf(_q(dy) @ _q(w2.t()).t()), 'dact')
  du = act_b(dact, u).cpu()
  _close(dw2, _q(dy.t()) @ _q(act.cpu().t()).t(), 'dw2')
  _close(xx.grad, _bf(_q(du) @ _q(w1.t()).t()), 'dx')
  _close(dw1, _q(du.t()) @ _q(x.t()).t(), 'dw1')


def test_mx_qkv_rope_fn_against_emulation(P):
  from plainlm_amd import ops
  m = _model(P, 'mxfp8')
  att = m.layers[0].attn
  B, T = 4, 64
  g = torch.Generator().manual_seed(3)
  x = torch.randn(B * T, 128, generator=g).to(BF)
  dy = (torch.randn(B * T, 384, generator=g) * 1e-3).to(BF)
  cos, sin = m._rope(torch.device('cuda'))
  xx = x.cuda().requires_grad_(True)
  from plainlm_amd import functional as Fn
  y = Fn.QKVRopeFn.apply(xx, att.w_qkv.weight, att.w_qkv, cos, sin, B, T, att.n_heads)
  y.backward(dy.cuda())
  w = att.w_qkv.weight.detach().cpu().to(BF)
  ry, rdx, rdw = _emul_linear(x, w, dy)
  ry = ry.to(BF).cuda()
  ops.rope_qk_(ry, cos, sin, B, T, att.n_heads)
  _close(y, ry.cpu(), 'y')
  _close(xx.grad, rdx, 'dx')
  _close(att.w_qkv.weight.grad, rdw, 'dw')


def _loss_and_grads(model, ids, tgt, mask=None):
  model.zero_grad(set_to_none=True)
  loss = model.loss(ids, tgt, mask)
  loss.backward()
  return float(loss), {n: p.grad.detach().float() for n, p in model.named_parameters()}


def _compare(P, mlp, d, layers, heads, B, T, mask_kind):
  g = torch.Generator(device='cuda').manual_seed(4)
  ids = torch.randint(0, 256, (B, T), device='cuda', generator=g)
  tgt = torch.randint(0, 256, (B, T), device='cuda', generator=g)
  mask = None
  if mask_kind:
    idx = torch.arange(T, device='cuda')
    doc = (idx // (T // 4)).view(1, T)
    mask = (doc.unsqueeze(2) == doc.unsqueeze(1)) & (idx.view(T, 1) >= idx.view(1, T))
    mask = mask.expand(B, T, T).contiguous()
  out = {}
  for prec in ('bf16', 'mxfp8'):
    m = _model(P, prec, mlp=mlp, d=d, layers=layers, heads=heads, T=T)
    if mask_kind == 'dense':
      m.cfg.attn_mask_mode = 'dense'
    out[prec] = _loss_and_grads(m, ids, tgt, mask)
  (lb, gb), (lm, gm) = out['bf16'], out['mxfp8']
  rel = abs(lm - lb) / abs(lb)
  cos, worst = min((float(torch.nn.functional.cosine_similarity(gb[n].flatten(), gm[n].flatten(), dim=0)), n) for n in gb)
  print(f'{mlp} {mask_kind} B={B} T={T} d={d}: loss rel {rel:.2e}, min grad cosine {cos:.5f} ({worst})')
  return rel, cos


@pytest.mark.parametrize('mlp,mask', [('glu', None), ('glu', 'doc'), ('glu', 'dense'), ('mlp', None), ('mlp_relu_sq', None)])
def test_whole_model_mxfp8_against_bf16_small(P, mlp, mask):
  """2 layers, d = 128, B = 4, T = 256, same init in both precisions: loss within 1e-3 relative, every parameter gradient at cosine >= 0.98.
  Measured on an MI355X: loss rel 1.1e-5 ... 1.1e-4, min cosine over all parameters 0.9957 ... 0.9965 (margins: ~9x on the loss, ~4.6x
  on 1 - cos)."""
  rel, cos = _compare(P, mlp, 128, 2, 2, 4, 256, mask)
  assert rel <= 1e-3 and cos >= 0.98, (rel, cos)


def test_whole_model_mxfp8_against_bf16_160m(P):
  """The 160M model (12 layers, d = 768) at B = 32, T = 1024: loss within 1e-3 relative, every parameter gradient at cosine >= 0.95.
  Measured on an MI355X: loss rel 1.5e-4, min cosine over all parameters 0.976 (margins: ~7x on the loss, 2x on 1 - cos)."""
  rel, cos = _compare(P, 'glu', 768, 12, 12, 32, 1024, None)
  assert rel <= 1e-3 and cos >= 0.95, (rel, cos)


def _engine_cfg(**over):
  EC = dict(model='transformer', vocab_size=256, seq_len=64, d_model=128, expand='8/3', n_layers=2, n_heads=2,
            mlp_class='glu', tie_embeddings=False, torch_compile=False, micro_batch_size=1, grad_accumulation_steps=2,
            dtype='bfloat16', optim='adamw', fused_optim=True, lr=3e-3, weight_decay=0.1, beta1=0.9, beta2=0.95, dampening=0.0,
            grad_clip=1.0, scheduler='warmup_cosine', warmup_steps=10, cooldown_steps=None, lr_start=0.0, lr_end=1e-5,
            lr_end_pct=None, steps_budget=150, resume=False, seed=100, linear_precision='bf16')
  EC.update(over)
  return namedtuple('Config', EC.keys())(**EC)


def test_engine_mxfp8_loss_curve_and_checkpoint_to_bf16(P, golden_dir):
  """The engine with linear_precision mxfp8 against bf16 from the same init over 300 micro-steps (150 optimizer steps, fused AdamW, clip) on
  the fixed token rows of tests/golden/engine.npz: both curves fall, and the mxfp8 loss tracks the bf16 one at every step
  (bound: |mx - bf16| <= 12 % of the first loss; measured on an MI355X: at most 0.39 = 6.9 %, mid-curve while both runs memorise the
  rows - 5.59 -> 0.05 - on slightly different trajectories; the ends agree within 0.002).  A checkpoint written under mxfp8 at step 100 resumes under bf16, and its first losses track the bf16 run."""
  tokens = torch.from_numpy(np.load(os.path.join(golden_dir, 'engine.npz'))['tokens'])
  batch = lambda i: {'input_ids': tokens[i % tokens.shape[0]]}  # noqa: E731
  curves, ckpt = {}, None
  for prec in ('bf16', 'mxfp8'):
    cfg = _engine_cfg(linear_precision=prec)
    torch.manual_seed(0)
    model, mcfg = P.construct_model(cfg)
    assert mcfg.linear_precision == prec
    eng = P.TorchEngine(model, cfg, 'cuda', None, None)
    losses = []
    for i in range(300):
      losses.append(float(eng.step(batch(i))))
      if prec == 'mxfp8' and i == 199:
        ckpt = copy.deepcopy({'step': 100, 'state_dict': eng.model.state_dict(), 'optimizer': eng.optimizer.state_dict(),
                              'scheduler': eng.scheduler.state_dict(), 'scaler': eng.scaler.state_dict()})
    curves[prec] = np.array(losses)
  b, mx = curves['bf16'], curves['mxfp8']
  gap = np.abs(mx - b) / (0.12 * b[0])
  print(f'engine: max |mx - bf16| {np.abs(mx - b).max():.3e}, max gap / bound {gap.max():.3f}, first {b[0]:.3f} / {mx[0]:.3f}, '
        f'last {b[-1]:.3f} / {mx[-1]:.3f}')
  assert np.isfinite(mx).all() and mx[-20:].mean() < mx[:20].mean()
  assert gap.max() <= 1.0, gap.max()
  cfg = _engine_cfg(linear_precision='bf16', resume=True)
  model, _ = P.construct_model(cfg)
  eng2 = P.TorchEngine(model, cfg, 'cuda', None, ckpt)
  resumed = np.array([float(eng2.step(batch(i))) for i in range(200, 220)])
  assert (np.abs(resumed - mx[200:220]) / (0.12 * b[0])).max() <= 1.0
