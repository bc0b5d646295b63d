"""The non-attention kernels against oracle/parity_ops.py's error budget on a real MI355X: cross-entropy on every fast-path
template and the generic kernel, RMSNorm on every template (partly filled chunks, the grid-stride backward), SwiGLU and both
plain-MLP activations over the whole exact-bf16 range that matters, the stand-alone RoPE pass at head dims 32 / 64 / 128,
and the fused GEMM epilogues at operands that reach exp2's overflow.  The shapes and input classes are parity_ops' lists,
on which tests/test_parity_budget_ops.py calibrates the budget; references are fp64, computed only on the rows a case
launches."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity_ops as P  # noqa: E402

BF16 = torch.bfloat16


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


@pytest.mark.parametrize('M,V,ld', P.CE_CASES)
def test_cross_entropy_budget(ops, M, V, ld):
  x, t = P.ce_inputs(M, V, seed=V + ld)
  gs = 1.0 / M
  buf = torch.full((M, ld), 7.0, dtype=BF16, device='cuda')
  buf[:, :V] = x.cuda()
  rows = ops.ce_fwd_bwd_(buf, t.cuda(), gs, V=V)
  P.check(P.ce(buf, rows, P.ce_reference(x, t, gs, V)), f'ce M={M} V={V} ld={ld}')


@pytest.mark.parametrize('M,d,branch', P.RMS_CASES)
def test_rmsnorm_budget(ops, M, d, branch):
  x, w, br, dy, gin = P.rms_inputs(M, d, M * d + branch, branch)
  wc = w.cuda()
  xout, y, rstd = ops.rmsnorm_fwd(x.cuda(), wc, 1e-6, branch=None if br is None else br.cuda(), write_xout=True)
  r = x + br.float() if br is not None else x
  assert torch.equal(xout.cpu(), r)
  ref_y, ref_rstd = P.rmsnorm_fwd_reference(r, w, 1e-6)
  dx, dxb, dw = ops.rmsnorm_bwd(dy.cuda(), xout, wc, rstd, gin=None if gin is None else gin.cuda(), want_bf16=True)
  assert torch.equal(dxb, dx.bfloat16())
  ref_dx, ref_dw, dw_scale = P.rmsnorm_bwd_reference(dy, r, w, rstd)
  m = P.merge(P.rmsnorm_fwd(y, rstd, ref_y, ref_rstd), P.rmsnorm_bwd(dx, dw, ref_dx, ref_dw, dw_scale, gin))
  # the two other ways the step reduces dw: accumulating onto a gradient, and deferred partials + one colsum_multi launch
  acc = torch.full((d,), 0.5, device='cuda')
  ops.rmsnorm_bwd(dy.cuda(), xout, wc, rstd, dw_out=acc, dw_accumulate=True)
  _, _, part = ops.rmsnorm_bwd(dy.cuda(), xout, wc, rstd, defer_dw=True)
  out = torch.full((d,), float('nan'), device='cuda')  # a column colsum_multi leaves unwritten stays NaN and fails
  ops.colsum_multi([(part, out, False)])
  m = P.merge(m, P.rmsnorm_bwd(dx, acc - 0.5, ref_dx, ref_dw, dw_scale, gin), P.rmsnorm_bwd(dx, out, ref_dx, ref_dw, dw_scale, gin))
  P.check(m, f'rmsnorm M={M} d={d} branch={branch}')


@pytest.mark.parametrize('M,h', P.SWIGLU_CASES)
def test_swiglu_budget(ops, M, h):
  u = P.act_inputs(M, 2 * h, M + h)
  dout = torch.randn(M, h, generator=torch.Generator().manual_seed(h)).to(BF16)
  out = ops.swiglu_fwd(u.cuda())
  du = ops.swiglu_bwd(dout.cuda(), u.cuda())
  ref_bwd, allow = P.swiglu_bwd_reference(dout, u)
  P.check(P.merge(P.elementwise(out, P.swiglu_fwd_reference(u)), P.elementwise(du, ref_bwd, allow)), f'swiglu M={M} h={h}')


@pytest.mark.parametrize('kind', ['silu', 'relu_sq'])
@pytest.mark.parametrize('M,n', P.ACT_CASES)
def test_mlp_activation_budget(ops, M, n, kind):
  u = P.act_inputs(M, n, M + n)
  dout = torch.randn(M, n, generator=torch.Generator().manual_seed(n)).to(BF16)
  out = ops.act_fwd(u.cuda(), kind)
  du = ops.act_bwd(dout.cuda(), u.cuda(), kind)
  ref_bwd, allow = P.act_bwd_reference(dout, u, kind)
  P.check(P.merge(P.elementwise(out, P.act_fwd_reference(u, kind)), P.elementwise(du, ref_bwd, allow)), f'act {kind} M={M} n={n}')


@pytest.mark.parametrize('hd,B,T,nh,tab', P.ROPE_CASES)
def test_rope_qk_budget(ops, hd, B, T, nh, tab):
  """plm_rope_qk directly against fp64 (the attention tests build their references from its output, where a RoPE defect
  cancels); hd 32 and 128 always take this pass, hd 64 when qkv_rope's fused epilogue does not apply."""
  d = nh * hd
  qkv = torch.randn(B * T, 3 * d, generator=torch.Generator().manual_seed(hd + T)).to(BF16)
  cos, sin = O.rope_table(hd, tab)
  got = ops.rope_qk_(qkv.cuda(), cos.cuda(), sin.cuda(), B, T, nh).cpu()
  assert torch.equal(got[:, 2 * d:], qkv[:, 2 * d:])
  ref, allow = P.rope_reference(qkv, cos, sin, B, T, nh)
  P.check(P.elementwise(got[:, :2 * d], ref, allow), f'rope hd={hd} B={B} T={T} nh={nh}')


# --------------------------------------------------------------------------------------
# the fused epilogues where plm_sigmoid's exp2 overflows: same bits as GEMM + the stand-alone kernel
# --------------------------------------------------------------------------------------
def test_fc1_swiglu_epilogue_at_extreme_operands(ops):
  """Weights scaled so that |u| reaches ~200 (exp2(-u log2e) overflows fp32 past u = -88.7): the fused epilogue still gives
  the stand-alone kernel's bits, and those are within the budget."""
  M, h, K = 2048, 2048, 768
  g = torch.Generator(device='cuda').manual_seed(31)
  x = torch.randn(M, K, generator=g, device='cuda').to(BF16)
  w = (1.5 * torch.randn(2 * h, K, generator=g, device='cuda')).to(BF16)
  u, act = ops.fc1_swiglu(x, w)
  assert u.float().abs().max().item() > 100
  assert torch.equal(u, ops.gemm_nt(x, w)) and torch.equal(act, ops.swiglu_fwd(u))
  rows = slice(0, 256)
  P.check(P.elementwise(act[rows], P.swiglu_fwd_reference(u[rows].cpu())), 'fc1_swiglu extreme')


def test_fc2_dx_swiglu_bwd_epilogue_at_extreme_operands(ops):
  """u over +-100 (parity_ops.act_inputs) and d(act) = dy @ w2t^T of size ~100: fused == GEMM + swiglu_bwd, bit for bit."""
  M, h, K = 2048, 2048, 768
  g = torch.Generator(device='cuda').manual_seed(32)
  dy = torch.randn(M, K, generator=g, device='cuda').to(BF16)
  w2t = (3.0 * torch.randn(h, K, generator=g, device='cuda')).to(BF16)
  u = P.act_inputs(M, 2 * h, 33).cuda()
  du = ops.fc2_dx_swiglu_bwd(dy, w2t, u)
  dact = ops.gemm_nt(dy, w2t)
  assert torch.equal(du, ops.swiglu_bwd(dact, u))
  rows = slice(0, 256)
  ref, allow = P.swiglu_bwd_reference(dact[rows].cpu(), u[rows].cpu())
  P.check(P.elementwise(du[rows], ref, allow), 'fc2_dx_swiglu_bwd extreme')


def test_qkv_rope_epilogue_at_large_operands(ops):
  """The RoPE epilogue of the w_qkv GEMM on a shape that takes the fused path, with projections of size ~100: same bits as
  GEMM + plm_rope_qk, within the budget."""
  B, T, nh, K = 8, 1024, 12, 768
  d = nh * 64
  g = torch.Generator(device='cuda').manual_seed(34)
  x = torch.randn(B * T, K, generator=g, device='cuda').to(BF16)
  w = (3.0 * torch.randn(3 * d, K, generator=g, device='cuda')).to(BF16)
  cos, sin = O.rope_table(64, T)
  got = ops.qkv_rope(x, w, cos.cuda(), sin.cuda(), B, T, nh)
  two = ops.gemm_nt(x, w)
  pre = two[T - 2:T + 2].cpu()  # rows around the sequence boundary (positions T-2, T-1, 0, 1)
  ops.rope_qk_(two, cos.cuda(), sin.cuda(), B, T, nh)
  assert torch.equal(got, two)
  rows = slice(T - 2, T + 2)
  ref, allow = P.rope_reference(pre, torch.cat([cos[T - 2:], cos[:2]]), torch.cat([sin[T - 2:], sin[:2]]), 1, 4, nh)
  P.check(P.elementwise(got[rows, :2 * d], ref, allow), 'qkv_rope large')
