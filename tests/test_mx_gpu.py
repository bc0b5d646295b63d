"""MXFP8 kernels (csrc/mx.hip) on a real MI355X against the CPU reference of the format (tests/mx_ref.py):

  * the quantizer bit for bit (bytes and scale bytes, both orientations): every finite bf16 bit pattern, random data from 1e-30 to 1e30,
    ragged shapes with zero / NaN / Inf blocks, the grouped launch;
  * the MX NT GEMM: exactly on small-integer e4m3 data with asymmetric per-block scales (pins the operand and scale lane maps of
    v_mfma_scale_f32_32x32x64_f8f6f4), within a measured accumulation bound on random data at the step's shapes, all three output modes,
    NaN / Inf blocks, run-to-run bit equality."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_ref  # noqa: E402

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


def _check_quant(ops, x):
  r, c = ops.mx_quant(x.cuda())
  d, s = mx_ref.quantize(x)
  assert torch.equal(r.data.cpu(), d), int((r.data.cpu() != d).sum())
  assert torch.equal(r.scales.cpu(), s), int((r.scales.cpu() != s).sum())
  dt, st = mx_ref.quantize(x.t())
  assert torch.equal(c.data.cpu(), dt), int((c.data.cpu() != dt).sum())
  assert torch.equal(c.scales.cpu(), st), int((c.scales.cpu() != st).sum())
  return r, c


def test_quant_every_finite_bf16_value(ops):
  """All 65280 finite bf16 bit patterns, shuffled into 32-element blocks, alone and with each block's first element replaced by a block
  maximum at the edges of the scale rule (448 * 2^e exactly, just above it, powers of two, a bf16 subnormal, the largest bf16)."""
  bits = torch.arange(1 << 16, dtype=torch.int32).to(torch.int16)
  vals = bits.view(BF)
  vals = vals[torch.isfinite(vals.float())]
  g = torch.Generator().manual_seed(0)
  vals = vals[torch.randperm(vals.numel(), generator=g)]
  n = vals.numel() // 256 * 256
  base = vals[:n].view(-1, 256)
  _check_quant(ops, base)
  for m in (448.0, 448.0 * 2.0 ** -20, 456.0, 1.0, 2.0 ** -126, 2.0 ** -130, 3.3895e38, 1.75, 1.7578125):
    x = base.clone()
    x[:, ::32] = torch.tensor(m, dtype=BF)
    _check_quant(ops, x)


def test_quant_random_scales_and_ragged_special_blocks(ops):
  g = torch.Generator().manual_seed(1)
  for sc in (1e-30, 1e-10, 1e-3, 1.0, 1e3, 1e10, 1e30):
    _check_quant(ops, (torch.randn(200, 328, generator=g) * sc).to(BF))
  x = (torch.randn(77, 200, generator=g)).to(BF)
  x[3, 40:72] = 0
  x[5, 10] = float('nan')
  x[9, 100] = float('inf')
  x[60, 199] = float('-inf')
  x[:, 64:96] *= 1e-38  # bf16 subnormals, the clamp at -127
  _check_quant(ops, x)
  _check_quant(ops, torch.zeros(1, 8, dtype=BF))
  # a leading dimension wider than the logical width, and one orientation at a time
  big = (torch.randn(130, 264, generator=g) * 3).to(BF).cuda()
  view = big[:, :136]
  r, c = ops.mx_quant(view, rows=True, cols=False)
  assert c is None and torch.equal(r.data.cpu(), mx_ref.quantize(view.cpu())[0])
  r, c = ops.mx_quant(view, rows=False, cols=True)
  assert r is None and torch.equal(c.scales.cpu(), mx_ref.quantize(view.cpu().t())[1])


def test_quant_multi_equals_single(ops):
  g = torch.Generator().manual_seed(2)
  xs = [(torch.randn(r, c, generator=g) * 10 ** (i - 3)).to(BF).cuda() for i, (r, c) in enumerate([(768, 768), (2304, 768), (96, 40), (33, 1000), (4096, 768), (768, 2048), (8, 8)])]
  multi = ops.mx_quant_multi(xs)
  for x, (r, c) in zip(xs, multi):
    r1, c1 = ops.mx_quant(x)
    for a, b in ((r, r1), (c, c1)):
      assert torch.equal(a.data, b.data) and torch.equal(a.scales, b.scales) and a.shape == b.shape


def _mx_from(ops, data, scales, k):
  return ops.MxTensor(data.cuda(), scales.cuda(), (data.shape[0], k))


def _int_operand(rows, kp, g, asym):
  """e4m3 bytes of small integers in [-2, 2] and scale bytes 124..130 (2^-3 .. 2^3), every block its own scale: fp32-exact products."""
  ints = torch.randint(-2, 3, (rows, kp), generator=g).float()
  ints += asym  # an asymmetric pattern on top (row / column index dependence)
  ints = ints.clamp(-2, 2)
  data = ints.to(torch.float8_e4m3fn).view(torch.uint8)
  scales = torch.randint(124, 131, (rows, kp // 32), generator=g).to(torch.uint8)
  return data, scales


@pytest.mark.parametrize('M,N,K', [(32, 32, 128), (200, 160, 512), (128, 256, 256), (300, 40, 384)])
def test_gemm_exact_on_small_integers(ops, M, N, K):
  """deq(A) deq(B)^T is exactly representable in fp32 here, so any lane-map or scale-map error shows as a wrong element."""
  g = torch.Generator().manual_seed(M + N + K)
  asym_a = (torch.arange(M).unsqueeze(1) % 3 == 0).float() * (torch.arange(K).unsqueeze(0) % 5 == 1).float()
  asym_b = (torch.arange(N).unsqueeze(1) % 7 == 2).float() * (torch.arange(K).unsqueeze(0) % 11 == 3).float() * -1
  da, sa = _int_operand(M, K, g, asym_a)
  db, sb = _int_operand(N, K, g, asym_b)
  ref = mx_ref.dequantize(da, sa) @ mx_ref.dequantize(db, sb).t()
  a, b = _mx_from(ops, da, sa, K), _mx_from(ops, db, sb, K)
  got = ops.gemm_mx_nt(a, b, out_dtype=torch.float32).cpu().double()
  bad = (got != ref).nonzero()
  assert bad.numel() == 0, (bad[:8].tolist(), got[tuple(bad[0])].item(), ref[tuple(bad[0])].item())
  # bf16 store = RNE of the same fp32 values; accumulate adds onto what is there
  assert torch.equal(ops.gemm_mx_nt(a, b).cpu(), ref.float().to(BF))
  base = torch.randn(M, N, generator=g).cuda()
  out = base.clone()
  ops.gemm_mx_nt(a, b, out=out, accumulate=True)
  assert torch.equal(out.cpu(), base.cpu() + ref.float())


def test_gemm_nan_and_inf_blocks_spread_to_exactly_their_rows_and_columns(ops):
  g = torch.Generator().manual_seed(5)
  x = torch.randn(160, 256, generator=g).to(BF)
  w = torch.randn(96, 256, generator=g).to(BF)
  x[5, 70] = float('nan')
  w[7, 200] = float('inf')
  a, _ = ops.mx_quant(x.cuda(), cols=False)
  b, _ = ops.mx_quant(w.cuda(), cols=False)
  out = ops.gemm_mx_nt(a, b, out_dtype=torch.float32).cpu()
  nan = torch.isnan(out)
  assert nan[5].all() and nan[:, 7].all()
  nan[5] = False
  nan[:, 7] = False
  assert not nan.any() and torch.isfinite(out[~torch.isnan(out)]).all()


def _sampled_check(a_bf, b_bf, got, g, rows=192, cols=192):
  """got [M, N] against fp64 deq(A) deq(B)^T on a random sample of rows and columns: |err| <= 2^-14 * sum |a||b| + the output's own
  rounding (2^-8 |ref| for bf16).  The scaled MFMA does not round like a chain of fp32 FMAs: measured on random normal operands, its fp32
  result is off by up to 1.4e-5 * sum |a||b| at K = 128 and 5.0e-6 at K = 768 (median 1e-6 / 5e-7); 2^-14 = 6.1e-5 leaves a margin of 4x.
  Small-integer data, where every partial sum is exact, comes out exact (test_gemm_exact_on_small_integers)."""
  M, N = got.shape
  ri = torch.randperm(M, generator=g)[:rows]
  ci = torch.randperm(N, generator=g)[:cols]
  qa = mx_ref.qdq(a_bf[ri].cpu())
  qb = mx_ref.qdq(b_bf[ci].cpu())
  ref = qa @ qb.t()
  mag = qa.abs() @ qb.abs().t()
  err = (got[ri][:, ci].cpu().double() - ref).abs()
  out_ulp = 2.0 ** -8 if got.dtype == BF else 2.0 ** -23
  assert (err <= 2.0 ** -14 * mag + out_ulp * ref.abs() + 1e-30).all(), float((err / (mag + 1e-30)).max())


SHAPES_160M = [(32768, 2304, 768), (32768, 768, 768), (32768, 4096, 768), (32768, 768, 2048),   # forward
               (32768, 768, 2304), (32768, 768, 4096), (32768, 2048, 768),                      # dX
               (2304, 768, 32768), (4096, 768, 32768), (768, 2048, 32768)]                      # dW (M = out_features, reduce over tokens)


@pytest.mark.parametrize('M,N,K', SHAPES_160M + [(16384, 5632, 1024), (1000, 2304, 768)])
def test_gemm_random_at_step_shapes(ops, M, N, K):
  g = torch.Generator().manual_seed(M ^ N ^ K)
  a_bf = torch.randn(M, K, generator=g).to(BF)
  b_bf = (torch.randn(N, K, generator=g) * 0.02).to(BF)
  a, _ = ops.mx_quant(a_bf.cuda(), cols=False)
  b, _ = ops.mx_quant(b_bf.cuda(), cols=False)
  out = ops.gemm_mx_nt(a, b)
  _sampled_check(a_bf, b_bf, out, g)
  out2 = ops.gemm_mx_nt(a, b)
  assert torch.equal(out, out2)
  if K == 32768:  # the dW form: fp32 accumulate across windows
    acc = torch.zeros(M, N, device='cuda')
    ops.gemm_mx_nt(a, b, out=acc, accumulate=True)
    ops.gemm_mx_nt(a, b, out=acc, accumulate=True)
    f = ops.gemm_mx_nt(a, b, out_dtype=torch.float32)
    assert torch.equal(acc, f + f)


def test_gemm_transposed_operands_for_dw(ops):
  """dW = dY^T X with both operands quantized along the token dimension (the column-blocked copies), ragged token count."""
  g = torch.Generator().manual_seed(9)
  T = 1000
  dy = torch.randn(T, 256, generator=g).to(BF)
  x = torch.randn(T, 384, generator=g).to(BF)
  _, dyt = ops.mx_quant(dy.cuda())
  _, xt = ops.mx_quant(x.cuda())
  dw = ops.gemm_mx_nt(dyt, xt, out_dtype=torch.float32).cpu().double()
  ref = mx_ref.qdq(dy.t()) @ mx_ref.qdq(x.t()).t()
  mag = mx_ref.qdq(dy.t()).abs() @ mx_ref.qdq(x.t()).abs().t()
  assert ((dw - ref).abs() <= 2.0 ** -14 * mag).all()
