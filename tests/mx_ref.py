"""CPU reference of the MXFP8 operand format (include/plainlm_hip.h plm_mx_quant): the contract the GPU quantizer
and MX GEMM are tested against bit for bit.

A block is 32 consecutive elements along the reduction dimension.  amax = max |x|, E = floor(log2 amax), e = E - 8 if amax <= 448 * 2^(E-8)
else E - 7 (the smallest e with amax <= 448 * 2^e), clamped to [-127, 127]; scale byte e + 127; element RNE_e4m3fn(x * 2^-e) with subnormals
(torch's CPU float8_e4m3fn cast).  amax = 0: scale byte 0 and zero elements; any NaN / Inf in the block: scale byte 0xFF, elements 0x7F.
The reduction dimension is zero-padded to a multiple of 128."""
import torch


def pad128(k):
  return (int(k) + 127) // 128 * 128


def quantize(x):
  """x [R, K] (any float dtype; the library quantizes bf16) -> (data uint8 [R, Kp], scales uint8 [R, Kp / 32]), blocked along K."""
  x = x.detach().to('cpu', torch.float64)
  R, K = x.shape
  kp = pad128(K)
  xp = torch.zeros((R, kp), dtype=torch.float64)
  xp[:, :K] = x
  blk = xp.view(R, kp // 32, 32)
  bad = ~torch.isfinite(blk).all(dim=2)
  amax = torch.where(bad, torch.zeros(()), blk.abs().amax(dim=2))
  mant, ex = torch.frexp(amax)               # amax = mant * 2^ex, mant in [0.5, 1)
  E = ex - 1                                 # floor(log2 amax)
  e = torch.where(amax <= 448.0 * torch.ldexp(torch.ones(()), E - 8), E - 8, E - 7).clamp(-127, 127)
  zero = amax == 0
  e = torch.where(zero | bad, torch.zeros_like(e), e)
  y = torch.ldexp(blk, -e.unsqueeze(2).to(torch.float64))  # exact: a power-of-two scaling in fp64
  y = torch.where(torch.isfinite(y), y, torch.zeros(()))
  q = y.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8).clone()  # fp64 -> fp32 is exact above 2^-126, below it both round to 0
  q[zero] = 0
  q[bad] = 0x7F
  s = (e + 127).to(torch.uint8)
  s[zero] = 0
  s[bad] = 0xFF
  return q.view(R, kp), s


def dequantize(data, scales):
  """(data uint8 [R, Kp], scales uint8 [R, Kp / 32]) -> float64 [R, Kp]; scale byte 0xFF is NaN."""
  R, kp = data.shape
  v = data.cpu().contiguous().view(torch.float8_e4m3fn).to(torch.float64).view(R, kp // 32, 32)
  sc = scales.cpu().to(torch.int64)
  f = torch.ldexp(torch.ones(sc.shape, dtype=torch.float64), (sc - 127).to(torch.float64))
  f = torch.where(sc == 255, torch.full((), float('nan'), dtype=torch.float64), f)
  return (v * f.unsqueeze(2)).view(R, kp)


def qdq(x):
  """x [R, K] -> float64 [R, K]: what an MX GEMM operand blocked along K represents."""
  d, s = quantize(x)
  return dequantize(d, s)[:, :x.shape[1]]
