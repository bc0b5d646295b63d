"""CPU reference of the FP8 KV cache format (include/plainlm_hip.h plm_kv8_quant_rows): the contract the GPU
quantisers, the dequantiser and the attention kernels over that cache are tested against bit for bit.  tests/mx_ref.py's rule with a
block of 16 and no padding:

A block is ``block`` consecutive elements of a row.  amax = max |x|, E = floor(log2 amax), e = E - 8 if amax <= 448 * 2^(E-8) else E - 7
(the smallest e with amax <= 448 * 2^e), clamped to [-127, 127]; scale byte e + 127; element RNE_e4m3fn(x * 2^-e) with subnormals (torch's
CPU float8_e4m3fn cast).  amax = 0: scale byte 0 and zero elements; any NaN / Inf in the block: scale byte 0xFF, elements 0x7F.
Dequantisation: code * 2^(s - 127), NaN for scale byte 0xFF.

``forward_qdq`` is the tiny model's forward with the rotated k and v passed through quantise-dequantise: what a model whose every
attention reads an FP8 cache computes, in fp32, built from oracle.cpu_ref's own functions."""
import torch

from oracle import cpu_ref as O

BLOCK = 16


def row_bytes(dm):
  """Bytes of a cache row: k codes dm | v codes dm | k scales dm/16 | v scales dm/16, rounded up to a multiple of 16."""
  return (2 * dm + dm // 8 + 15) // 16 * 16


def quantize(x, block=BLOCK):
  """x [R, K] (any float dtype; the library quantises bf16), K % block == 0 -> (codes uint8 [R, K], scales uint8 [R, K / block])."""
  x = x.detach().to('cpu', torch.float64)
  R, K = x.shape
  assert K % block == 0
  blk = x.view(R, K // block, block)
  bad = ~torch.isfinite(blk).all(dim=2)
  amax = torch.where(bad, torch.zeros(()), blk.abs().amax(dim=2))
  _, ex = torch.frexp(amax)                  # amax = mant * 2^ex, mant in [0.5, 1)
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
  return q.view(R, K), s


def dequantize(codes, scales, block=BLOCK):
  """(codes uint8 [R, K], scales uint8 [R, K / block]) -> float64 [R, K]; scale byte 0xFF is NaN."""
  R, K = codes.shape
  v = codes.cpu().contiguous().view(torch.float8_e4m3fn).to(torch.float64).view(R, K // block, block)
  sc = scales.cpu().to(torch.int64)
  f = torch.ldexp(torch.ones(sc.shape, dtype=torch.float64), (sc - 127).to(torch.float64))
  f = torch.where(sc == 255, torch.full((), float('nan'), dtype=torch.float64), f)
  return (v * f.unsqueeze(2)).view(R, K)


def qdq(x, block=BLOCK):
  """x [..., K] -> float64 of the same shape: what the cache holds of x."""
  flat = x.reshape(-1, x.shape[-1])
  return dequantize(*quantize(flat, block), block).view(x.shape)


def pack_rows(kvrows, ld=None):
  """bf16 / float k | v rows [R, 2*dm] -> cache rows uint8 [R, ld] (default row_bytes(dm)); pad bytes are zero."""
  R, two_dm = kvrows.shape
  dm = two_dm // 2
  q, s = quantize(kvrows)
  out = torch.zeros((R, row_bytes(dm) if ld is None else ld), dtype=torch.uint8)
  out[:, :two_dm] = q
  out[:, two_dm:two_dm + two_dm // BLOCK] = s
  return out


def unpack_rows(rows, dm):
  """cache rows uint8 [R, >= 2*dm + dm/8] -> (codes [R, 2*dm], scales [R, dm/8])."""
  rows = rows.cpu()
  return rows[:, :2 * dm], rows[:, 2 * dm:2 * dm + 2 * dm // BLOCK]


def forward_qdq(params, cfg, ids, qdq_fn=qdq, round_kv=None):
  """oracle.cpu_ref.forward with qdq_fn applied to the rotated k and to v (blocks of 16 along a head): ids int64 [B, T] -> fp32 logits
  [B, T, V].  qdq_fn=None is the plain forward.  round_kv: a dtype k / v are rounded to before qdq_fn (the library quantises bf16 values;
  None: the fp32 ones)."""
  B, T = ids.shape
  d, nh, hd, h = cfg.dim, cfg.n_heads, cfg.head_dim, cfg.hidden
  cos, sin = O.rope_table(hd, cfg.seq_len, cfg.rope_theta)

  def cached(t):  # [B, T, nh, hd]
    if round_kv is not None:
      t = t.to(round_kv).float()
    return t if qdq_fn is None else qdq_fn(t).to(torch.float32)
  x = params['embed_tokens.weight'][ids]
  for i in range(cfg.n_layers):
    p = f'layers.{i}.'
    n1 = O.rmsnorm(x, params[p + 'attn_norm.weight'], cfg.rmsnorm_eps)
    qkv = n1 @ params[p + 'attn.w_qkv.weight'].t()
    q, k, v = (t.reshape(B, T, nh, hd) for t in qkv.split(d, dim=2))
    q, k = O.rope_apply(q, cos, sin), O.rope_apply(k, cos, sin)
    a = O.attention(q, cached(k), cached(v))
    x = x + a @ params[p + 'attn.w_out.weight'].t()
    n2 = O.rmsnorm(x, params[p + 'mlp_norm.weight'], cfg.rmsnorm_eps)
    u = n2 @ params[p + 'mlp.fc1.weight'].t()
    x = x + O.mlp_act(u, h, cfg.mlp) @ params[p + 'mlp.fc2.weight'].t()
  xn = O.rmsnorm(x, params['out_norm.weight'], cfg.rmsnorm_eps)
  head = params['embed_tokens.weight'] if cfg.tie_embeddings else params['lm_head.weight']
  return xn @ head.t()
