"""Times of the dense-mask attention family (csrc/attn_masked.hip) on one GPU: the pack kernel, and one layer's masked forward and backward at
the 160M shape for a causal mask given as a dense mask, a sliding window and a prefix-LM mask, next to the causal kernels on the same shape.
Usage: python tools/masked_bench.py [--B 32] [--T 1024] [--nh 12] [--hd 64] [--pack-B 32] [--pack-T 2048] [--iters 20]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cpu_ref as O  # noqa: E402
from plainlm_amd import ops  # noqa: E402


def timed(fn, iters):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  for _ in range(iters):
    fn()
  b.record()
  torch.cuda.synchronize()
  return a.elapsed_time(b) / iters * 1e3  # us


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--B', type=int, default=32)
  ap.add_argument('--T', type=int, default=1024)
  ap.add_argument('--nh', type=int, default=12)
  ap.add_argument('--hd', type=int, default=64)
  ap.add_argument('--pack-B', type=int, default=32)
  ap.add_argument('--pack-T', type=int, default=2048)
  ap.add_argument('--window', type=int, default=256)
  ap.add_argument('--iters', type=int, default=20)
  a = ap.parse_args()
  res = {}
  pm = torch.ones(a.pack_T, a.pack_T, dtype=torch.bool, device='cuda').tril().expand(a.pack_B, a.pack_T, a.pack_T).contiguous()
  res[f'pack_us B={a.pack_B} T={a.pack_T}'] = timed(lambda: ops.attn_mask_pack(pm), a.iters)
  del pm
  B, T, nh, hd = a.B, a.T, a.nh, a.hd
  g = torch.Generator(device='cuda').manual_seed(0)
  d = nh * hd
  qkv = torch.randn(B * T, 3 * d, generator=g, device='cuda').to(torch.bfloat16)
  dout = torch.randn(B * T, d, generator=g, device='cuda').to(torch.bfloat16)
  cos, sin = (t.cuda() for t in O.rope_table(hd, T))
  qrot = ops.rope_qk_(qkv, cos, sin, B, T, nh)
  out, lse = ops.attn_fwd(qrot, B, T, nh)
  res['causal_kernels_fwd_us'] = timed(lambda: ops.attn_fwd(qrot, B, T, nh), a.iters)
  res['causal_kernels_bwd_us'] = timed(lambda: ops.attn_bwd(qrot, out, dout, lse, cos, sin, B, T, nh), a.iters)
  i = torch.arange(T, device='cuda').view(T, 1)
  j = torch.arange(T, device='cuda').view(1, T)
  masks = {'causal_as_dense': j <= i, f'window{a.window}': (j <= i) & (j > i - a.window), f'prefix{T // 2}': (j <= i) | (j < T // 2)}
  for name, m in masks.items():
    bits, cls = ops.attn_mask_pack(m.expand(B, T, T).contiguous())
    o, l = ops.attn_fwd_masked(qrot, bits, cls, B, T, nh)
    res[f'{name}_fwd_us'] = timed(lambda: ops.attn_fwd_masked(qrot, bits, cls, B, T, nh), a.iters)
    res[f'{name}_bwd_us'] = timed(lambda: ops.attn_bwd_masked(qrot, o, dout, l, cos, sin, bits, cls, B, T, nh), a.iters)
  print(json.dumps({'shape': dict(B=B, T=T, nh=nh, hd=hd), **{k: round(v, 1) for k, v in res.items()}}))


if __name__ == '__main__':
  main()
