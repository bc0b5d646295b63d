"""A/B of loss + prediction per token in one process, the sides alternating, random operands (zeros run fast, see README):
  A  gemm_nt into a fresh [M, out_pad] bf16 buffer + torch.argmax + ce_fwd_bwd_ + mean   (today's route; entropy left out, in A's favour)
  B  head_predict (pred, logp, entropy, nll) + mean                                      
  S  head_score + mean                                                                   (the loss alone: what the prediction mode adds to it)
Medians of --runs timed runs after --warmup, HIP events around each run; peak memory of A and B above the operands.
Usage: python tools/head_predict_bench.py [--runs 12] [--out profiles/head_predict_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plainlm_amd import ops  # noqa: E402

BF = torch.bfloat16
SHAPES = [(32768, 50280, 768), (65536, 50280, 768), (16384, 50280, 1024)]


def timed(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1)


def peak(fn):
  torch.cuda.synchronize()
  torch.cuda.empty_cache()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  fn()
  torch.cuda.synchronize()
  return torch.cuda.max_memory_allocated() - base


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=12)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  lines = ['# tools/head_predict_bench.py: one process, A / B / S alternating, random normal operands (W std 0.02), median of %d runs [min max]' % a.runs,
           '# A = gemm_nt into a fresh [M, out_pad] buffer + torch.argmax + ce_fwd_bwd_ + mean; B = head_predict + mean; S = head_score + mean',
           '# %-20s %26s %26s %26s %7s %7s %11s %11s' % ('M, V, K', 'A ms', 'B ms', 'S ms', 'B / A', 'B / S', 'A peak MiB', 'B peak MiB')]
  for M, V, K in SHAPES:
    pad = (V + 63) // 64 * 64
    Y = torch.randn(M, K, device='cuda').to(BF)
    W = (0.02 * torch.randn(V, K, device='cuda')).to(BF)
    t = torch.randint(0, V, (M,), device='cuda')

    def fa():
      buf = torch.empty((M, pad), dtype=BF, device='cuda')
      ops.gemm_nt(Y, W, out=buf[:, :V])
      pred = torch.argmax(buf[:, :V], dim=-1)
      return pred, ops.mean(ops.ce_fwd_bwd_(buf, t, 1.0 / M, V=V))

    def fb():
      r = ops.head_predict(Y, W, t)
      return r.pred, ops.mean(r.nll)

    def fs():
      return ops.mean(ops.head_score(Y, W, t))

    ops.release_workspaces()
    pb = peak(fb)
    pa = peak(fa)
    for _ in range(a.warmup):
      timed(fa), timed(fb), timed(fs)
    ta, tb, ts = [], [], []
    for _ in range(a.runs):
      ta.append(timed(fa))
      tb.append(timed(fb))
      ts.append(timed(fs))
    ma, mb, ms = statistics.median(ta), statistics.median(tb), statistics.median(ts)
    cell = lambda m, v: '%.3f [%.3f %.3f]' % (m, min(v), max(v))  # noqa: E731
    lines.append('  %-20s %26s %26s %26s %7.3f %7.3f %11.1f %11.1f'
                 % ('%d, %d, %d' % (M, V, K), cell(ma, ta), cell(mb, tb), cell(ms, ts), mb / ma, mb / ms, pa / 2**20, pb / 2**20))
    del Y, W
    ops.release_workspaces()
    torch.cuda.empty_cache()
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
