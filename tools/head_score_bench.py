"""A/B of the evaluation head in one process, the two sides alternating, random operands (zeros run 17-41 % fast, see README):
  A  gemm_nt into a fresh [M, out_pad] bf16 buffer + ce_fwd_bwd_ + mean   (HeadLossFn.forward under no_grad: today's eval head)
  B  head_score + mean                                                     (eval_head: fused)
and the plain gemm_nt alone (into a reused buffer) as the floor.  Medians of --runs timed runs after --warmup, HIP events around each
run; peak memory of each side above the operands.
Usage: python tools/head_score_bench.py [--runs 20] [--out profiles/head_score_bench.txt]"""
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
  ap.add_argument('--runs', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  lines = ['# tools/head_score_bench.py: one process, A / B / floor alternating, random normal operands (W std 0.02), median of %d runs' % a.runs,
           '# A = gemm_nt into a fresh [M, out_pad] buffer + ce_fwd_bwd_ + mean; B = head_score + mean; floor = gemm_nt alone (reused buffer)',
           '# %-24s %10s %10s %10s %8s %12s %12s' % ('M, V, K', 'A ms', 'B ms', 'floor ms', 'B / A', 'A peak MiB', 'B peak MiB')]
  for M, V, K in SHAPES:
    pad = (V + 63) // 64 * 64
    Y = torch.randn(M, K, device='cuda').to(BF)
    W = (0.02 * torch.randn(V, K, device='cuda')).to(BF)
    t = torch.randint(0, V, (M,), device='cuda')

    def fa():
      buf = torch.empty((M, pad), dtype=BF, device='cuda')
      ops.gemm_nt(Y, W, out=buf[:, :V])
      return ops.mean(ops.ce_fwd_bwd_(buf, t, 1.0 / M, V=V))

    def fb():
      return ops.mean(ops.head_score(Y, W, t))

    ops.release_workspaces()
    pb = peak(fb)
    pa = peak(fa)
    keep = torch.empty((M, pad), dtype=BF, device='cuda')
    ff = lambda: ops.gemm_nt(Y, W, out=keep[:, :V])  # noqa: E731
    for _ in range(a.warmup):
      timed(fa), timed(fb), timed(ff)
    ta, tb, tf = [], [], []
    for _ in range(a.runs):
      ta.append(timed(fa))
      tb.append(timed(fb))
      tf.append(timed(ff))
    ma, mb, mf = statistics.median(ta), statistics.median(tb), statistics.median(tf)
    lines.append('  %-24s %10.3f %10.3f %10.3f %8.3f %12.1f %12.1f   (A min %.3f max %.3f, B min %.3f max %.3f)'
                 % ('%d, %d, %d' % (M, V, K), ma, mb, mf, mb / ma, pa / 2**20, pb / 2**20, min(ta), max(ta), min(tb), max(tb)))
    del keep, Y, W
    torch.cuda.empty_cache()
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
