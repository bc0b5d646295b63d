"""A/B of the k best tokens with their log-probabilities in one process, the sides alternating, random operands (zeros run fast, see README):
  A  gemm_nt into a fresh [M, V] bf16 buffer + torch.topk(k) + torch.logsumexp   (today's route, outside HIP after the GEMM)
  B  head_topk(k) at each chunk size (PLM_HT_CHUNK = 256 / 512 / 1024 rows)      
  P  head_predict                                                                (the argmax alone: what the list costs on top of it)
Medians of --runs timed runs after --warmup, HIP events around each run; peak memory of A and B above the operands.
Usage: python tools/head_topk_bench.py [--runs 20] [--out profiles/head_topk_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plainlm_amd import ops  # noqa: E402

BF = torch.bfloat16
SHAPES = [(32768, 50280, 768), (65536, 50280, 768), (16384, 50280, 1024)]
KS = (1, 5, 64)
CHUNKS = (256, 512, 1024)


def timed(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1)


def peak(fn):
  torch.cuda.synchronize()
  ops.release_workspaces()
  torch.cuda.empty_cache()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  fn()
  torch.cuda.synchronize()
  return torch.cuda.max_memory_allocated() - base


def set_chunk(rows):
  os.environ['PLM_HT_CHUNK'] = str(rows)
  ops.reload_env()
  assert ops.head_topk_chunk_rows() == rows


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit('head_topk_bench needs an MI355X: a timing taken anywhere else says nothing')
  default = ops.head_topk_chunk_rows()
  cell = lambda v: '%.3f [%.3f %.3f]' % (statistics.median(v), min(v), max(v))  # noqa: E731
  lines = ['# tools/head_topk_bench.py: one process, the sides alternating, random normal operands (W std 0.02), median of %d runs [min max], ms' % a.runs,
           '# A = gemm_nt into a fresh [M, V] buffer + torch.topk(k) + torch.logsumexp; B<rows> = head_topk(k, targets) with PLM_HT_CHUNK = rows; '
           'P = head_predict(targets); the library constant is %d' % default,
           '# %-18s %3s %24s %24s %24s %24s %24s %7s %7s %10s %10s'
           % ('M, V, K', 'k', 'A', 'B256', 'B512', 'B1024', 'P', 'B / A', 'B / P', 'A peak MiB', 'B peak MiB')]
  for M, V, K in SHAPES:
    Y = torch.randn(M, K, device='cuda').to(BF)
    W = (0.02 * torch.randn(V, K, device='cuda')).to(BF)
    t = torch.randint(0, V, (M,), device='cuda')
    for k in KS:
      def fa():
        buf = torch.empty((M, V), dtype=BF, device='cuda')
        ops.gemm_nt(Y, W, out=buf)
        return torch.topk(buf, k, dim=-1), torch.logsumexp(buf, dim=-1)

      def fb(rows):
        set_chunk(rows)
        return ops.head_topk(Y, W, k, t, want_lse=True)

      def fp():
        return ops.head_predict(Y, W, t)

      pb = peak(lambda: fb(default))
      pa = peak(fa)
      sides = [fa] + [lambda rows=rows: fb(rows) for rows in CHUNKS] + [fp]
      for _ in range(a.warmup):
        for f in sides:
          timed(f)
      ts = [[] for _ in sides]
      for _ in range(a.runs):
        for f, v in zip(sides, ts):
          v.append(timed(f))
      med = [statistics.median(v) for v in ts]
      mb = med[1 + CHUNKS.index(default)]
      lines.append('  %-18s %3d %24s %24s %24s %24s %24s %7.3f %7.3f %10.1f %10.1f'
                   % (('%d, %d, %d' % (M, V, K), k) + tuple(cell(v) for v in ts) + (mb / med[0], mb / med[-1], pa / 2**20, pb / 2**20)))
      print(lines[-1], flush=True)
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
