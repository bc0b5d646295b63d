"""Shared-prefix pages on one MI355X, the numbers of profiles/cascade_bench.txt:
  python tools/cascade_bench.py --out profiles/cascade_bench.txt
(a) one layer's attention for decode rows that share a prefix and hold 64 own keys each: ops.attn_ragged_paged_cascade against
ops.attn_ragged_paged on the same aliased table; (b) serve_shared(fused='wide', prefill_chunk=128) on the 64-prompt mix behind a
1024-token prefix against serve(fused='wide', prefill_chunk=128) with the prefix prepended to every prompt, and the peak pages in use.
One process, sides alternating, median [min max]."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--serve-runs', type=int, default=3)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  from gen_bench import ModelConfig, Transformer, med, ops, timed
  from plainlm_amd import generate as G
  torch.manual_seed(0)
  cfg = ModelConfig(vocab_size=50280, seq_len=4096 + 512, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu')
  m = Transformer(cfg).cuda()
  nh = cfg.n_heads
  lines = ['# tools/cascade_bench.py: 160M (12 layers, d 768, 12 heads, V 50280); one process, sides alternating; attention: ms, HIP events, '
           'median of %d [min max]; serve: wall ms, median of %d [min max]' % (a.runs, a.serve_runs)]

  def alternating(sides, measure, runs, warmup):
    v = {k: [] for k in sides}
    for i in range(warmup + runs):
      for k, fn in sides.items():
        torch.cuda.synchronize()
        e = measure(fn)
        if i >= warmup:
          v[k].append(e)
    return v

  def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3

  with torch.no_grad():
    for rows, shared in ((32, 4096), (32, 1024), (8, 4096)):
      pool = m.new_page_pool(shared // 64 + 2 * rows)
      pool.kv[0].copy_(torch.randn(pool.kv[0].shape, device='cuda') * 0.5)
      prefix = G.PagedPrefix(pool, pool.alloc(shared // 64), torch.zeros(0, dtype=torch.int64))
      cache = m.new_cache_paged(rows, pool, shared + 128)
      for b in range(rows):
        cache.admit_prefix(b, prefix)
      cache.reserve(65)  # 64 own keys and the step's row
      cu, row_seq, _, NT, key_lo, tile_rows, tile_seq, tile_keys, NTg, Pcap = ops.cascade_plan([1] * rows, cache.key_lo, cache.group)
      words = [w.cuda() for w in (cu, row_seq, key_lo, tile_rows, tile_seq, tile_keys)]
      l0 = torch.full((rows,), shared + 64, dtype=torch.int32, device='cuda')
      q = torch.randn(rows, cfg.dim, device='cuda').to(torch.bfloat16)
      table, Lcap = cache.table, cache.lcap()
      sides = {'cascade': lambda: ops.attn_ragged_paged_cascade(q, pool.kv[0], table, l0, words[2], words[0], words[1], *words[3:], nh, NT, NTg, Pcap,
                                                                Lcap=Lcap),
               'ragged': lambda: ops.attn_ragged_paged(q, pool.kv[0], table, l0, words[0], words[1], nh, NT, Lcap=Lcap)}
      v = alternating(sides, timed, a.runs, a.warmup)
      lines.append('(a) %d decode rows, %d shared + 64 own keys, one layer\'s attention: attn_ragged_paged_cascade %s   attn_ragged_paged %s' %
                   (rows, shared, med(v['cascade']), med(v['ragged'])))
      del cache, pool, prefix, sides
    g = torch.Generator().manual_seed(1)
    N, S = 64, 16
    plen = torch.randint(32, 257, (N,), generator=g).tolist()
    budget = torch.randint(16, 129, (N,), generator=g).tolist()
    prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).cuda() for n in plen]
    head = torch.randint(0, cfg.vocab_size, (1024,), generator=g).cuda()
    peak = {}

    class Watched(G.PagePool):  # the pool with a high-water mark of the pages in use
      def alloc(self, k):
        ids = super().alloc(k)
        peak[self.tag] = max(peak.get(self.tag, 0), self.n_pages - self.n_free)
        return ids

    def pool_for(tag, n):
      p = Watched(cfg.n_layers, n, nh, cfg.dim // nh, 'cuda')
      p.tag = tag
      return p
    own = max(-(-(1024 + n + b) // 64) for n, b in zip(plen, budget))
    sides = {"serve_shared(fused='wide', prefill_chunk=128)":
             lambda: m.serve_shared(head, prompts, budget, S, pool=pool_for('shared', 16 + S * (own - 16)), fused='wide', prefill_chunk=128),
             "serve(fused='wide', prefill_chunk=128), prefix prepended":
             lambda: m.serve([torch.cat([head, t]) for t in prompts], budget, S, pool=pool_for('prepended', S * own), fused='wide', prefill_chunk=128)}
    v = alternating(sides, wall_ms, a.serve_runs, 1)
    lines.append('(b) %d prompts (32 .. 256 tokens) behind a 1024-token prefix, budgets 16 .. 128, max_batch %d:' % (N, S))
    lines += ['  %-58s %s   peak pages in use %d' % (k, med(t), peak['shared' if 'shared' in k else 'prepended']) for k, t in v.items()]
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'a') as f:
      f.write(text)


if __name__ == '__main__':
  main()
