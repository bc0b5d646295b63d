"""The paged KV cache against the contiguous one at the 160M shape:
  C  decode_step on a KVCache [B, Tmax, 2*dim]           P  decode_step on a PagedKVCache over a PagePool
unfused and fused (FC, FP: one ops.decode_layer / ops.decode_layer_paged call per layer),
at uniform lengths (B, context) and on a ragged batch of 32 sequences with lengths spread from 64 to 4096, the sides alternating in one
process (tools/gen_bench.py's ``alternate``): device ms by HIP events, median of --runs [min max], host enqueue.  Then one layer's
attention alone (ops.attn_decode / ops.attn_decode_paged), the pool bytes in use against B * Tmax bytes, and ``serve`` against
``generate`` / ``generate_fused`` run in static waves of max_batch prompts on --prompts prompts with mixed lengths and budgets (wall ms,
one run each after a warm-up run).  --lib: another build of the library (the chunk size is a compile-time constant of it).
Usage: python tools/paged_bench.py [--runs 20] [--lib path/to/libplainlm_hip.so] --out profiles/paged_bench.txt"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--prompts', type=int, default=64)
  ap.add_argument('--max-batch', type=int, default=16)
  ap.add_argument('--lib', default=None)
  ap.add_argument('--no-serve', action='store_true')
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  from plainlm_amd import _lib
  if a.lib:
    _lib.LIB_PATH = os.path.abspath(a.lib)
  from gen_bench import ModelConfig, Transformer, alternate, med, ops, timed
  from plainlm_amd import ops_paged
  ops.KV_PAGED_CHUNK = ops_paged.KV_PAGED_CHUNK = chunk = int(_lib.load().plm_kv_paged_chunk_rows())
  torch.manual_seed(0)
  cfg = ModelConfig(vocab_size=50280, seq_len=4096 + 68, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu')
  m = Transformer(cfg).cuda()
  nh = cfg.n_heads
  lines = ['# tools/paged_bench.py: 160M (12 layers, d 768, 12 heads, V 50280), chunk = %d keys per decode workgroup; C = contiguous cache, '
           'P = paged cache; one process, sides alternating; ms, HIP events, median of %d [min max]' % (chunk, a.runs)]

  def alone(fn):
    v = []
    for i in range(a.warmup + a.runs):
      torch.cuda.synchronize()
      e = timed(fn)
      if i >= a.warmup:
        v.append(e)
    return v

  with torch.no_grad():
    ragged = [64 + round(i * (4096 - 64) / 31) for i in range(32)]
    for tag, lens in (('B = 8, context 1024', [1024] * 8), ('B = 32, context 4096', [4096] * 32), ('B = 32, ragged 64 .. 4096', ragged)):
      B, Tmax = len(lens), max(lens) + 4
      cont = m.new_cache(B, Tmax)
      pool = m.new_page_pool(sum(-(-(n + 4) // 64) for n in lens) + 8)
      paged = m.new_cache_paged(B, pool, Tmax)
      for i in range(cfg.n_layers):
        cont.kv[i].copy_(torch.randn(cont.kv[i].shape, device='cuda') * 0.5)
        pool.kv[i].copy_(torch.randn(pool.kv[i].shape, device='cuda') * 0.5)
      l_dev = torch.tensor(lens, dtype=torch.int32, device='cuda')
      nxt = torch.randint(0, cfg.vocab_size, (B,), device='cuda')

      def reset():
        cont.set_lens(l_dev)
        paged.set_lens(lens)
      sides = {'C': lambda: m.decode_step(nxt, cont), 'P': lambda: m.decode_step(nxt, paged),
               'FC': lambda: m.decode_step(nxt, cont, fused=True), 'FP': lambda: m.decode_step(nxt, paged, fused=True)}
      dev, host, calls, _ = alternate(sides, reset, a)
      reset()
      lines.append('%s: cache bytes C %d, P (pages in use) %d = %.2f of C' % (tag, sum(t.numel() * 2 for t in cont.kv), pool.bytes_in_use(),
                                                                             pool.bytes_in_use() / sum(t.numel() * 2 for t in cont.kv)))
      for how, kc, kp in (('unfused', 'C', 'P'), ('fused  ', 'FC', 'FP')):
        for k, name in ((kc, 'contiguous step (C)'), (kp, 'paged step (P)     ')):
          lines.append('  %s %s  device %s   host enqueue %s   library calls %3d' % (how, name, med(dev[k]), med(host[k]), len(calls[k])))
        c, p = dev[kc], dev[kp]
        where = 'overlaps' if min(p) <= max(c) and min(c) <= max(p) else ('lies above' if min(p) > max(c) else 'lies below')
        lines.append('    P / C (medians) %.2f; P\'s [min max] %s C\'s' % (statistics.median(p) / statistics.median(c), where))
      q = torch.randn(B, cfg.dim, device='cuda').to(torch.bfloat16)
      lines.append('  alone, one layer: attn_decode %s   attn_decode_paged %s' % (
          med(alone(lambda: ops.attn_decode(q, cont.kv[0], cont.lens, nh))),
          med(alone(lambda: ops.attn_decode_paged(q, pool.kv[0], paged.table, paged.lens, nh, Lcap=paged.lcap())))))
      del cont, paged, pool, sides
    if not a.no_serve:
      g = torch.Generator().manual_seed(1)
      N, S = a.prompts, a.max_batch
      plen = torch.randint(32, 257, (N,), generator=g).tolist()
      budget = torch.randint(16, 129, (N,), generator=g).tolist()
      prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).cuda() for n in plen]

      def waves(gen):
        for w in range(0, N, S):
          idx = list(range(w, min(w + S, N)))
          T = max(plen[i] for i in idx)
          x = torch.zeros((len(idx), T), dtype=torch.int64, device='cuda')
          for r, i in enumerate(idx):
            x[r, :plen[i]] = prompts[i]
          gen(x, max(budget[i] for i in idx), prompt_lens=[plen[i] for i in idx])

      def wall(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
      lines.append('%d prompts (32 .. 256 tokens), budgets 16 .. 128 (%d tokens asked for), max_batch %d, wall ms of one run after a warm-up run:'
                   % (N, sum(budget), S))
      lines.append('  serve %.1f   serve(fused=True) %.1f   generate in static waves %.1f   generate_fused in static waves %.1f' % (
          wall(lambda: m.serve(prompts, budget, S)), wall(lambda: m.serve(prompts, budget, S, fused=True)), wall(lambda: waves(m.generate)),
          wall(lambda: waves(m.generate_fused))))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'a') as f:
      f.write(text)


if __name__ == '__main__':
  main()
