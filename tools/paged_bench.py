"""The paged KV cache against the contiguous one at the 160M shape:
  C  decode_step on a KVCache [B, Tmax, 2*dim]           P  decode_step on a PagedKVCache over a PagePool
unfused and fused (FC, FP: one ops.decode_layer / ops.decode_layer_paged call per layer),
at uniform lengths (B, context) and on a ragged batch of 32 sequences with lengths spread from 64 to 4096, the sides alternating in one
process (tools/gen_bench.py's ``alternate``): device ms by HIP events, median of --runs [min max], host enqueue.  Then one layer's
attention alone (ops.attn_decode / ops.attn_decode_paged), the pool bytes in use against B * Tmax bytes, and ``serve`` against
``generate`` / ``generate_fused`` run in static waves of max_batch prompts on --prompts prompts with mixed lengths and budgets (wall ms,
one run each after a warm-up run).  --lib: another build of the library (the chunk size is a compile-time constant of it).
--ragged measures the ragged step instead: (a) one layer's attention for 15 decode rows + one 128-row prompt chunk at
context 1024, ops.attn_ragged_paged on the 143 packed rows against ops.attn_extend_paged on the padded [16, 128] form; (b) an all-decode
batch at (32, 4096) against ops.attn_decode_paged; (c) ``serve`` on the prompt mix with and without prefill_chunk, fused and unfused,
against the static waves, --serve-runs wall-clock runs each, the sides alternating.
Usage: python tools/paged_bench.py [--runs 20] [--lib path/to/libplainlm_hip.so] --out profiles/paged_bench.txt
       python tools/paged_bench.py --ragged --out profiles/ragged_bench.txt
--ragged --wide measures the wide fused layer instead: (a) one ops.ragged_layer_paged_wide call against the unfused
ops chain on the same packed rows (15 decode rows + a 128-row chunk, and 256 rows, context 1024), device ms and host enqueue ms; (b) ``serve``
with fused='wide' at prefill_chunk 64 and 128 against serve(fused=True), serve(prefill_chunk=128) and the fused static waves; (c) a
decode-only step_ragged of 16 rows, fused='wide' against fused=True.
       python tools/paged_bench.py --ragged --wide --out profiles/wide_bench.txt"""
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
  ap.add_argument('--ragged', action='store_true')
  ap.add_argument('--serve-runs', type=int, default=5)
  ap.add_argument('--wide', action='store_true', help='--ragged: the wide fused layer (DESIGN.md section 27) in place of the attention sides')
  ap.add_argument('--prefill-chunk', type=int, default=128, help='--ragged: prompt rows per unfused step (a fused step takes 32 - max_batch)')
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

  def sides_alternating(sides, measure, runs, warmup):
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

  if a.ragged and a.wide:
    lines[0] = ('# tools/paged_bench.py --ragged --wide: 160M (12 layers, d 768, 12 heads, V 50280); one process, sides alternating; layer and step: '
                'ms, median of %d [min max]; serve: wall ms, median of %d [min max]' % (a.runs, a.serve_runs))

    def host_ms(fn):  # the enqueue alone: the device is idle before and drained after
      t0 = time.perf_counter()
      fn()
      e = (time.perf_counter() - t0) * 1e3
      torch.cuda.synchronize()
      return e
    with torch.no_grad():
      i32 = lambda v: torch.tensor(v, dtype=torch.int32, device='cuda')  # noqa: E731
      m.refresh_shadows()
      L0, eps, rope = m.layers[0], m.layers[0].attn_norm.eps, m._rope(torch.device('cuda'))
      an, mn = L0.attn_norm.weight, L0.mlp_norm.weight
      wq, wo, w1, w2 = L0.attn.w_qkv.shadow()[0], L0.attn.w_out.shadow()[0], L0.mlp.fc1.shadow()[0], L0.mlp.fc2.shadow()[0]
      for tag, lens0, counts in (('(a1) 15 decode rows + one 128-row chunk, context 1024', [1024] * 16, [1] * 15 + [128]),
                                 ('(a2) 256 rows: two 128-row chunks, context 1024', [1024] * 2, [128] * 2)):
        pool = m.new_page_pool(sum(-(-(l + c) // 64) for l, c in zip(lens0, counts)))
        cache = m.new_cache_paged(len(counts), pool, max(l + c for l, c in zip(lens0, counts)))
        cache.set_lens([l + c for l, c in zip(lens0, counts)])  # the pages of the step's rows are held
        pool.kv[0].copy_(torch.randn(pool.kv[0].shape, device='cuda') * 0.5)
        table, l0, Lcap = cache.table, i32(lens0), cache.lcap()
        cu, row_seq, _, NT = ops.ragged_plan(counts)
        cu, row_seq = cu.cuda(), row_seq.cuda()
        x0 = torch.randn(sum(counts), cfg.dim, device='cuda')

        def wide():
          ops.ragged_layer_paged_wide(x0.clone(), an, mn, eps, wq, wo, w1, w2, l0, cu, row_seq, rope[0], rope[1], pool.kv[0], table, nh, 'glu',
                                      cache.status, NT, Lcap=Lcap)

        def chain():
          x = x0.clone()
          q, _ = ops.kv_paged_append_rope_packed(ops.gemm_nt(ops.rmsnorm_fwd(x, an, eps)[1], wq), l0, cu, row_seq, rope[0], rope[1], pool.kv[0], table,
                                                 nh, status=cache.status)
          x = x + ops.gemm_nt(ops.attn_ragged_paged(q, pool.kv[0], table, l0, cu, row_seq, nh, NT, Lcap=Lcap), wo).float()
          x + ops.gemm_nt(ops.swiglu_fwd(ops.gemm_nt(ops.rmsnorm_fwd(x, mn, eps)[1], w1)), w2).float()
        sides = {'ragged_layer_paged_wide': wide, 'unfused ops chain': chain}
        dev, host = sides_alternating(sides, timed, a.runs, a.warmup), sides_alternating(sides, host_ms, a.runs, a.warmup)
        lines.append('%s, one layer (%d rows):' % (tag, sum(counts)))
        lines += ['  %-26s device %s   host enqueue %s' % (k, med(dev[k]), med(host[k])) for k in sides]
        del cache, pool, sides
      S = a.max_batch
      tok = torch.randint(0, cfg.vocab_size, (S,), device='cuda')
      pool = m.new_page_pool(S * 17)
      cache = m.new_cache_paged(S, pool, 1024 + 64)

      def step(fused):
        cache.set_lens([1024] * S)
        m.step_ragged(tok, [1] * S, cache, fused=fused)
      v = sides_alternating({"step_ragged(fused='wide')": lambda: step('wide'), 'step_ragged(fused=True)': lambda: step(True)}, timed, a.runs, a.warmup)
      lines.append('(c) a decode-only step of %d rows at context 1024 (set_lens included on both sides), the price of the bits rule:' % S)
      lines += ['  %-26s %s' % (k, med(t)) for k, t in v.items()]
      del cache, pool
      if not a.no_serve:
        g = torch.Generator().manual_seed(1)
        N = a.prompts
        plen = torch.randint(32, 257, (N,), generator=g).tolist()
        budget = torch.randint(16, 129, (N,), generator=g).tolist()
        prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).cuda() for n in plen]

        def waves(gen):
          for w in range(0, N, S):
            idx = list(range(w, min(w + S, N)))
            x = torch.zeros((len(idx), max(plen[i] for i in idx)), dtype=torch.int64, device='cuda')
            for r, i in enumerate(idx):
              x[r, :plen[i]] = prompts[i]
            gen(x, max(budget[i] for i in idx), prompt_lens=[plen[i] for i in idx])
        sides = {"serve(fused='wide', prefill_chunk=64)": lambda: m.serve(prompts, budget, S, fused='wide', prefill_chunk=64),
                 "serve(fused='wide', prefill_chunk=128)": lambda: m.serve(prompts, budget, S, fused='wide', prefill_chunk=128),
                 'serve(fused=True)': lambda: m.serve(prompts, budget, S, fused=True),
                 'serve(prefill_chunk=128)': lambda: m.serve(prompts, budget, S, prefill_chunk=128),
                 'generate_fused in static waves': lambda: waves(m.generate_fused)}
        v = sides_alternating(sides, wall_ms, a.serve_runs, 1)
        lines.append('(b) %d prompts (32 .. 256 tokens), budgets 16 .. 128 (%d tokens asked for), max_batch %d, wall ms, %d runs each after a warm-up run:'
                     % (N, sum(budget), S, a.serve_runs))
        lines += ['  %-40s %s' % (k, med(t)) for k, t in v.items()]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
      with open(a.out, 'a') as f:
        f.write(text)
    return

  if a.ragged:
    lines[0] = ('# tools/paged_bench.py --ragged: 160M (12 layers, d 768, 12 heads, V 50280); one process, sides alternating; attention: ms, HIP '
                'events, median of %d [min max]; serve: wall ms, median of %d [min max]' % (a.runs, a.serve_runs))
    with torch.no_grad():
      i32 = lambda v: torch.tensor(v, dtype=torch.int32, device='cuda')  # noqa: E731
      for tag, lens0, counts in (('(a) 15 decode rows + one 128-row chunk, context 1024', [1024] * 16, [1] * 15 + [128]),
                                 ('(b) 32 decode rows, context 4096', [4095] * 32, [1] * 32)):
        B, n = len(counts), max(counts)
        pool = m.new_page_pool(sum(-(-(l + c) // 64) for l, c in zip(lens0, counts)))
        cache = m.new_cache_paged(B, pool, max(l + c for l, c in zip(lens0, counts)))
        cache.set_lens([l + c for l, c in zip(lens0, counts)])  # the step's rows are appended already
        pool.kv[0].copy_(torch.randn(pool.kv[0].shape, device='cuda') * 0.5)
        table, l0, Lcap = cache.table, i32(lens0), cache.lcap()
        cu, row_seq, _, NT = ops.ragged_plan(counts)
        cu, row_seq = cu.cuda(), row_seq.cuda()
        q = torch.randn(sum(counts), cfg.dim, device='cuda').to(torch.bfloat16)
        sides = {'ragged': lambda: ops.attn_ragged_paged(q, pool.kv[0], table, l0, cu, row_seq, nh, NT, Lcap=Lcap)}
        if n > 1:
          qp, nn = torch.zeros(B * n, cfg.dim, device='cuda', dtype=torch.bfloat16), i32(counts)
          for b in range(B):
            qp[b * n:b * n + counts[b]] = q[cu[b]:cu[b + 1]]
          sides['extend_paged, padded [%d, %d]' % (B, n)] = lambda: ops.attn_extend_paged(qp, pool.kv[0], table, l0, nh, n_new=nn, Lcap=Lcap)
        else:
          lens = i32([l + 1 for l in lens0])
          sides['decode_paged'] = lambda: ops.attn_decode_paged(q, pool.kv[0], table, lens, nh, Lcap=Lcap)
        v = sides_alternating(sides, timed, a.runs, a.warmup)
        (k0, r), (k1, o) = v.items()
        where = 'overlaps' if min(r) <= max(o) and min(o) <= max(r) else ('lies above' if min(r) > max(o) else 'lies below')
        lines.append('%s, one layer\'s attention: attn_ragged_paged (%d rows, %d tiles) %s   attn_%s %s' % (tag, sum(counts), NT, med(r), k1, med(o)))
        lines.append('    ragged / other (medians) %.2f; ragged\'s [min max] %s the other\'s' % (statistics.median(r) / statistics.median(o), where))
        del cache, pool, sides
      if not a.no_serve:
        g = torch.Generator().manual_seed(1)
        N, S = a.prompts, a.max_batch
        plen = torch.randint(32, 257, (N,), generator=g).tolist()
        budget = torch.randint(16, 129, (N,), generator=g).tolist()
        prompts = [torch.randint(0, cfg.vocab_size, (n,), generator=g).cuda() for n in plen]

        def waves(gen):
          for w in range(0, N, S):
            idx = list(range(w, min(w + S, N)))
            x = torch.zeros((len(idx), max(plen[i] for i in idx)), dtype=torch.int64, device='cuda')
            for r, i in enumerate(idx):
              x[r, :plen[i]] = prompts[i]
            gen(x, max(budget[i] for i in idx), prompt_lens=[plen[i] for i in idx])
        C, Cf = a.prefill_chunk, 32 - S
        sides = {'serve': lambda: m.serve(prompts, budget, S), 'serve(prefill_chunk=%d)' % C: lambda: m.serve(prompts, budget, S, prefill_chunk=C),
                 'generate in static waves': lambda: waves(m.generate), 'serve(fused=True)': lambda: m.serve(prompts, budget, S, fused=True),
                 'serve(fused=True, prefill_chunk=%d)' % Cf: lambda: m.serve(prompts, budget, S, fused=True, prefill_chunk=Cf),
                 'generate_fused in static waves': lambda: waves(m.generate_fused)}
        v = sides_alternating(sides, wall_ms, a.serve_runs, 1)
        lines.append('(c) %d prompts (32 .. 256 tokens), budgets 16 .. 128 (%d tokens asked for), max_batch %d, wall ms, %d runs each after a warm-up run:'
                     % (N, sum(budget), S, a.serve_runs))
        lines += ['  %-40s %s' % (k, med(t)) for k, t in v.items()]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
      with open(a.out, 'a') as f:
        f.write(text)
    return

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
