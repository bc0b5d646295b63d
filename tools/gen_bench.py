"""Cost of one new token at the 160M shape (12 layers, d = 768, 12 heads, V = 50280), B = 8, context 1024:
  C  one cached decode step (Transformer.decode_step on a cache prefilled with the context)
  R  predict(last_only=True) on the same full prefix: the recompute route, all there was before the cache
Both alternate in one process, random weights (the model's own init) and random tokens, HIP events around each call, median of --runs
after --warmup.  Also: the host time to enqueue C (its launches return before the kernels finish: a step that takes no longer than
its enqueue is launch-bound), the two new kernels alone (append; decode attention per split count), and whether C and R pick the
same tokens.
With --fused the two sides are the decode step as it is (U) and the fused one (F, decode_step(fused=True)): both
alternate in one process at the same shape (and at every --batch / --context given besides), HIP events, median of --runs with [min max];
per side the device time of a step, the host time to enqueue it, the library calls it makes (counted at _lib.check) and the kernel
launches they stand for (the per-entry-point counts of include/plainlm_hip.h, plus the one torch launch that moves the cache lengths).
With --fused-extend the sides are ``extend`` as it is and ``extend(fused=True)`` at (B, n) = (8, 4), (4, 8) and
(1, 32) on 1024 cached tokens, then one generate_lookup round against one generate_lookup_fused round at B = 4, n_draft = 7 (the round
of tools/lookup_bench.py: draft launch, the extend of n_draft + 1 rows, acceptance, commit_round and the cache move, on a periodic prompt
so that every round carries n_draft proposals), with the fused decode step at B = 8 beside them for scale: the same columns.
With --kv fp8 the sides are the two cache formats: one model, a bf16 cache and an FP8 cache prefilled with the same
tokens, the unfused and the fused decode step over each alternating in one process at (B, context) = (8, 1024), (8, 4096), (32, 1024),
(32, 4096), then extend(fused=True) at (B, n) = (8, 4) on 1024 cached tokens: device ms, median of --runs [min max], and per row whether the
FP8 side's [min max] lies wholly below the bf16 side's.
Usage: python tools/gen_bench.py [--runs 20] [--out profiles/generate_bench.txt]
       python tools/gen_bench.py --fused [--batch 1 32] [--context 4096] --out profiles/fused_decode_bench.txt
       python tools/gen_bench.py --fused-extend --out profiles/fused_extend_bench.txt
       python tools/gen_bench.py --kv fp8 --out profiles/kv8_bench.txt"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plainlm_amd import ModelConfig, Transformer, ops  # noqa: E402
from plainlm_amd import generate as G  # noqa: E402

B, CTX, SEQ = 8, 1024, 1028  # the timed step appends token number CTX + 1; the recompute route sees CTX + 4 rows (rows are 4 at a time)


def timed(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1)


def med(v):
  return '%.3f [%.3f %.3f]' % (statistics.median(v), min(v), max(v))


# kernel launches behind one call of an entry point at the decode shapes (include/plainlm_hip.h)
LAUNCHES = {'plm_attn_decode': 2, 'plm_head_predict_bf16': 2, 'plm_decode_layer_bf16': 6}


def alternate(sides, reset, a):
  """sides: {key: callable}, run alternately after reset() (outside the timed region).  Returns ({key: device ms}, {key: host enqueue
  ms}, {key: the library calls of one run, counted at _lib.check outside the timed runs}, {key: what that run returned})."""
  from plainlm_amd import _lib
  calls, ret, real = {}, {}, _lib.check
  for k, fn in sides.items():
    seen = []
    _lib.check = lambda rc, what: seen.append(what) or real(rc, what)
    try:
      reset()
      ret[k] = fn()
    finally:
      _lib.check = real
    calls[k] = seen
  dev, host = {k: [] for k in sides}, {k: [] for k in sides}
  for i in range(a.warmup + a.runs):
    for k, fn in sides.items():
      reset()
      torch.cuda.synchronize()
      e = timed(fn)
      reset()
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      fn()
      h = (time.perf_counter() - t0) * 1e3
      torch.cuda.synchronize()
      if i >= a.warmup:
        dev[k].append(e), host[k].append(h)
  return dev, host, calls, ret


def extend_launches(seen, nh, hd, n, B, Tmax):
  """Kernel launches behind the library calls of one extend (include/plainlm_hip.h): plm_attn_extend is two launches, one when it
  resolves to a single split (read off its workspace query: fp32 partials of 2 + hd per (row, head, split)); plm_extend_layer_bf16 is
  four more; the head is two."""
  from plainlm_amd import _lib
  one = (B * n * nh * (2 + hd) * 4 + 15) // 16 * 16
  ext = 1 if _lib.load().plm_attn_extend_workspace_bytes(B, n, nh, hd, Tmax, 0) == one else 2
  per = {'plm_attn_extend': ext, 'plm_extend_layer_bf16': 4 + ext, 'plm_head_predict_bf16': 2, 'plm_decode_layer_bf16': 6}
  return sum(per.get(w, 1) for w in seen)


def report(name, k, dev, host, calls, launches):
  return '  %-34s device %s   host enqueue %s   library calls %3d   kernel launches %s' % (name, med(dev[k]), med(host[k]), len(calls[k]), launches)


def verdict(dev, u, f):
  below = max(dev[f]) < min(dev[u])
  return 'U / F (medians) %.2f; F\'s [min max] lies %s U\'s' % (statistics.median(dev[u]) / statistics.median(dev[f]),
                                                                  'wholly below' if below else 'NOT wholly below')


class LookupRound:
  """One round of a _LookupSession run again and again from the same state (tools/lookup_bench.py's Round): reset() winds the cache, the
  lengths and the history back."""

  def __init__(self, session, cache, first, lens0, new):
    B = first.shape[0]
    self.s, self.cache, self.first, self.lens0 = session, cache, first, lens0
    self.live = torch.ones((B,), dtype=torch.bool, device='cuda')
    self.carry = torch.zeros((B,), dtype=torch.bool, device='cuda')
    self.out_tok = torch.zeros((B, new), dtype=torch.int64, device='cuda')
    self.out_lp = torch.zeros((B, new), dtype=torch.float32, device='cuda')
    self.count = torch.ones((B,), dtype=torch.int32, device='cuda')
    self.done = torch.zeros((B,), dtype=torch.bool, device='cuda')

  def reset(self):
    s = self.s
    self.cache.set_lens(self.lens0)
    s.tlen.copy_(self.lens0)
    s.hlen.copy_(self.lens0)
    s.round = 0
    s.add, s.n_add = self.first[:, None].contiguous(), None

  def __call__(self):
    s = self.s
    d, dout = s.draft_round(self.first, self.first, self.carry, self.live)
    res = s.accept(d, dout, s.target_round(self.first, d, self.live))
    _, _, moved = G.commit_round(self.out_tok, self.out_lp, self.count, self.done, d, *res)
    s.advance(moved, self.live)
    return s.n_prop.clone(), res[1]


def main_fused_extend(a):
  torch.manual_seed(0)
  room = 64  # cache rows beyond the context: a chunk of 32 rows, a lookup round of 8
  cfg = ModelConfig(vocab_size=50280, seq_len=CTX + room, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu')
  m = Transformer(cfg).cuda()
  nh = cfg.n_heads
  lines = ['# tools/gen_bench.py --fused-extend: 160M (12 layers, d 768, 12 heads, V 50280), %d cached tokens, cache of %d rows; one process, '
           'sides alternating; ms per call, HIP events, median of %d [min max]; host enqueue = wall time of the call, not waited for; kernel '
           'launches counted from the documented launch counts of the entry points, the one torch launch that moves the lengths included'
           % (CTX, CTX + room, a.runs)]
  with torch.no_grad():
    for Bx, n in ((8, 4), (4, 8), (1, 32)):
      tok = torch.randint(0, cfg.vocab_size, (Bx, CTX + n), device='cuda')
      lens = torch.full((Bx,), CTX, dtype=torch.int32, device='cuda')
      cache, _ = m.prefill(tok[:, :CTX].contiguous())
      chunk = tok[:, CTX:].contiguous()
      sides = {'U': lambda: m.extend(chunk, cache), 'F': lambda: m.extend(chunk, cache, fused=True)}
      dev, host, calls, ret = alternate(sides, lambda: cache.set_lens(lens), a)
      same = (ret['U'].tokens == ret['F'].tokens).float().mean().item()
      dlp = (ret['U'].logprob - ret['F'].logprob).abs().max().item()
      lines.append('extend, B = %d, n = %d (%d chunk rows)' % (Bx, n, Bx * n))
      for k, name in (('U', 'extend as it is (U)'), ('F', 'extend(fused=True) (F)')):
        lines.append(report(name, k, dev, host, calls, '%3d' % (1 + extend_launches(calls[k], nh, m.head_dim, n, Bx, cache.Tmax))))
      lines.append('  %s; same greedy token %.3f of %d sequences, max |dlogp| %.2e' % (verdict(dev, 'U', 'F'), same, Bx, dlp))
      del cache
    # a lookup round, B = 4, n_draft = 7, on a periodic prompt: every round carries n_draft proposals
    Bx, k, new = 4, 7, 64
    block = torch.randint(0, cfg.vocab_size, (Bx, 37), device='cuda')
    prompt = block.repeat(1, CTX // 37 + 1)[:, :CTX].contiguous()
    lens0 = torch.full((Bx,), CTX, dtype=torch.int32, device='cuda')
    first = prompt[:, CTX - 37].contiguous()  # the token the block continues with: the lookup matches the whole suffix
    cache, _ = m.prefill(prompt)
    rounds = {key: LookupRound(G._LookupSession(m, cache, prompt, first, k, (1, 4), new, None, None, fused=fused), cache, first, lens0, new)
              for key, fused in (('U', False), ('F', True))}
    dev, host, calls, ret = alternate(rounds, lambda: [r.reset() for r in rounds.values()], a)
    lines.append('lookup round, greedy, B = %d, n_draft = %d (%d chunk rows)' % (Bx, k, Bx * (k + 1)))
    for key, name in (('U', 'generate_lookup round (U)'), ('F', 'generate_lookup_fused round (F)')):
      lines.append(report(name, key, dev, host, calls, '%3d + torch\'s own' % extend_launches(calls[key], nh, m.head_dim, k + 1, Bx, cache.Tmax)))
    lines.append('  %s; proposals per sequence in the timed round U %s, F %s; same next token %.3f of %d sequences'
                 % (verdict(dev, 'U', 'F'), ret['U'][0].tolist(), ret['F'][0].tolist(), (ret['U'][1] == ret['F'][1]).float().mean().item(), Bx))
    del cache, rounds
    # for scale: the fused decode step at B = 8 (tools/gen_bench.py --fused), in this process
    tok = torch.randint(0, cfg.vocab_size, (B, CTX + 4), device='cuda')
    lens = torch.full((B,), CTX, dtype=torch.int32, device='cuda')
    cache, _ = m.prefill(tok[:, :CTX].contiguous())
    nxt = tok[:, CTX].contiguous()
    dev, host, calls, _ = alternate({'D': lambda: m.decode_step(nxt, cache, fused=True)}, lambda: cache.set_lens(lens), a)
    lines.append('for scale: fused decode step, B = %d' % B)
    lines.append(report('decode_step(fused=True)', 'D', dev, host, calls, '%3d' % (1 + sum(LAUNCHES.get(w, 1) for w in calls['D']))))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'w') as f:
      f.write(text)


def fused_side_by_side(m, a, batch, ctx):
  """One row of the --fused report: U and F alternating at batch x ctx.  Returns the report lines."""
  cfg = m.cfg
  tok = torch.randint(0, cfg.vocab_size, (batch, ctx + 4), device='cuda')
  lens = torch.full((batch,), ctx, dtype=torch.int32, device='cuda')
  with torch.no_grad():
    cache, _ = m.prefill(tok[:, :ctx].contiguous(), max_len=ctx + 4)
    nxt = tok[:, ctx].contiguous()
    sides = {'U': lambda: m.decode_step(nxt, cache), 'F': lambda: m.decode_step(nxt, cache, fused=True)}
    dev, host, seen, ret = alternate(sides, lambda: cache.set_lens(lens), a)
  calls = {k: (len(seen[k]), 1 + sum(LAUNCHES.get(w, 1) for w in seen[k])) for k in sides}
  same = (ret['U'].tokens == ret['F'].tokens).float().mean().item()
  dlp = (ret['U'].logprob - ret['F'].logprob).abs().max().item()
  name = {'U': 'decode step as it is (U)', 'F': 'fused decode step (F)   '}
  out = ['B = %d, context %d' % (batch, ctx)]
  for k in sides:
    out.append('  %s  device %s   host enqueue %s   library calls %3d   kernel launches %3d'
               % (name[k], med(dev[k]), med(host[k]), calls[k][0], calls[k][1]))
  below = max(dev['F']) < min(dev['U'])
  out.append('  U / F (medians) %.2f; F\'s [min max] lies %s U\'s; same greedy token %.3f of %d sequences, max |dlogp| %.2e'
             % (statistics.median(dev['U']) / statistics.median(dev['F']), 'wholly below' if below else 'NOT wholly below', same, batch, dlp))
  return out


def main_fused(a):
  torch.manual_seed(0)
  ctxs = [CTX] + [c for c in a.context if c != CTX]
  cfg = ModelConfig(vocab_size=50280, seq_len=max(ctxs) + 4, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu')
  m = Transformer(cfg).cuda()
  lines = ['# tools/gen_bench.py --fused: 160M (12 layers, d 768, 12 heads, V 50280); one process, sides alternating; ms per step, HIP events, '
           'median of %d [min max]; host enqueue = wall time of the call, not waited for' % a.runs]
  for batch, ctx in [(B, CTX)] + [(b, CTX) for b in a.batch if b != B] + [(B, c) for c in ctxs[1:]]:
    lines += fused_side_by_side(m, a, batch, ctx)
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'w') as f:
      f.write(text)


def main_kv(a):
  torch.manual_seed(0)
  shapes = [(8, 1024), (8, 4096), (32, 1024), (32, 4096)]
  room = 8
  cfg = ModelConfig(vocab_size=50280, seq_len=max(c for _, c in shapes) + room, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu')
  m = Transformer(cfg).cuda()
  lines = ['# tools/gen_bench.py --kv %s: 160M (12 layers, d 768, 12 heads, V 50280); one model, a bf16 and an %s KV cache prefilled with the '
           'same tokens; one process, sides alternating; device ms per call, HIP events, median of %d [min max]; "below": the %s side\'s '
           '[min max] lies wholly below the bf16 side\'s' % (a.kv, a.kv, a.runs, a.kv)]

  def row(name, dev, b, f):
    below = max(dev[f]) < min(dev[b])
    return '  %-22s bf16 %s   %s %s   bf16 / %s (medians) %.2f; %s' % (name, med(dev[b]), a.kv, med(dev[f]), a.kv,
                                                                     statistics.median(dev[b]) / statistics.median(dev[f]),
                                                                     'below' if below else 'NOT below')
  with torch.no_grad():
    for batch, ctx in shapes:
      tok = torch.randint(0, cfg.vocab_size, (batch, ctx + 4), device='cuda')
      lens = torch.full((batch,), ctx, dtype=torch.int32, device='cuda')
      caches = {kv: m.prefill(tok[:, :ctx].contiguous(), max_len=ctx + room, kv_dtype=kv)[0] for kv in ('bf16', a.kv)}
      nxt = tok[:, ctx].contiguous()
      sides = {(kv, fused): (lambda kv=kv, fused=fused: m.decode_step(nxt, caches[kv], fused=fused)) for fused in (False, True) for kv in caches}
      dev, _, _, ret = alternate(sides, lambda: [c.set_lens(lens) for c in caches.values()], a)
      lines.append('B = %d, context %d: cache bytes per layer bf16 %d, %s %d' % (batch, ctx, caches['bf16'].kv[0].numel() * 2, a.kv,
                                                                                 caches[a.kv].kv[0].numel()))
      for fused, name in ((False, 'decode step'), (True, 'fused decode step')):
        same = (ret[('bf16', fused)].tokens == ret[(a.kv, fused)].tokens).float().mean().item()
        lines.append(row(name, dev, ('bf16', fused), (a.kv, fused)) + '; same greedy token %.3f of %d' % (same, batch))
      if (batch, ctx) == (8, 1024):
        chunk = tok[:, ctx:ctx + 4].contiguous()
        sides = {kv: (lambda kv=kv: m.extend(chunk, caches[kv], fused=True)) for kv in caches}
        dev, _, _, _ = alternate(sides, lambda: [c.set_lens(lens) for c in caches.values()], a)
        lines.append(row('extend(fused), n = 4', dev, 'bf16', a.kv))
      del caches
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'w') as f:
      f.write(text)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  ap.add_argument('--fused', action='store_true', help='compare the fused decode step with the decode step as it is')
  ap.add_argument('--batch', type=int, nargs='*', default=[], help='--fused: extra batch sizes at context %d' % CTX)
  ap.add_argument('--context', type=int, nargs='*', default=[], help='--fused: extra contexts at B = %d' % B)
  ap.add_argument('--fused-extend', action='store_true', help='compare extend(fused=True) and a generate_lookup_fused round with the unfused ones')
  ap.add_argument('--kv', choices=['fp8'], default=None, help='compare the decode steps over an FP8 KV cache with those over the bf16 cache')
  a = ap.parse_args()
  if a.kv:
    return main_kv(a)
  if a.fused:
    return main_fused(a)
  if a.fused_extend:
    return main_fused_extend(a)
  torch.manual_seed(0)
  cfg = ModelConfig(vocab_size=50280, seq_len=SEQ, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu')
  m = Transformer(cfg).cuda()
  tok = torch.randint(0, cfg.vocab_size, (B, CTX + 4), device='cuda')
  lens = torch.full((B,), CTX, dtype=torch.int32, device='cuda')
  with torch.no_grad():
    cache, first = m.prefill(tok[:, :CTX].contiguous())
    nxt = tok[:, CTX].contiguous()

    def step():  # the same step every time: the cache is wound back to the context before it (outside the timed region)
      return m.decode_step(nxt, cache)

    def recompute():  # the prefix + the new token, right-padded to the kernels' 4 rows: the prediction after token CTX + 1 is row CTX
      return m.predict(tok)

    def recompute_last():
      return m.predict(tok, last_only=True)

    r_c = step()
    r_r = recompute()
    same = (r_c.tokens == r_r.tokens[:, CTX]).float().mean().item()
    dlp = (r_c.logprob - r_r.logprob[:, CTX]).abs().max().item()
    tc, tr, th = [], [], []
    for i in range(a.warmup + a.runs):
      cache.set_lens(lens)
      torch.cuda.synchronize()
      e = timed(step)
      # enqueue time: a second step, not waited for
      cache.set_lens(lens)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      step()
      h = (time.perf_counter() - t0) * 1e3
      torch.cuda.synchronize()
      r = timed(recompute_last)
      if i >= a.warmup:
        tc.append(e), tr.append(r), th.append(h)
    # the two new kernels alone, at this shape
    nh, hd = cfg.n_heads, m.head_dim
    rope = m._rope(tok.device)
    qkv = torch.randn(B, 3 * cfg.dim, device='cuda').to(torch.bfloat16)
    pos = lens.clone()
    ta = [timed(lambda: ops.kv_append_rope(qkv, pos, rope[0], rope[1], cache.kv[0], nh, status=cache.status)) for _ in range(a.warmup + a.runs)][a.warmup:]
    q = torch.randn(B, cfg.dim, device='cuda').to(torch.bfloat16)
    full = torch.full((B,), CTX + 1, dtype=torch.int32, device='cuda')
    ks = {}
    for s in (0, 1, 2, 4, 8, 16, 32, 64):
      ks[s] = [timed(lambda: ops.attn_decode(q, cache.kv[0], full, nh, splits=s)) for _ in range(a.warmup + a.runs)][a.warmup:]
  launches = 2 + 10 * cfg.n_layers + 1 + 2  # lens += 1, embedding; per layer 2 norms, 4 GEMMs, append, 2 decode, activation; out norm; head (2)
  mc, mr = statistics.median(tc), statistics.median(tr)
  kv_bytes = B * (CTX + 1) * 2 * cfg.dim * 2
  lines = [
    '# tools/gen_bench.py: 160M (12 layers, d 768, 12 heads, V 50280), B = %d, context %d; one process, sides alternating; ms, median of %d [min max]' % (B, CTX, a.runs),
    'cached decode step (C)                       %s' % med(tc),
    'predict(last_only=True) on the prefix (R)    %s' % med(tr),
    'R / C                                        %.2f' % (mr / mc),
    'host time to enqueue C (%d launches)        %s' % (launches, med(th)),
    'C and R choose the same token                %.3f of %d sequences (max |dlogp| %.2e; random weights: near-uniform logits)' % (same, B, dlp),
    'plm_kv_append_rope alone                     %s' % med(ta),
  ]
  for s, v in ks.items():
    lines.append('plm_attn_decode alone, splits = %-2s %s       %s   (%.0f GB/s of k | v)'
                 % (s, '(auto)' if s == 0 else '      ', med(v), kv_bytes / statistics.median(v) / 1e6))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
