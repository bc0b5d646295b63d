"""Cost of one round of draft-free speculative decoding at the 160M shape (12 layers, d = 768, 12 heads,
V = 50280), B = 8, context 1024, by tools/gen_bench.py's method: one process, the sides alternating, HIP events around each call,
median of --runs after --warmup with min and max.
  D  one cached decode step (Transformer.decode_step)
  L  one generate_lookup round at n_draft = 4 / 8 / 16, greedy and sampled (0.8 / top-50): the ops.lookup_draft launch, the extend of
     n_draft + 1 rows, acceptance, commit_round and the cache move - everything speculative_loop does per round but its one host read
  S  one generate_speculative round at n_draft = 4 with a 2-layer draft of the same width, greedy and sampled
The prompt is a 37-token block repeated, so that every lookup finds a match and every round of L carries n_draft proposals (a round
without a proposal runs the same launches on padded rows).  Also: the library calls of a round by entry point, the kernels torch's
profiler counts in it (when it can), the host time to enqueue a round, the two new kernels alone, and tokens per round and accepted /
drafted for whole generate_lookup calls on this random-init model - which say nothing about text: a random model's continuation of a
periodic prompt is not periodic, and its continuation of random tokens repeats nothing.
Usage: python tools/lookup_bench.py [--runs 20] [--out profiles/lookup_bench.txt]"""
import argparse
import collections
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plainlm_amd import ModelConfig, Transformer, _lib, ops  # noqa: E402
from plainlm_amd import generate as G  # noqa: E402

B, CTX, NEW, SEQ = 8, 1024, 64, 1024 + 64 + 32
KS = (4, 8, 16)
SAMPLING = (0.8, 50, 1.0)


def timed(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1)


def med(v):
  return '%.3f [%.3f %.3f]' % (statistics.median(v), min(v), max(v))


class Counting:
  """The loaded library with its plm_* calls counted by name."""

  def __init__(self, lib):
    self.lib, self.calls = lib, collections.Counter()

  def __getattr__(self, name):
    fn = getattr(self.lib, name)
    if not name.startswith('plm_') or name == 'plm_last_error_string':
      return fn

    def counted(*a):
      self.calls[name] += 1
      return fn(*a)
    return counted


class Round:
  """One round of a session, run again and again from the same state: reset() winds the caches, the lengths and the history back."""

  def __init__(self, session, caches, first, k, lens0):
    self.s, self.caches, self.first, self.k, self.lens0 = session, caches, first, k, lens0
    self.live = torch.ones((B,), dtype=torch.bool, device='cuda')
    self.carry = torch.zeros((B,), dtype=torch.bool, device='cuda')
    self.out_tok = torch.zeros((B, NEW), dtype=torch.int64, device='cuda')
    self.out_lp = torch.zeros((B, NEW), dtype=torch.float32, device='cuda')
    self.count = torch.ones((B,), dtype=torch.int32, device='cuda')
    self.done = torch.zeros((B,), dtype=torch.bool, device='cuda')
    self.n_prop = None

  def reset(self):
    s = self.s
    for c in self.caches:
      c.set_lens(self.lens0)
    s.tlen.copy_(self.lens0)
    s.round = 0
    if hasattr(s, 'dlen'):
      s.dlen.copy_(self.lens0)
    else:
      s.hlen.copy_(self.lens0)
      s.add, s.n_add = self.first[:, None].contiguous(), None

  def __call__(self):
    s = self.s
    d, dout = s.draft_round(self.first, self.first, self.carry, self.live)
    res = s.accept(d, dout, s.target_round(self.first, d, self.live))
    _, _, moved = G.commit_round(self.out_tok, self.out_lp, self.count, self.done, d, *res)
    s.advance(moved, self.live)
    self.n_prop = getattr(s, 'n_prop', None)


def kernels_in(fn):
  """Device kernels torch's profiler sees in one call of fn, or None when it cannot tell."""
  try:
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
      fn()
      torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA'))
    return n or None
  except Exception:  # noqa: BLE001  a profiler that does not work here is no reason to lose the timings
    return None


def write(lines, out):
  text = '\n'.join(lines) + '\n'
  if out:
    with open(out, 'w') as f:
      f.write(text)
  return text


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  torch.manual_seed(0)
  cfg = ModelConfig(vocab_size=50280, seq_len=SEQ, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu')
  m = Transformer(cfg).cuda()
  draft = Transformer(ModelConfig(vocab_size=50280, seq_len=SEQ, dim=768, expand=8 / 3, n_layers=2, n_heads=12, mlp='glu')).cuda()
  block = torch.randint(0, cfg.vocab_size, (B, 37), device='cuda')
  prompt = block.repeat(1, CTX // 37 + 1)[:, :CTX].contiguous()
  rand_prompt = torch.randint(0, cfg.vocab_size, (B, CTX), device='cuda')
  lens0 = torch.full((B,), CTX, dtype=torch.int32, device='cuda')
  first = prompt[:, CTX - 37].contiguous()  # the token the block continues with: the lookup matches the whole suffix
  lines = ['# tools/lookup_bench.py: 160M (12 layers, d 768, 12 heads, V 50280), B = %d, context %d; one process, sides alternating; ms, median of '
           '%d [min max]' % (B, CTX, a.runs)]
  with torch.no_grad():
    cache, _ = m.prefill(prompt)
    dcache, _ = draft.prefill(prompt)
    sides = collections.OrderedDict()
    sides['D  decode step'] = (lambda: m.decode_step(first, cache), lambda: cache.set_lens(lens0))
    rounds = {}
    for sampling in (None, SAMPLING):
      tag = 'greedy ' if sampling is None else 'sampled'
      for k in KS:
        u = None if sampling is None else G.lookup_uniforms(NEW, k, B, 'cuda', seed=1)
        r = Round(G._LookupSession(m, cache, prompt, first, k, (1, 4), NEW, sampling, u), [cache], first, k, lens0)
        rounds['L', tag, k] = r
        sides['L  lookup round, %s, n_draft = %-2d' % (tag, k)] = (r, r.reset)
      u = None if sampling is None else G.speculative_uniforms(NEW, 4, B, 'cuda', seed=1)
      r = Round(G._SpecSession(m, draft, cache, dcache, 4, sampling, u), [cache, dcache], first, 4, lens0)
      rounds['S', tag, 4] = r
      sides['S  speculative round (2-layer draft), %s, n_draft = 4 ' % tag] = (r, r.reset)
    times = {name: [] for name in sides}
    host = {name: [] for name in sides}
    for i in range(a.warmup + a.runs):
      for name, (fn, reset) in sides.items():
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
          times[name].append(e), host[name].append(h)
    d_ms = statistics.median(times['D  decode step'])
    for name in sides:
      lines.append('%-62s %s   %.2f x D   host enqueue %s' % (name, med(times[name]), statistics.median(times[name]) / d_ms, med(host[name])))
    for (side, tag, k), r in rounds.items():
      if side == 'L':
        assert r.n_prop.tolist() == [k] * B, (tag, k, r.n_prop.tolist())
    lines.append('every timed lookup round carried n_draft proposals per sequence (n_prop = n_draft)')
    # the launches of a round
    counting = Counting(_lib.load())
    _lib._lib = counting
    try:
      for key in (('L', 'greedy ', 8), ('L', 'sampled', 8), ('S', 'greedy ', 4), ('S', 'sampled', 4)):
        r = rounds[key]
        r.reset()
        counting.calls.clear()
        r()
        torch.cuda.synchronize()
        calls = dict(counting.calls)
        lines.append('%s round, %s, n_draft = %d: %d library calls: %s'
                     % ('lookup' if key[0] == 'L' else 'speculative', key[1].strip(), key[2], sum(calls.values()),
                        ', '.join('%s x%d' % (n[4:], c) for n, c in sorted(calls.items()))))
      cache.set_lens(lens0)
      counting.calls.clear()
      m.decode_step(first, cache)
      lines.append('decode step: %d library calls' % sum(counting.calls.values()))
    finally:
      _lib._lib = counting.lib
    # the two new kernels alone
    for k in KS:
      hist = torch.zeros((B, CTX + NEW), dtype=torch.int64, device='cuda')
      hist[:, :CTX] = prompt
      add = first[:, None].contiguous()
      hl = lens0.clone()
      t = []
      for _ in range(a.warmup + a.runs):
        hl.copy_(lens0)
        t.append(timed(lambda: ops.lookup_draft(hist, hl, add, None, k=k, ngram=(1, 4))))
      logits = torch.randn(B * (k + 1), cfg.vocab_size, device='cuda').to(torch.bfloat16)
      st = ops.sample_logits(logits, torch.rand(B * (k + 1), device='cuda'), *SAMPLING, want_stats=True)
      dt = st.tokens.view(B, k + 1)[:, :k].contiguous()   # the sampler's own token: inside the kept set, so a full pass over the row
      n_prop = torch.full((B,), k, dtype=torch.int32, device='cuda')
      ua, ur = torch.rand(k, B, device='cuda'), torch.rand(B, device='cuda')
      tv = [timed(lambda: ops.spec_verify_lookup(logits, dt, n_prop, st.cutoff, st.tokens, ua, ur, SAMPLING[0]))
            for _ in range(a.warmup + a.runs)][a.warmup:]
      lines.append('plm_lookup_draft_i64 alone (history %d, k = %-2d)  %s     plm_spec_verify_lookup_bf16 alone (k = %-2d, 2 launches)  %s'
                   % (CTX + 1, k, med(t[a.warmup:]), k, med(tv)))
    # whole calls on the random-init model: this says nothing about text
    lines.append('# whole generate_lookup calls, %d new tokens, n_draft = 8, ngram (1, 4), random-init weights: this says NOTHING about text' % NEW)
    for pname, p in (('periodic prompt (37-token block)', prompt), ('random prompt', rand_prompt)):
      for tag, kw in (('greedy ', {}), ('sampled', dict(temperature=SAMPLING[0], top_k=SAMPLING[1], seed=3))):
        _, stats = m.generate_lookup(p, NEW, n_draft=8, return_stats=True, **kw)
        dr, ac = stats['drafted'].sum().item(), stats['accepted'].sum().item()
        lines.append('%-34s %s  %2d rounds (of the slowest sequence), %.2f tokens per round, %d of %d proposals accepted (%.3f)'
                     % (pname, tag, stats['rounds'], (NEW - 1) / max(stats['rounds'], 1), ac, dr, ac / max(dr, 1)))
    write(lines, a.out)
    # device kernels per round, torch's own included, as torch's profiler counts them: last, so that a profiler that fails loses nothing
    cache.set_lens(lens0)
    counts = [('decode step', kernels_in(lambda: m.decode_step(first, cache)))]
    for key in (('L', 'greedy ', 8), ('L', 'sampled', 8), ('S', 'greedy ', 4), ('S', 'sampled', 4)):
      rounds[key].reset()
      counts.append(('%s round, %s, n_draft = %d' % ('lookup' if key[0] == 'L' else 'speculative', key[1].strip(), key[2]), kernels_in(rounds[key])))
    lines.append('device kernels (torch\'s own included): ' + '; '.join('%s %s' % (n, 'n/a' if c is None else c) for n, c in counts))
  print(write(lines, a.out), end='')


if __name__ == '__main__':
  main()
