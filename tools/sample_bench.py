"""Cost of sampling one new token at the 160M shape (12 layers, d = 768, 12 heads, V = 50280), B = 8, context 1024:
  a  the greedy cached step (Transformer.decode_step: the fused prediction head, no logits)
  b  the step with on-device sampling: decode_step(logits=True) + ops.sample_logits (temperature 0.8, top_k 50, top_p 0.95)
  c  the step through generate's sample= route (decode_step(logits=True) + generate.sampled) with a conventional torch sampler:
     temperature, top-k through torch.topk, a sort-based nucleus, torch.multinomial
  d  the sampling launch alone at V = 50280, per filter setting
All alternate in one process, random weights (the model's own init) and random tokens, HIP events around each call, median of --runs
after --warmup.  Also the host time to enqueue what b adds to the logits step (the sampling launch), and the same for c's sampler.
Usage: python tools/sample_bench.py [--runs 20] [--out profiles/sample_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plainlm_amd import ModelConfig, Transformer, generate as G, ops  # noqa: E402

B, CTX, SEQ = 8, 1024, 1028
TAU, TOP_K, TOP_P = 0.8, 50, 0.95


def timed(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1)


def host(fn):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  fn()
  h = (time.perf_counter() - t0) * 1e3
  torch.cuda.synchronize()
  return h


def med(v):
  return '%.3f [%.3f %.3f]' % (statistics.median(v), min(v), max(v))


def torch_sampler(logits):
  """The customary few lines: fp32 logits [B, V] -> int64 [B]."""
  z = logits / TAU
  kth = torch.topk(z, TOP_K, dim=-1).values[:, -1:]
  z = z.masked_fill(z < kth, float('-inf'))
  sz, idx = torch.sort(z, dim=-1, descending=True)
  pr = torch.softmax(sz, dim=-1)
  before = torch.cumsum(pr, dim=-1) - pr
  sz = sz.masked_fill(before >= TOP_P, float('-inf'))
  z = torch.full_like(z, float('-inf')).scatter(1, idx, sz)
  return torch.multinomial(torch.softmax(z, dim=-1), 1)[:, 0]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  torch.manual_seed(0)
  cfg = ModelConfig(vocab_size=50280, seq_len=SEQ, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu')
  m = Transformer(cfg).cuda()
  tok = torch.randint(0, cfg.vocab_size, (B, CTX + 4), device='cuda')
  lens = torch.full((B,), CTX, dtype=torch.int32, device='cuda')
  u = G.draw_uniforms(1, B, tok.device, seed=0)[0]
  with torch.no_grad():
    cache, _ = m.prefill(tok[:, :CTX].contiguous())
    nxt = tok[:, CTX].contiguous()

    def greedy():  # the same step every time: the cache is wound back to the context before it (outside the timed region)
      return m.decode_step(nxt, cache)

    def on_device():
      return ops.sample_logits(m.decode_step(nxt, cache, logits=True), u, TAU, TOP_K, TOP_P)

    def through_torch():
      return G.sampled(torch_sampler, m.decode_step(nxt, cache, logits=True))

    sides = (greedy, on_device, through_torch)
    t = [[] for _ in sides]
    for i in range(a.warmup + a.runs):
      for j, fn in enumerate(sides):
        cache.set_lens(lens)
        torch.cuda.synchronize()
        e = timed(fn)
        if i >= a.warmup:
          t[j].append(e)
    # the sampling stage alone on the logits of the step
    cache.set_lens(lens)
    logits = m.decode_step(nxt, cache, logits=True)
    alone = {}
    for name, (tau, k, p) in (('tau 0.8, top_k 50, top_p 0.95', (TAU, TOP_K, TOP_P)), ('tau 1, filters off', (1.0, 0, 1.0)),
                              ('tau 0.8, top_k 50', (TAU, TOP_K, 1.0)), ('tau 0.8, top_p 0.95', (TAU, 0, TOP_P))):
      alone[name] = [timed(lambda: ops.sample_logits(logits, u, tau, k, p)) for _ in range(a.warmup + a.runs)][a.warmup:]
    t_torch = [timed(lambda: G.sampled(torch_sampler, logits)) for _ in range(a.warmup + a.runs)][a.warmup:]
    h_dev = [host(lambda: ops.sample_logits(logits, u, TAU, TOP_K, TOP_P)) for _ in range(a.warmup + a.runs)][a.warmup:]
    h_torch = [host(lambda: G.sampled(torch_sampler, logits)) for _ in range(a.warmup + a.runs)][a.warmup:]
  ma, mb, mc = (statistics.median(v) for v in t)
  lines = [
    '# tools/sample_bench.py: 160M (12 layers, d 768, 12 heads, V 50280), B = %d, context %d; one process, sides alternating; ms, median of %d [min max]'
    % (B, CTX, a.runs),
    '(a) greedy cached step (fused prediction head)                          %s' % med(t[0]),
    '(b) step with on-device sampling (logits GEMM + plm_sample_logits_bf16) %s' % med(t[1]),
    '(c) step through sample= with a torch sampler (topk, sort, multinomial) %s' % med(t[2]),
    '(b) - (a)                                                               %.3f' % (mb - ma),
    '(c) - (b)                                                               %.3f' % (mc - mb),
    '(b) and (c) ranges disjoint, (b) below                                  %s' % (max(t[1]) < min(t[2])),
    'host time to enqueue the sampling launch of (b)                         %s' % med(h_dev),
    'host time to enqueue the sampler of (c) (cast, sampler, log_softmax)    %s' % med(h_torch),
    '(c)\'s sampler alone on the step\'s logits, device time                   %s' % med(t_torch),
  ]
  for name, v in alone.items():
    lines.append('(d) plm_sample_logits_bf16 alone, %-30s        %s' % (name, med(v)))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
