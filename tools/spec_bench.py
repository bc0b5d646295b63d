"""Cost of one speculative round at the 160M shape (12 layers, d = 768, 12 heads, V = 50280), B = 8, context 1024,
with a 2-layer draft of the same width, against the plain cached decode step in the same process, sides alternating:
  S  one decode step of the target (Transformer.decode_step, as tools/gen_bench.py times it)
  R  one round of Transformer.generate_speculative per n_draft in {2, 4, 8}: the draft's k steps, the target's extend of k + 1 rows,
     acceptance, the bookkeeping and both cache moves - greedy, and sampled (0.8 / top-k 50 / top-p 0.95) - with the per-round read of
     the finished flag and without it
  plm_spec_verify_bf16 alone at B = 8, V = 50280, on random rows (q = p + noise), all accepted and rejected at row 0
The break-even is R / S: the mean number of tokens a round must yield (accepted + 1) to match plain decoding.  Random weights (the
models' own init) and random tokens: the acceptance of a random draft says nothing about text; the self-draft acceptance (draft = the
target's own weights) shows how often two routes to the same logits agree.
HIP events around the round loop, divided by its rounds; median of --runs after --warmup.
Usage: python tools/spec_bench.py [--runs 7] [--out profiles/spec_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plainlm_amd import ModelConfig, Transformer, ops  # noqa: E402
from plainlm_amd import generate as G  # noqa: E402

B, CTX, N, N_SELF, V = 8, 1024, 17, 33, 50280   # N - 1 = 16 rounds per call: a random draft is accepted almost never
SEQ = CTX + N_SELF + 8 + 1 + 6                  # the longest call's prompt + new tokens + n_draft + 1, rounded up to the kernels' 4 rows
SAMPLING = dict(temperature=0.8, top_k=50, top_p=0.95)


def timed(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1)


def med(v):
  return '%.3f [%.3f %.3f]' % (statistics.median(v), min(v), max(v))


def round_ms(target, draft, prompt, k, read, **kw):
  """ms per round of one generate_speculative call (the prefills are outside the events), and its statistics."""
  real, got = G.speculative_loop, {}

  def loop(*a, **k2):
    if not read:
      k2['all_done'] = lambda d: False   # the loop then runs its N - 1 rounds whatever happens
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = real(*a, **k2)
    e1.record()
    got['ev'], got['rounds'] = (e0, e1), r[2]['rounds']
    return r
  G.speculative_loop = loop
  try:
    _, stats = target.generate_speculative(prompt, N, draft, n_draft=k, seed=1, return_stats=True, **kw)
  finally:
    G.speculative_loop = real
  got['ev'][1].synchronize()
  return got['ev'][0].elapsed_time(got['ev'][1]) / max(got['rounds'], 1), stats


def verify_inputs(k, same):
  g = torch.Generator(device='cuda').manual_seed(k)
  xp = (torch.randn(B * (k + 1), V, generator=g, device='cuda') * 2).to(torch.bfloat16)
  xq = xp.view(B, k + 1, V)[:, :k].transpose(0, 1).reshape(k * B, V).contiguous()
  if not same:
    xq = (xq.float() + 4 * torch.randn(k * B, V, generator=g, device='cuda')).to(torch.bfloat16)
  u = lambda *s: torch.rand(*s, generator=g, device='cuda')  # noqa: E731
  st = ops.sample_logits(xp, u(B * (k + 1)), want_stats=True, **SAMPLING)
  sq = ops.sample_logits(xq, u(k * B), want_stats=True, **SAMPLING)
  return (xp, xq, sq.tokens.view(k, B), st.cutoff, sq.cutoff, st.tokens, u(k, B), u(B), SAMPLING['temperature'])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  torch.manual_seed(0)
  shape = dict(vocab_size=V, seq_len=SEQ, dim=768, expand=8 / 3, n_heads=12, mlp='glu')
  target = Transformer(ModelConfig(n_layers=12, **shape)).cuda()
  draft = Transformer(ModelConfig(n_layers=2, **shape)).cuda()
  prompt = torch.randint(0, V, (B, CTX), device='cuda')
  lens = torch.full((B,), CTX, dtype=torch.int32, device='cuda')
  modes = [('greedy', {}), ('sampled', SAMPLING)]
  ks = (2, 4, 8)
  t_step = []
  t_round = {(k, name, read): [] for k in ks for name, _ in modes for read in (True, False)}
  acc = {}
  with torch.no_grad():
    cache, _ = target.prefill(prompt, max_len=SEQ)
    nxt = prompt[:, 0].contiguous()
    for i in range(a.warmup + a.runs):
      for key in t_round:   # sides alternating: a plain step between any two rounds' calls
        cache.set_lens(lens)
        torch.cuda.synchronize()
        s = timed(lambda: target.decode_step(nxt, cache))
        k, name, read = key
        r, stats = round_ms(target, draft, prompt, k, read, **dict(modes)[name])
        if i >= a.warmup:
          t_step.append(s)
          t_round[key].append(r)
          acc[key] = (stats['accepted'].sum().item(), stats['drafted'].sum().item())
    # the self-draft: the target's own weights in a second module
    twin = Transformer(ModelConfig(n_layers=12, **shape)).cuda()
    twin.load_state_dict(target.state_dict())
    selfacc = {}
    for name, kw in modes:
      for k in ks:
        _, stats = target.generate_speculative(prompt, 33, twin, n_draft=k, seed=2, return_stats=True, **kw)
        selfacc[name, k] = (stats['accepted'].sum().item(), stats['drafted'].sum().item(), stats['rounds'])
    del twin
    t_verify = {}
    for k in ks:
      for same in (True, False):
        inp = verify_inputs(k, same)
        n_acc = ops.spec_verify(*inp).n_accept.float().mean().item()
        t_verify[k, same] = ([timed(lambda: ops.spec_verify(*inp)) for _ in range(a.warmup + 20)][a.warmup:], n_acc)
  ms = statistics.median(t_step)
  lines = ['# tools/spec_bench.py: target 160M (12 layers, d 768, 12 heads, V 50280), draft 2 layers of the same width, B = %d, context %d; one '
           'process, sides alternating; ms, median of %d [min max]; a round = the loop\'s time / its %d rounds' % (B, CTX, a.runs, N - 1),
           'plain cached decode step of the target (S)                         %s' % med(t_step)]
  for k in ks:
    for name, _ in modes:
      w, wo = t_round[k, name, True], t_round[k, name, False]
      mw = statistics.median(w)
      lines.append('round, n_draft = %d, %-7s with the per-round read (R)          %s   break-even R / S = %.2f tokens per round'
                   % (k, name, med(w), mw / ms))
      lines.append('round, n_draft = %d, %-7s without the read                     %s   the read costs %+.3f'
                   % (k, name, med(wo), mw - statistics.median(wo)))
      lines.append('    accepted / drafted with the random 2-layer draft: %d / %d' % acc[k, name, True])
  for k in ks:
    for same in (True, False):
      v, n_acc = t_verify[k, same]
      lines.append('plm_spec_verify_bf16 alone, k = %d, %-22s              %s   (mean n_accept %.2f)'
                   % (k, 'q = p (all accepted)' if same else 'q = p + noise', med(v), n_acc))
  for (name, k), (x, d, r) in selfacc.items():
    lines.append('self-draft (the target\'s own weights), %-7s n_draft = %d: %d of %d drafted tokens accepted (%.3f), %d rounds for 33 tokens'
                 % (name, k, x, d, x / max(d, 1), r))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
