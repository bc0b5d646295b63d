"""Cost of appending a chunk of tokens to a live cache at the 160M shape (12 layers, d = 768, 12 heads, V = 50280), B = 8, 1024 cached
tokens (the setup of tools/gen_bench.py):
  E8 / D8     Transformer.extend with n = 8 against 8 Transformer.decode_step calls that append the same 8 tokens
  E128 / P    Transformer.extend with n = 128 against Transformer.prefill of the whole 1152-token sequence
  kernels     plm_attn_extend alone at n = 1, 8 and 128 (automatic splits) against plm_attn_decode; plm_kv_append_rope_rows alone
The sides of a pair alternate in one process, random weights (the model's own init) and random tokens, HIP events around each call,
median of --runs after --warmup with min and max.  The cache is wound back to 1024 tokens before every timed call, outside the timed
region.  Also the host time to enqueue E8 (its launches return before the kernels finish).
Usage: python tools/extend_bench.py [--runs 20] [--out profiles/extend_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plainlm_amd import ModelConfig, Transformer, ops  # noqa: E402

B, CTX, SEQ = 8, 1024, 1152


def timed(fn):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  fn()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1)


def med(v):
  return '%.3f [%.3f %.3f]' % (statistics.median(v), min(v), max(v))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  torch.manual_seed(0)
  cfg = ModelConfig(vocab_size=50280, seq_len=SEQ, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu')
  m = Transformer(cfg).cuda()
  tok = torch.randint(0, cfg.vocab_size, (B, SEQ), device='cuda')
  lens = torch.full((B,), CTX, dtype=torch.int32, device='cuda')
  nh, hd = cfg.n_heads, m.head_dim
  with torch.no_grad():
    cache, _ = m.prefill(tok[:, :CTX].contiguous(), max_len=SEQ)
    chunk8 = tok[:, CTX:CTX + 8].contiguous()
    chunk128 = tok[:, CTX:CTX + 128].contiguous()
    cols8 = [chunk8[:, i].contiguous() for i in range(8)]

    def rewind():
      cache.set_lens(lens)
      torch.cuda.synchronize()

    def e8():
      return m.extend(chunk8, cache)

    def d8():
      for t in cols8:
        r = m.decode_step(t, cache)
      return r

    def e128():
      return m.extend(chunk128, cache)

    def prefill():
      return m.prefill(tok, max_len=SEQ)[1]

    # the same next token from both routes of a pair?
    rewind()
    r_e = e8()
    rewind()
    r_d = d8()
    same8 = (r_e.tokens == r_d.tokens).float().mean().item()
    dlp8 = (r_e.logprob - r_d.logprob).abs().max().item()
    rewind()
    r_e = e128()
    r_p = prefill()
    same128 = (r_e.tokens == r_p.tokens).float().mean().item()
    dlp128 = (r_e.logprob - r_p.logprob).abs().max().item()
    cache.check()

    t_e8, t_d8, t_e128, t_p, t_h = [], [], [], [], []
    for i in range(a.warmup + a.runs):
      rewind()
      x = timed(e8)
      rewind()
      y = timed(d8)
      rewind()
      z = timed(e128)
      w = timed(prefill)
      rewind()
      t0 = time.perf_counter()
      e8()  # enqueue time: not waited for
      h = (time.perf_counter() - t0) * 1e3
      torch.cuda.synchronize()
      if i >= a.warmup:
        t_e8.append(x), t_d8.append(y), t_e128.append(z), t_p.append(w), t_h.append(h)
    # one decode step alone, for the "about one decode step" expectation
    t_d1 = []
    for i in range(a.warmup + a.runs):
      rewind()
      t_d1.append(timed(lambda: m.decode_step(cols8[0], cache)))
    t_d1 = t_d1[a.warmup:]

    # the kernels alone, layer 0's cache, every sequence at 1024 + n keys
    rope = m._rope(tok.device)
    n_runs = a.warmup + a.runs
    q1 = torch.randn(B, cfg.dim, device='cuda').to(torch.bfloat16)
    full = torch.full((B,), CTX + 1, dtype=torch.int32, device='cuda')
    t_dec = [timed(lambda: ops.attn_decode(q1, cache.kv[0], full, nh)) for _ in range(n_runs)][a.warmup:]
    t_ext, t_app = {}, {}
    for n in (1, 8, 128):
      q = torch.randn(B * n, cfg.dim, device='cuda').to(torch.bfloat16)
      qkv = torch.randn(B * n, 3 * cfg.dim, device='cuda').to(torch.bfloat16)
      ws = ops.attn_extend_workspace(B, n, nh, hd, SEQ, 0, q.device)
      t_ext[n] = [timed(lambda: ops.attn_extend(q, cache.kv[0], lens, nh, workspace=ws)) for _ in range(n_runs)][a.warmup:]
      t_app[n] = [timed(lambda: ops.kv_append_rope_rows(qkv, lens, rope[0], rope[1], cache.kv[0], nh, status=cache.status))
                  for _ in range(n_runs)][a.warmup:]
    ext_s1 = [timed(lambda: ops.attn_extend(q1, cache.kv[0], lens, nh, splits=1)) for _ in range(n_runs)][a.warmup:]
    cache.check()
  m_e8, m_d8, m_d1, m_e128, m_p = (statistics.median(v) for v in (t_e8, t_d8, t_d1, t_e128, t_p))
  launches = 2 + 10 * cfg.n_layers + 1 + 2 + 1  # as a decode step (tools/gen_bench.py) plus the gather of the last rows
  lines = [
    '# tools/extend_bench.py: 160M (12 layers, d 768, 12 heads, V 50280), B = %d, %d cached tokens, cache of %d rows; one process, sides alternating; ms, median of %d [min max]'
    % (B, CTX, SEQ, a.runs),
    'extend, n = 8 (E8)                                   %s' % med(t_e8),
    '8 decode steps (D8)                                  %s' % med(t_d8),
    'D8 / E8                                              %.2f' % (m_d8 / m_e8),
    'one decode step (D1)                                 %s' % med(t_d1),
    'E8 / D1                                              %.2f' % (m_e8 / m_d1),
    'host time to enqueue E8 (about %d launches)         %s' % (launches, med(t_h)),
    'E8 and D8 choose the same next token                 %.3f of %d sequences (max |dlogp| %.2e; random weights: near-uniform logits)' % (same8, B, dlp8),
    'extend, n = 128 (E128)                               %s' % med(t_e128),
    'prefill of all %d tokens (P)                       %s' % (SEQ, med(t_p)),
    'P / E128                                             %.2f' % (m_p / m_e128),
    'E128 and P choose the same next token                %.3f of %d sequences (max |dlogp| %.2e)' % (same128, B, dlp128),
    'plm_attn_decode alone, 1025 keys, automatic splits   %s' % med(t_dec),
  ]
  for n in (1, 8, 128):
    lines.append('plm_attn_extend alone, n = %-3d automatic splits      %s' % (n, med(t_ext[n])))
  lines.append('plm_attn_extend alone, n = 1, splits = 1 (one launch) %s' % med(ext_s1))
  for n in (1, 8, 128):
    lines.append('plm_kv_append_rope_rows alone, n = %-3d               %s' % (n, med(t_app[n])))
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
