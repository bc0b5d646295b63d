"""Cost of one beam-search token at the 160M shape, P = 1 prompt, G beams, after 64 generated tokens:
  S  the sampling step of generate_samples on a SharedPrefixCache: decode_step(logits=True) + ops.sample_logits    (the yardstick: the same
     rows through the same model, no re-parenting)
  B  the beam step on a fork_beam cache: decode_step(logits=True) + ops.beam_select + ops.beam_advance, identity ancestry (every beam on
     its own slot: no (slot, tile) pair is dead, the suffix kernel's worst case)
unfused and fused, the four sides alternating in one process (tools/gen_bench.py's ``alternate``): device ms by HIP events, median of --runs
[min max], host enqueue, library calls.  Then alone, same statistics: the attention of one layer (ops.attn_decode_shared; ops.attn_decode_beam
with identity and with collapsed ancestry - every beam on slot 0's rows), ops.beam_select, ops.beam_advance; and the suffix-cache bytes
against the two copies a ping-pong gather needs.
Usage: python tools/beam_bench.py [--beams 4 8 32] [--context 1024 4096] [--runs 20] --out profiles/beam_bench.txt"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_bench import ModelConfig, Transformer, alternate, med, ops, timed  # noqa: E402


def alone(fn, a):
  v = []
  for i in range(a.warmup + a.runs):
    torch.cuda.synchronize()
    e = timed(fn)
    if i >= a.warmup:
      v.append(e)
  return med(v)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--runs', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--beams', type=int, nargs='+', default=[4, 8, 32])
  ap.add_argument('--context', type=int, nargs='+', default=[1024, 4096])
  ap.add_argument('--out', default=None)
  a = ap.parse_args()
  torch.manual_seed(0)
  done, room = 64, 68
  cfg = ModelConfig(vocab_size=50280, seq_len=max(a.context) + room, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu')
  m = Transformer(cfg).cuda()
  nh = cfg.n_heads
  lines = ['# tools/beam_bench.py: 160M (12 layers, d 768, 12 heads, V 50280), P = 1 prompt, G beams, after %d generated tokens; S = sampling step on a '
           'SharedPrefixCache, B = beam step (identity ancestry); one process, the four sides alternating; ms, HIP events, median of %d [min max]'
           % (done, a.runs)]
  with torch.no_grad():
    for ctx in a.context:
      prompt = torch.randint(0, cfg.vocab_size, (1, ctx), device='cuda')
      pcache, _ = m.prefill(prompt, max_len=ctx)
      for Gs in a.beams:
        shared, beamc = m.fork(pcache, Gs, room), m.fork_beam(pcache, Gs, room)
        buf = beamc.beam
        for i in range(cfg.n_layers):
          shared.kv[i].copy_(torch.randn(shared.kv[i].shape, device='cuda') * 0.5)
          beamc.kv[i].copy_(shared.kv[i])
        ident = torch.arange(Gs, dtype=torch.uint8, device='cuda')[:, None].expand(Gs, room).contiguous()
        buf._anc[:] = ident
        buf.score.copy_(-torch.rand(Gs, device='cuda'))
        l_s = torch.full((Gs,), done, dtype=torch.int32, device='cuda')
        nxt, u = torch.randint(0, cfg.vocab_size, (Gs,), device='cuda'), torch.rand(Gs, device='cuda')
        sides = {}
        for f in (False, True):
          sides[('S', f)] = lambda f=f: ops.sample_logits(m.decode_step(nxt, shared, logits=True, fused=f), u, 1.0, 0, 1.0)
          sides[('B', f)] = lambda f=f: ops.beam_advance(buf, ops.beam_select(m.decode_step(nxt, beamc, logits=True, fused=f), buf.score, Gs, Gs))

        def reset():
          for c in (shared, beamc):
            c._pl[1].copy_(l_s)
            c._pl[0].copy_(l_s - 1)
          buf.steps = done
        dev, host, calls, _ = alternate(sides, reset, a)
        suffix = sum(t.numel() * 2 for t in beamc.kv)
        lines.append('G = %d, prompt %d: suffix-cache bytes %d (a ping-pong gather holds %d), ancestor tables %d B' % (Gs, ctx, suffix, 2 * suffix,
                                                                                                                   buf._anc.numel()))
        for f, what in ((False, 'unfused'), (True, 'fused  ')):
          for k, name in (('S', 'sampling step (S)'), ('B', 'beam step (B)    ')):
            lines.append('  %s %s  device %s   host enqueue %s   library calls %3d' % (what, name, med(dev[(k, f)]), med(host[(k, f)]), len(calls[(k, f)])))
          s, b = dev[('S', f)], dev[('B', f)]
          where = 'overlaps' if min(b) <= max(s) and min(s) <= max(b) else ('lies above' if min(b) > max(s) else 'lies below')
          lines.append('    B / S (medians) %.2f; B\'s [min max] %s S\'s' % (statistics.median(b) / statistics.median(s), where))
        # alone: one layer's attention, the selection, the bookkeeping
        reset()
        q = torch.randn(Gs, cfg.dim, device='cuda').to(torch.bfloat16)
        lens = l_s + 1
        coll = torch.zeros_like(ident)
        kp, lp, ks = pcache.kv[0], pcache.lens, beamc.kv[0]
        logits = torch.randn(Gs, cfg.vocab_size, device='cuda').to(torch.bfloat16)
        cand = ops.beam_select(logits, buf.score, Gs, Gs)

        def advance():
          buf.steps = done
          ops.beam_advance(buf, cand)
        lines.append('  alone: attn_decode_shared %s   attn_decode_beam identity %s   collapsed %s' % (
            alone(lambda: ops.attn_decode_shared(q, kp, lp, ks, lens, nh), a), alone(lambda: ops.attn_decode_beam(q, kp, lp, ks, lens, ident, nh), a),
            alone(lambda: ops.attn_decode_beam(q, kp, lp, ks, lens, coll, nh), a)))
        lines.append('  alone: sample_logits %s   beam_select %s   beam_advance %s' % (
            alone(lambda: ops.sample_logits(logits, u, 1.0, 0, 1.0), a), alone(lambda: ops.beam_select(logits, buf.score, Gs, Gs), a), alone(advance, a)))
        del shared, beamc, sides
      del pcache
  text = '\n'.join(lines) + '\n'
  print(text, end='')
  if a.out:
    with open(a.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
