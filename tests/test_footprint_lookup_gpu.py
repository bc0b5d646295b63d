"""Where the launches of draft-free speculative decoding read and write, on a real MI355X: the footprint cases of plm_lookup_draft_i64
and plm_spec_verify_lookup_bf16.  Same machinery as tests/test_footprint_gpu.py (tests/footprint.py: every
buffer between margins, two runs that differ in one fill byte; W / I / C+R / U are bit equality); that file's completeness test counts
these rows.  hist and lens are in/out operands, treated as tests/test_footprint_extend_gpu.py treats the cache and the status word:
the appended extent is written, what lies beyond a sequence's new length is untouched, and everything at and beyond its old length
holds the run's fill bytes when the launch starts (it is written before it is read, or never read).  The history itself and a refused
sequence's length are read, so they hold data under both fills; the test compares them after the runs.  The logits operand is a column window of a
wider buffer, as in tests/test_footprint_spec_gpu.py, and its rows beyond n_prop[b] hold the fill bytes too."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import P, call  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
CASES = {}      # id -> (entry points covered, case function)
EXPECT = {}     # draft case tag -> (lens, appended counts, refused sequences)
SKIP, TAIL, PAD = 3, 2, 8   # columns of the logits buffer before the window, after it, and the pad beyond the payload


def _draft_cases():
  # (tag, ld, lens, n_add or None, ld_add or 0 for no add_tok, k, ngram): appends of every size, a sequence that does not fit, no append at all
  rows = (('append', 300, (0, 1, 255, 290, 37), (1, 5, 0, 5, 3), 5, 4, (1, 4)),
          ('append-all', 300, (0, 1, 255, 290, 37), None, 2, 31, (1, 16)),
          ('one-outside', 300, (10, 297, 255, 300, 37), (5, 5, 2, 0, 1), 5, 8, (2, 4)),
          ('no-add', 64, (0, 1, 2, 64, 33), None, 0, 1, (1, 1)))
  for tag, ld, lens, n_add, ld_add, k, ngram in rows:
    def fn(ar, tag=tag, ld=ld, lens=lens, n_add=n_add, ld_add=ld_add, k=k, ngram=ngram):
      B = len(lens)
      g = torch.Generator().manual_seed(ld + k)
      counts = [0] * B if not ld_add else ([ld_add] * B if n_add is None else [min(max(c, 0), ld_add) for c in n_add])
      refused = [b for b in range(B) if lens[b] + counts[b] > ld]
      written = torch.zeros(B, ld, dtype=torch.bool)
      beyond = torch.zeros(B, ld, dtype=torch.bool)
      unread = torch.zeros(B, ld, dtype=torch.bool)
      for b in range(B):
        unread[b, lens[b]:] = True
        grown = 0 if b in refused else counts[b]
        written[b, lens[b]:lens[b] + grown] = True
        beyond[b, lens[b] + grown:] = True
      # [0, lens[b]) is read and never written: it is claimed as payload, and the test below compares it between the runs
      hist = ar.inout('hist', torch.randint(3, (B, ld), generator=g), written=written, untouched=beyond, unread=unread, misalign=True)
      # lens: rewritten (with the same bits under both fills) for every sequence that is not refused; a refused one is read, so it cannot
      # hold a fill: the test below looks at it
      ln = ar.inout('lens', torch.tensor(lens, dtype=I32), written=torch.tensor([b not in refused for b in range(B)]))
      EXPECT[tag] = (lens, counts, refused)
      add = ar.inp('add_tok', torch.randint(3, (B, ld_add), generator=g)) if ld_add else None
      na = ar.inp('n_add', torch.tensor(n_add, dtype=I32), index_margin=(0, 1)) if n_add is not None else None
      draft = ar.out('draft_tok', I64, B, k)
      n_prop = ar.out('n_prop', I32, B)
      match_len = ar.out('match_len', I32, B)
      st = torch.tensor([bool(refused)])
      status = ar.inout('status', torch.zeros(1, dtype=I32), written=st, untouched=~st)
      return lambda: call('plm_lookup_draft_i64', P(hist), ld, P(ln), P(add), ld_add, P(na), P(draft), P(n_prop), P(match_len), P(status), B, k,
                          ngram[0], ngram[1])
    CASES[f'lookup_draft-{tag}'] = (('plm_lookup_draft_i64',), fn)


def _verify_cases():
  # a ragged V with a head, a vector body and a tail; a row of fewer columns than one vector; k = 1 and k = 8; ragged n_prop with 0 and k
  for B, V, k, tau, cut, n_prop in ((3, 1000, 8, 0.8, 0.5, (8, 0, 3)), (3, 1000, 1, 0.8, 0.5, (1, 0, 1)), (5, 5, 4, 1.0, -1e30, (4, 2, 0, 1, 3)),
                                    (2, 257, 8, 0.05, -1e30, (8, 5)), (2, 50283, 2, 0.8, 1.0, (1, 2))):
    def fn(ar, B=B, V=V, k=k, tau=tau, cut=cut, n_prop=n_prop):
      cols = SKIP + V + TAIL
      g = torch.Generator().manual_seed(V + B + k)
      xp = (torch.randn(B * (k + 1), cols, generator=g) * 2).to(BF16)
      xp[0, SKIP + V // 2] = float('nan')          # a non-finite logit inside the window is an ordinary input
      ld = cols + PAD + (1 - (cols + PAD) % 2)     # odd: every row starts at another 2-byte alignment
      unread = torch.ones(B * (k + 1), cols, dtype=torch.bool)
      live_rows = torch.zeros(B * (k + 1), dtype=torch.bool)
      for b in range(B):
        live_rows[b * (k + 1):b * (k + 1) + n_prop[b] + 1] = True   # chunk rows 0 .. n_prop[b]: the proposal's rows and the bonus row
      unread[live_rows, SKIP:SKIP + V] = False
      # in-place role with nothing written: what lies outside the window, and every row beyond n_prop[b], gets the run's fill bytes
      p_logits = ar.inout('p_logits', xp, ld=ld, misalign=True, written=torch.zeros(B * (k + 1), cols, dtype=torch.bool), unread=unread)
      # the proposal: the row's argmax inside the window (accepted or not by u), one of them outside [0, V)
      tok = xp[:, SKIP:SKIP + V].float().nan_to_num(-1e30).argmax(dim=1).view(B, k + 1)[:, :k].contiguous()
      tok[-1, 0] = V + 7
      draft_tok = ar.inp('draft_tok', tok.to(I64), index_margin=(0, V - 1))
      npr = ar.inp('n_prop', torch.tensor(n_prop, dtype=I32), index_margin=(0, 1))
      p_cutoff = ar.inp('p_cutoff', torch.full((B * (k + 1),), cut))
      p_tok = ar.inp('p_tok', torch.randint(V, (B * (k + 1),), generator=g), index_margin=(0, V - 1))
      u_accept = ar.inp('u_accept', torch.rand(k * B, generator=g))
      u_resid = ar.inp('u_resid', torch.rand(B, generator=g))
      n_accept = ar.out('n_accept', I32, B)
      next_tok = ar.out('next_tok', I64, B)
      logp = ar.out('logp', F32, B * (k + 1))
      return lambda: call('plm_spec_verify_lookup_bf16', P(p_logits, 2 * SKIP), ld, P(draft_tok), P(npr), P(p_cutoff), P(p_tok), P(u_accept),
                          P(u_resid), tau, P(n_accept), P(next_tok), P(logp), B, k, V)
    CASES[f'spec_verify_lookup-B{B}-V{V}-k{k}'] = (('plm_spec_verify_lookup_bf16',), fn)


_draft_cases()
_verify_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  arenas = FP.run_on_gpu(cid, *CASES[cid])
  if cid.startswith('lookup_draft-'):
    lens, counts, refused = EXPECT[cid[len('lookup_draft-'):]]
    h0, h1 = (next(x for x in ar.bufs if x.name == 'hist') for ar in arenas)
    for b, n in enumerate(lens):
      assert torch.equal(h0.body[b, :n], h1.body[b, :n]) and int(h0.body[b, :n].min() if n else 0) >= 0 and int(h0.body[b, :n].max() if n else 0) < 3
    for ar in arenas:
      buf = {x.name: x for x in ar.bufs}
      assert buf['lens'].t.tolist() == [n + (0 if b in refused else counts[b]) for b, n in enumerate(lens)]
      assert all(buf['n_prop'].t[b].item() == 0 for b in refused)
    return
  for ar in arenas:
    buf = {b.name: b for b in ar.bufs}
    V = buf['p_logits'].cols - SKIP - TAIL
    B = buf['n_accept'].t.numel()
    k = buf['logp'].t.numel() // B - 1
    assert ((buf['next_tok'].t >= 0) & (buf['next_tok'].t < V)).all()
    assert ((buf['n_accept'].t >= 0) & (buf['n_accept'].t <= buf['n_prop'].t) & (buf['n_accept'].t <= k)).all()
