"""Where the launch of plm_sample_logits_bf16 reads and writes, on a real MI355X.  Same machinery as tests/test_footprint_gpu.py
(tests/footprint.py: every buffer between margins, two runs that differ in one fill byte; W / I / C+R / U are bit equality); that file's
completeness test counts these rows.  The logits are a column window of a wider buffer: the base is 3 columns (6 bytes) into a row, the
row stride is odd, so every row starts at another 2-byte alignment; the columns before the window, the columns >= V and the pad hold the
fill bytes - NaN in one run - and a result that took one in differs between the runs."""
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
SKIP, TAIL, PAD = 3, 2, 8   # columns of the buffer before the window, after it, and the pad beyond the payload


def _cases():
  # (B, V): rows kept in LDS, with a head, a vector body and a tail; a row of fewer columns than one vector; a row wider than the LDS copy
  for B, V, stats, tau, k, p in ((5, 1000, 1, 0.8, 50, 0.95), (5, 1000, 0, 0.8, 50, 0.95), (33, 5, 1, 1.0, 0, 0.9), (7, 257, 1, 0.05, 1, 1.0),
                                 (2, 65544, 1, 0.8, 50, 0.95), (2, 65544, 0, 50.0, 0, 1.0)):
    def fn(ar, B=B, V=V, stats=stats, tau=tau, k=k, p=p):
      cols = SKIP + V + TAIL
      ld = cols + PAD + (1 - (cols + PAD) % 2)  # odd
      g = torch.Generator().manual_seed(V + B)
      x = (torch.randn(B, cols, generator=g) * 2).to(BF16)
      x[0, SKIP + V // 2] = float('nan')          # a non-finite logit inside the window is an ordinary input
      window = torch.zeros(B, cols, dtype=torch.bool)
      window[:, SKIP:SKIP + V] = True
      nothing = torch.zeros(B, cols, dtype=torch.bool)
      # in-place role with nothing written: the columns outside the window get the run's fill bytes and must not reach a result
      logits = ar.inout('logits', x, ld=ld, misalign=True, written=nothing, unread=~window)
      u = ar.inp('u', torch.rand(B, generator=g))
      tok = ar.out('tok', I64, B)
      logp = ar.out('logp', F32, B)
      n_kept = ar.out('n_kept', I32, B) if stats else None
      cutoff = ar.out('cutoff', F32, B) if stats else None
      return lambda: call('plm_sample_logits_bf16', P(logits, 2 * SKIP), ld, P(u), tau, k, p, P(tok), P(logp), P(n_kept), P(cutoff), B, V)
    CASES[f'sample_logits-B{B}-V{V}-{"stats" if stats else "nostats"}'] = (('plm_sample_logits_bf16',), fn)


_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  arenas = FP.run_on_gpu(cid, *CASES[cid])
  # the in-place role does not compare the payload with its pre-launch state: the window must still hold what was put there
  for ar in arenas:
    logits = next(b for b in ar.bufs if b.name == 'logits')
    tok = next(b for b in ar.bufs if b.name == 'tok')
    V = logits.cols - SKIP - TAIL
    assert ((tok.t >= 0) & (tok.t < V)).all()
  a, b = (next(x for x in ar.bufs if x.name == 'logits') for ar in arenas)
  assert torch.equal(a.body[:, SKIP:SKIP + V], b.body[:, SKIP:SKIP + V])
