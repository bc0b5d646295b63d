"""Where the two launches of plm_spec_verify_bf16 read and write, on a real MI355X.  Same machinery as tests/test_footprint_gpu.py
(tests/footprint.py: every buffer between margins, two runs that differ in one fill byte; W / I / C+R / U are bit equality); that file's
completeness test counts these rows.  Both logits operands are column windows of wider buffers, as in tests/test_footprint_sample_gpu.py:
the base is 3 columns into a row and the row stride is odd, so every row starts at another 2-byte alignment; the columns before the
window, the columns >= V and the pad hold the fill bytes - NaN in one run - and a result that took one in differs between the runs.
logp is scratch between the launches and an output after them: every one of its B * (k + 1) entries must end up written."""
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


def _window(ar, name, x, V):
  rows, cols = x.shape
  ld = cols + PAD + (1 - (cols + PAD) % 2)  # odd
  window = torch.zeros(rows, cols, dtype=torch.bool)
  window[:, SKIP:SKIP + V] = True
  # in-place role with nothing written: the columns outside the window get the run's fill bytes and must not reach a result
  return ar.inout(name, x, ld=ld, misalign=True, written=torch.zeros(rows, cols, dtype=torch.bool), unread=~window), ld


def _cases():
  # a ragged V with a head, a vector body and a tail; a row of fewer columns than one vector; k = 1 and k = 8; a filtered and an unfiltered cutoff
  for B, V, k, tau, cut in ((3, 1000, 8, 0.8, 0.5), (3, 1000, 1, 0.8, 0.5), (5, 5, 4, 1.0, -1e30), (2, 257, 8, 0.05, -1e30), (2, 50283, 2, 0.8, 1.0)):
    def fn(ar, B=B, V=V, k=k, tau=tau, cut=cut):
      cols = SKIP + V + TAIL
      g = torch.Generator().manual_seed(V + B + k)
      xp = (torch.randn(B * (k + 1), cols, generator=g) * 2).to(BF16)
      xq = (xp.view(B, k + 1, cols)[:, :k].transpose(0, 1).reshape(k * B, cols).float() + torch.randn(k * B, cols, generator=g)).to(BF16)
      xp[0, SKIP + V // 2] = float('nan')          # a non-finite logit inside the window is an ordinary input
      xq[0, SKIP] = float('-inf')
      p_logits, ldp = _window(ar, 'p_logits', xp, V)
      q_logits, ldq = _window(ar, 'q_logits', xq, V)
      # the drafted token: the draft row's argmax inside the window (accepted or not by u), one of them outside [0, V)
      tok = xq[:, SKIP:SKIP + V].float().nan_to_num(-1e30).argmax(dim=1)
      tok[-1] = V + 7
      draft_tok = ar.inp('draft_tok', tok.to(I64), index_margin=(0, V - 1))
      p_cutoff = ar.inp('p_cutoff', torch.full((B * (k + 1),), cut))
      q_cutoff = ar.inp('q_cutoff', torch.full((k * B,), cut))
      p_tok = ar.inp('p_tok', torch.randint(V, (B * (k + 1),), generator=g), index_margin=(0, V - 1))
      u_accept = ar.inp('u_accept', torch.rand(k * B, generator=g))
      u_resid = ar.inp('u_resid', torch.rand(B, generator=g))
      n_accept = ar.out('n_accept', I32, B)
      next_tok = ar.out('next_tok', I64, B)
      logp = ar.out('logp', F32, B * (k + 1))
      return lambda: call('plm_spec_verify_bf16', P(p_logits, 2 * SKIP), ldp, P(q_logits, 2 * SKIP), ldq, P(draft_tok), P(p_cutoff),
                          P(q_cutoff), P(p_tok), P(u_accept), P(u_resid), tau, P(n_accept), P(next_tok), P(logp), B, k, V)
    CASES[f'spec_verify-B{B}-V{V}-k{k}'] = (('plm_spec_verify_bf16',), fn)


_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  arenas = FP.run_on_gpu(cid, *CASES[cid])
  for ar in arenas:
    buf = {b.name: b for b in ar.bufs}
    V = buf['p_logits'].cols - SKIP - TAIL
    B = buf['n_accept'].t.numel()
    k = buf['logp'].t.numel() // B - 1
    assert ((buf['next_tok'].t >= 0) & (buf['next_tok'].t < V)).all()
    assert ((buf['n_accept'].t >= 0) & (buf['n_accept'].t <= k)).all()
  # the in-place role does not compare the payload with its pre-launch state: the windows must still hold what was put there
  for name in ('p_logits', 'q_logits'):
    a, b = (next(x for x in ar.bufs if x.name == name) for ar in arenas)
    assert torch.equal(a.body[:, SKIP:SKIP + V], b.body[:, SKIP:SKIP + V])
