"""Where the launches of the cascade read and write, on a real MI355X: the footprint cases of its entry points, on
tests/test_footprint_ragged_gpu.py's served step.  Sequence 0 shares its first page and sequence 2 its first four, each the only
member of its group; the plan's words are inputs with index margins, the padding row's q is NaN and never loaded, every out / lse
row is written, and the claim words of the workspace never reach a result.  test_footprint_gpu.py's completeness test counts these rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402
from test_footprint_paged_gpu import BF16, D, F32, HD, I32, LD, MAXP, NH, NP, PG, _pool_in, _rows, _table, rnd  # noqa: E402
from test_footprint_ragged_gpu import B, EPS, HIDDEN, SERVED, _rope_in, _words  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {}
KEY_LO, NTG, PCAP = (PG, 0, 4 * PG, 0), 2, 4 * PG
TILE_ROWS = [list(range(5)) + [-1] * 27, list(range(6, 11)) + [-1] * 27]  # SERVED packs 5, 1 and 5 rows, then the padding row


def _plan(ar):
  i32 = lambda name, v, hi: ar.inp(name, torch.tensor(v, dtype=I32).reshape(-1), index_margin=(0, hi))  # noqa: E731
  return i32('key_lo', KEY_LO, PG), i32('tile_rows', TILE_ROWS, 1), i32('tile_seq', [0, 2], 1), i32('tile_keys', [PG, 4 * PG], PG)


def _attend(ar):
  l0, cu, rs, R, NT = _words(ar, *SERVED)
  kl, tr, ts, tk = _plan(ar)
  Lcap = MAXP * PG
  nbytes = int(L().plm_attn_ragged_paged_cascade_workspace_bytes(R, NH, HD, Lcap, NTG, PCAP))
  assert nbytes > 0
  qd = rnd(33, R, D, dtype=BF16)
  qd[-1] = float('nan')  # the padding row is never loaded
  q = ar.inp('q', qd, misalign=True)
  pool, tb = _pool_in(ar, 34, [a + c for a, c in zip(*SERVED)]), _table(ar)
  out, lse, ws = ar.out('out', BF16, R, D), ar.out('lse', F32, R * NH), ar.ws('workspace', nbytes)
  return lambda: call('plm_attn_ragged_paged_cascade', P(q), P(pool), LD, P(tb), P(l0), P(kl), P(cu), P(rs), P(tr), P(ts), P(tk), P(out), P(lse), R, B,
                      NT, NTG, Lcap, PCAP, MAXP, NP, NH, HD, P(ws), nbytes)


def _layer(ar):
  lens0, counts = SERVED
  l0, cu, rs, R, NT = _words(ar, lens0, counts)
  kl, tr, ts, tk = _plan(ar)
  w = lambda seed, *shape: ar.inp(f'w{seed}', (0.1 * rnd(seed, *shape)).to(BF16))  # noqa: E731
  x = ar.inout('x', rnd(41, R, D), misalign=True)
  an, mn = ar.inp('attn_norm_w', 1 + 0.1 * rnd(42, D)), ar.inp('mlp_norm_w', 1 + 0.1 * rnd(43, D))
  wq, wo, w1, w2 = w(44, 3 * D, D), w(45, D, D), w(46, 2 * HIDDEN, D), w(47, D, HIDDEN)
  rc, rsn = _rope_in(ar)
  wr = _rows([(a, a + c) for a, c in zip(lens0, counts)])
  stale = ~_rows([(0, a + c) for a, c in zip(lens0, counts)])  # the layer attends the rows below the new lengths
  pool = ar.inout('pool', rnd(48, NP * PG, 2 * D, dtype=BF16), ld=LD, written=wr, untouched=stale, unread=stale | wr)
  tb, status = _table(ar), ar.inout('status', torch.zeros(1, dtype=I32))
  Lcap = MAXP * PG
  nbytes = int(L().plm_ragged_layer_paged_wide_cascade_workspace_bytes(R, NH, HD, HIDDEN, Lcap, NTG, PCAP))
  assert nbytes > 0
  wsp = ar.ws('workspace', nbytes)
  return lambda: call('plm_ragged_layer_paged_wide_cascade_bf16', P(x), P(an), P(mn), EPS, P(wq), P(wo), P(w1), P(w2), P(l0), P(kl), P(cu), P(rs),
                      P(tr), P(ts), P(tk), P(rc), P(rsn), MAXP * PG, P(pool), LD, P(tb), P(status), R, B, NT, NTG, Lcap, PCAP, MAXP, NP, NH, HD,
                      HIDDEN, 0, P(wsp), nbytes)


CASES['attn_ragged_paged_cascade'] = (('plm_attn_ragged_paged_cascade', 'plm_attn_ragged_paged_cascade_workspace_bytes'), _attend)
CASES['ragged_layer_paged_wide_cascade'] = (('plm_ragged_layer_paged_wide_cascade_bf16', 'plm_ragged_layer_paged_wide_cascade_workspace_bytes'),
                                            _layer)


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
