"""Where the launches of the wide fused layer read and write, on a real MI355X: one footprint case per entry
point of csrc/layer_wide.hip, on tests/test_footprint_paged_gpu.py's pool and table.  Every case has M = 65 rows, so that a row tile of
one row sits between the guard margins; the ragged cases pack 64 rows of four sequences and one padding row (row_seq = -1)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402
from test_footprint_paged_gpu import BF16, D, MAXP, NH, HD, I32, LD, NP, PG, _rows, _table, rnd  # noqa: E402
from test_footprint_ragged_gpu import B, EPS, HIDDEN, _rope_in, _words  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {}
M = 65
REFUSING = ((125, 0, 5 * PG - 2, 0), (20, 3, 39, 2))  # (lens0, counts): sequences 2 (past max_pages) and 3 (no page) are refused
SERVED = ((125, 0, 250, 0), (20, 3, 41, 0))           # across a page edge, a first chunk, over two pages, idle
w = lambda ar, seed, *shape: ar.inp(f'w{seed}', (0.1 * rnd(seed, *shape)).to(BF16))  # noqa: E731


def _residual(ar):
  x = ar.inout('x', rnd(51, M, D), misalign=True)
  a = ar.inp('A', rnd(52, M, HIDDEN, dtype=BF16))
  return lambda: call('plm_wide_gemm_residual_bf16', P(x), P(a), P(w(ar, 53, D, HIDDEN)), M, D, HIDDEN)


def _fc1(ar):
  x = ar.inp('x', rnd(54, M, D), misalign=True)
  nw, act = ar.inp('norm_w', 1 + 0.1 * rnd(55, D)), ar.out('act', BF16, M, HIDDEN)
  return lambda: call('plm_wide_norm_fc1_act_bf16', P(x), P(nw), EPS, P(w(ar, 56, 2 * HIDDEN, D)), P(act), M, D, HIDDEN, 0)


def _ragged(ar, layer):
  lens0, counts = SERVED if layer else REFUSING
  l0, cu, rs, R, NT = _words(ar, lens0, counts)
  assert R == M
  x = (ar.inout if layer else ar.inp)('x', rnd(61, R, D), misalign=True)
  an, wq = ar.inp('attn_norm_w', 1 + 0.1 * rnd(62, D)), w(ar, 64, 3 * D, D)
  rc, rsn = _rope_in(ar)
  wr = _rows([(a, a + c) for a, c in zip(lens0, counts)] if layer else [(125, 145), (0, 3), (0, 0), (0, 0)])
  stale = ~_rows([(0, a + c) for a, c in zip(lens0, counts)]) if layer else ~wr  # a layer attends the rows below the new lengths
  pool = ar.inout('pool', rnd(68, NP * PG, 2 * D, dtype=BF16), ld=LD, written=wr, untouched=stale, unread=stale | wr)
  tb, status = _table(ar), ar.inout('status', torch.zeros(1, dtype=I32))
  if not layer:
    q_out = ar.out('q_out', BF16, R, D)
    return lambda: call('plm_ragged_norm_qkv_append_paged_wide_bf16', P(x), P(an), EPS, P(wq), P(l0), P(cu), P(rs), P(rc), P(rsn), MAXP * PG, P(q_out),
                        P(pool), LD, P(tb), P(status), R, B, MAXP, NP, NH, HD)
  mn, wo, w1, w2 = ar.inp('mlp_norm_w', 1 + 0.1 * rnd(63, D)), w(ar, 65, D, D), w(ar, 66, 2 * HIDDEN, D), w(ar, 67, D, HIDDEN)
  Lcap = MAXP * PG
  nbytes = int(L().plm_ragged_layer_paged_wide_workspace_bytes(R, NH, HD, HIDDEN, Lcap))
  assert nbytes > 0
  wsp = ar.ws('workspace', nbytes)
  return lambda: call('plm_ragged_layer_paged_wide_bf16', P(x), P(an), P(mn), EPS, P(wq), P(wo), P(w1), P(w2), P(l0), P(cu), P(rs), P(rc), P(rsn),
                      MAXP * PG, P(pool), LD, P(tb), P(status), R, B, NT, Lcap, MAXP, NP, NH, HD, HIDDEN, 0, P(wsp), nbytes)


CASES['wide_gemm_residual'] = (('plm_wide_gemm_residual_bf16',), _residual)
CASES['wide_norm_fc1_act'] = (('plm_wide_norm_fc1_act_bf16',), _fc1)
CASES['ragged_norm_qkv_append_paged_wide'] = (('plm_ragged_norm_qkv_append_paged_wide_bf16',), lambda ar: _ragged(ar, False))
CASES['ragged_layer_paged_wide'] = (('plm_ragged_layer_paged_wide_bf16', 'plm_ragged_layer_paged_wide_workspace_bytes'), lambda ar: _ragged(ar, True))


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
