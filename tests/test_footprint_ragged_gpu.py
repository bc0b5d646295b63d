"""Where the launches of a ragged step read and write, on a real MI355X: the footprint cases of its entry points,
on tests/test_footprint_paged_gpu.py's pool and table.  Every case packs four sequences and one padding row (row_seq = -1), whose q_out /
out / lse are written and whose inputs are never read.  test_footprint_gpu.py's completeness test counts these rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402
from test_footprint_paged_gpu import BF16, D, F32, HD, I32, LD, MAXP, NH, NP, PG, _pool_in, _rope, _rows, _table, rnd  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {}
B, HIDDEN, EPS = 4, 256, 1e-6
REFUSING = ((125, 0, 5 * PG - 2, 0), (5, 1, 3, 2))  # (lens0, counts): sequences 2 (past max_pages) and 3 (no page) are refused
SERVED = ((125, 0, 5 * PG - 5, 0), (5, 1, 5, 0))    # across a page edge, a first token, up to the table's end, idle


def _words(ar, lens0, counts):
  """lens0, cu_rows, row_seq (one padding row at the end) as inputs; returns them with R and NT."""
  cu = [sum(counts[:b]) for b in range(B + 1)]
  seq = [b for b, c in enumerate(counts) for _ in range(c)] + [-1]
  i32 = lambda name, v: ar.inp(name, torch.tensor(v, dtype=I32), index_margin=(0, 1))  # noqa: E731
  return i32('lens0', lens0), i32('cu_rows', cu), i32('row_seq', seq), len(seq), sum(-(-c // 32) for c in counts)


def _rope_in(ar):
  cos, sin = _rope(MAXP * PG)
  return ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)


def _append(ar):
  l0, cu, rs, R, _ = _words(ar, *REFUSING)
  ld_qkv = 3 * D + 8
  qkv = ar.inp('qkv', rnd(31, R, 3 * D, dtype=BF16), ld=ld_qkv, misalign=True)
  rc, rsn = _rope_in(ar)
  q_out = ar.out('q_out', BF16, R, D)  # every row is written: rotated q, or zeros
  rows = _rows([(125, 130), (0, 1), (0, 0), (0, 0)])
  pool = ar.inout('pool', rnd(32, NP * PG, 2 * D, dtype=BF16), ld=LD, written=rows, untouched=~rows, unread=torch.ones(NP * PG, 2 * D, dtype=torch.bool))
  tb, status = _table(ar), ar.inout('status', torch.zeros(1, dtype=I32))
  return lambda: call('plm_kv_paged_append_rope_packed', P(qkv), ld_qkv, P(l0), P(cu), P(rs), P(rc), P(rsn), MAXP * PG, P(q_out), P(pool), LD, P(tb),
                      P(status), R, B, MAXP, NP, NH, HD)


def _attend(ar):
  l0, cu, rs, R, NT = _words(ar, *SERVED)
  Lcap = MAXP * PG
  nbytes = int(L().plm_attn_ragged_paged_workspace_bytes(R, NH, HD, Lcap))
  assert nbytes > 0
  qd = rnd(33, R, D, dtype=BF16)
  qd[-1] = float('nan')  # the padding row is never loaded
  q = ar.inp('q', qd, misalign=True)
  pool, tb = _pool_in(ar, 34, [a + c for a, c in zip(*SERVED)]), _table(ar)
  out, lse, ws = ar.out('out', BF16, R, D), ar.out('lse', F32, R * NH), ar.ws('workspace', nbytes)
  return lambda: call('plm_attn_ragged_paged', P(q), P(pool), LD, P(tb), P(l0), P(cu), P(rs), P(out), P(lse), R, B, NT, Lcap, MAXP, NP, NH, HD, P(ws),
                      nbytes)


def _fused(ar, layer):
  lens0, counts = SERVED if layer else REFUSING
  l0, cu, rs, R, NT = _words(ar, lens0, counts)
  w = lambda seed, *shape: ar.inp(f'w{seed}', (0.1 * rnd(seed, *shape)).to(BF16))  # noqa: E731
  x = (ar.inout if layer else ar.inp)('x', rnd(41, R, D), misalign=True)
  an, wq = ar.inp('attn_norm_w', 1 + 0.1 * rnd(42, D)), w(44, 3 * D, D)
  rc, rsn = _rope_in(ar)
  wr = _rows([(a, a + c) for a, c in zip(lens0, counts)] if layer else [(125, 130), (0, 1), (0, 0), (0, 0)])
  stale = ~_rows([(0, a + c) for a, c in zip(lens0, counts)]) if layer else ~wr  # a layer attends the rows below the new lengths
  pool = ar.inout('pool', rnd(48, NP * PG, 2 * D, dtype=BF16), ld=LD, written=wr, untouched=stale, unread=stale | wr)
  tb, status = _table(ar), ar.inout('status', torch.zeros(1, dtype=I32))
  if not layer:
    q_out = ar.out('q_out', BF16, R, D)
    return lambda: call('plm_ragged_norm_qkv_append_paged_bf16', P(x), P(an), EPS, P(wq), P(l0), P(cu), P(rs), P(rc), P(rsn), MAXP * PG, P(q_out),
                        P(pool), LD, P(tb), P(status), R, B, MAXP, NP, NH, HD)
  mn, wo, w1, w2 = ar.inp('mlp_norm_w', 1 + 0.1 * rnd(43, D)), w(45, D, D), w(46, 2 * HIDDEN, D), w(47, D, HIDDEN)
  Lcap = MAXP * PG
  nbytes = int(L().plm_ragged_layer_paged_workspace_bytes(R, NH, HD, HIDDEN, Lcap))
  assert nbytes > 0
  wsp = ar.ws('workspace', nbytes)
  return lambda: call('plm_ragged_layer_paged_bf16', P(x), P(an), P(mn), EPS, P(wq), P(wo), P(w1), P(w2), P(l0), P(cu), P(rs), P(rc), P(rsn), MAXP * PG,
                      P(pool), LD, P(tb), P(status), R, B, NT, Lcap, MAXP, NP, NH, HD, HIDDEN, 0, P(wsp), nbytes)


CASES['kv_paged_append_rope_packed'] = (('plm_kv_paged_append_rope_packed',), _append)
CASES['attn_ragged_paged'] = (('plm_attn_ragged_paged', 'plm_attn_ragged_paged_workspace_bytes'), _attend)
CASES['ragged_norm_qkv_append_paged'] = (('plm_ragged_norm_qkv_append_paged_bf16',), lambda ar: _fused(ar, False))
CASES['ragged_layer_paged'] = (('plm_ragged_layer_paged_bf16', 'plm_ragged_layer_paged_workspace_bytes'), lambda ar: _fused(ar, True))


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
