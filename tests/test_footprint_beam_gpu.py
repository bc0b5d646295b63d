"""Where the launches of beam search read and write, on a real MI355X: one footprint case per new entry point on
tests/footprint.py's machinery.  The ancestor table is an index-valued input: its margins hold in-range slots."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402
from test_footprint_shared_gpu import EPS, _rope, rnd  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, I32, I64, U8 = torch.bfloat16, torch.float32, torch.int32, torch.int64, torch.uint8
CASES = {}
NP, G, NH, HD, TP, TS, HIDDEN = 2, 5, 2, 64, 300, 40, 96
D, M = NH * HD, NP * G
LENS_P = (257, 0)
ROWS = 34  # suffix rows held: either side of a 32-row tile
N_NEW, T_STEP, EOS = 9, 4, 7


def _anc(ar):
  g = torch.Generator().manual_seed(431)
  return ar.inp('anc', torch.randint(0, G, (M, TS), generator=g).to(U8), index_margin=(0, G - 1))


def _attn_case(splits_s, want_lse):
  def fn(ar):
    nbytes = int(L().plm_attn_decode_beam_workspace_bytes(NP, G, NH, HD, TP, TS, 0, splits_s))
    assert nbytes > 0
    q = ar.inp('q', rnd(401, M, D, dtype=BF16), misalign=True)
    kv_p = ar.inp('kv_p', rnd(403, NP * TP, 2 * D, dtype=BF16), ld=2 * D + 8)
    kv_s = ar.inp('kv_s', rnd(402, M * TS, 2 * D, dtype=BF16), ld=2 * D + 8)
    lp = ar.inp('lens_p', torch.tensor(LENS_P, dtype=I32), index_margin=(1, TP))
    ls = ar.inp('lens_s', torch.tensor([ROWS] * G + [TS] * G, dtype=I32), index_margin=(1, TS))
    anc = _anc(ar)
    out = ar.out('out', BF16, M, D)
    lse = ar.out('lse', F32, M * NH) if want_lse else None
    ws = ar.ws('workspace', nbytes)
    return lambda: call('plm_attn_decode_beam', P(q), P(kv_p), 2 * D + 8, P(lp), P(kv_s), 2 * D + 8, P(ls), P(anc), P(out), P(lse), NP, G, TP, TS, NH,
                        HD, 0, splits_s, P(ws), nbytes)
  return ('plm_attn_decode_beam', 'plm_attn_decode_beam_workspace_bytes'), fn


def _layer_case(ar):
  nbytes = int(L().plm_decode_layer_beam_workspace_bytes(NP, G, NH, HD, HIDDEN, TP, TS, 0, 0))
  assert nbytes > 0
  row = [ROWS - 1] * G + [TS - 1] * G
  x = ar.inout('x', rnd(421, M, D), misalign=True)
  an, mn = ar.inp('attn_norm_w', 1 + 0.1 * rnd(422, D)), ar.inp('mlp_norm_w', 1 + 0.1 * rnd(423, D))
  w_qkv = ar.inp('w_qkv', rnd(424, 3 * D, D, dtype=BF16, scale=0.1))
  w_out = ar.inp('w_out', rnd(425, D, D, dtype=BF16, scale=0.1))
  w_fc1 = ar.inp('w_fc1', rnd(426, 2 * HIDDEN, D, dtype=BF16, scale=0.1))
  w_fc2 = ar.inp('w_fc2', rnd(427, D, HIDDEN, dtype=BF16, scale=0.1))
  rw = ar.inp('row', torch.tensor(row, dtype=I32), index_margin=(0, TS - 1))
  ls = ar.inp('lens_s', torch.tensor([r + 1 for r in row], dtype=I32), index_margin=(1, TS))
  r0 = ar.inp('rot0', torch.tensor([LENS_P[i // G] for i in range(M)], dtype=I32), index_margin=(0, 1))
  lp = ar.inp('lens_p', torch.tensor(LENS_P, dtype=I32), index_margin=(1, TP))
  anc = _anc(ar)
  cos, sin = _rope(TP + TS)
  rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
  kv_p = ar.inp('kv_p', rnd(403, NP * TP, 2 * D, dtype=BF16), ld=2 * D + 8)
  rows = torch.zeros(M * TS, 2 * D, dtype=torch.bool)
  beyond = torch.ones(M * TS, 2 * D, dtype=torch.bool)
  for i, r in enumerate(row):
    rows[i * TS + r] = True
    beyond[i * TS:i * TS + r + 1] = False
  status = ar.inout('status', torch.zeros(1, dtype=I32), written=torch.tensor([False]), untouched=torch.tensor([True]))
  kv_s = ar.inout('kv_s', rnd(402, M * TS, 2 * D, dtype=BF16), ld=2 * D + 8, written=rows, untouched=beyond, unread=beyond | rows)
  ws = ar.ws('workspace', nbytes)
  return lambda: call('plm_decode_layer_beam_bf16', P(x), P(an), P(mn), EPS, P(w_qkv), P(w_out), P(w_fc1), P(w_fc2), P(rw), P(ls), P(r0), P(lp), P(anc),
                      P(rc), P(rs), TP + TS, P(kv_p), 2 * D + 8, P(kv_s), 2 * D + 8, P(status), NP, G, TP, TS, NH, HD, HIDDEN, 0, 0, 0, P(ws), nbytes)


def _select_case(V, rpp):
  def fn(ar):
    rows = NP * rpp
    nbytes = int(L().plm_beam_select_workspace_bytes(rows, G))
    assert nbytes > 0
    logits = ar.inp('logits', rnd(441, rows, V, dtype=BF16, scale=3.0), ld=V + 8, misalign=True)
    score = ar.inp('score', -rnd(442, rows).abs())
    cs, cb, ct = ar.out('cand_score', F32, NP * 2 * G), ar.out('cand_beam', I32, NP * 2 * G), ar.out('cand_tok', I32, NP * 2 * G)
    ws = ar.ws('workspace', nbytes)
    return lambda: call('plm_beam_select_bf16', P(logits), V + 8, P(score), P(cs), P(cb), P(ct), NP, rpp, G, V, P(ws), nbytes)
  return ('plm_beam_select_bf16', 'plm_beam_select_workspace_bytes'), fn


def _histories(ar, role):
  g = torch.Generator().manual_seed(451)
  th, ph = torch.randint(0, 50, (NP * N_NEW, G), generator=g).to(I32), torch.randint(0, G, (NP * N_NEW, G), generator=g).to(I32)
  if role == 'in':
    return ar.inp('tok_hist', th), ar.inp('par_hist', ph, index_margin=(0, G - 1))
  step = torch.zeros(NP * N_NEW, G, dtype=torch.bool)
  step[[p * N_NEW + T_STEP for p in range(NP)]] = True
  return ar.inout('tok_hist', th, written=step, untouched=~step), ar.inout('par_hist', ph, written=step, untouched=~step)


def _pool(ar, role):
  add = ar.inp if role == 'in' else ar.inout
  pf = add('pool_f', torch.tensor([[-1.0, -3.0], [-2.0, -8.0]] * G).reshape(NP * G, 2)[:NP * G])
  pi = add('pool_i', torch.tensor([[3, 1, 2]] * (NP * G), dtype=I32), **({'index_margin': (1, 1)} if role == 'in' else {}))
  pn = add('pool_n', torch.tensor([2, G], dtype=I32), **({'index_margin': (0, G)} if role == 'in' else {}))
  done = add('done', torch.tensor([0, 0], dtype=I32), **({'index_margin': (0, 1)} if role == 'in' else {}))
  return pf, pi, pn, done


def _advance_case(ar):
  cs = ar.inp('cand_score', (-0.5 * torch.arange(2 * G, dtype=F32)).repeat(NP, 1), misalign=True)
  cb = ar.inp('cand_beam', torch.tensor([[0, 2, 2, 1, 4, 3, 0, 1, 2, 4], [1, 1, 0, 3, 3, 2, 4, 0, -1, -1]], dtype=I32), index_margin=(0, G - 1))
  ct = ar.inp('cand_tok', torch.tensor([[9, EOS, 3, 4, 5, EOS, 6, 8, 1, 2], [EOS, 2, 3, EOS, 5, 6, EOS, 9, -1, -1]], dtype=I32), index_margin=(0, 1))
  g = torch.Generator().manual_seed(452)
  anc_in = ar.inp('anc_in', torch.randint(0, G, (M, N_NEW), generator=g).to(U8), index_margin=(0, G - 1))
  cols = torch.zeros(M, N_NEW, dtype=torch.bool)
  cols[:, :T_STEP + 1] = True
  anc_out = ar.out('anc_out', U8, M, N_NEW, written=cols, untouched=~cols)
  tok, sc, par = ar.out('tok_next', I64, M), ar.out('score_out', F32, M), ar.out('parent', I32, M)
  th, ph = _histories(ar, 'inout')
  pf, pi, pn, done = _pool(ar, 'inout')
  return lambda: call('plm_beam_advance', P(cs), P(cb), P(ct), P(anc_in), P(anc_out), P(tok), P(sc), P(par), P(th), P(ph), P(pf), P(pi), P(pn), P(done),
                      NP, G, N_NEW, T_STEP, EOS, 1.0, 0)


def _finalize_case(ar):
  R = 3
  score = ar.inp('score', -rnd(461, M).abs(), misalign=True)
  th, ph = _histories(ar, 'in')
  pf, pi, pn, done = _pool(ar, 'in')
  tokens, lengths, scores = ar.out('tokens', I64, NP * R, N_NEW), ar.out('lengths', I32, NP * R), ar.out('scores', F32, NP * R)
  return lambda: call('plm_beam_finalize', P(score), P(th), P(ph), P(pf), P(pi), P(pn), P(done), P(tokens), P(lengths), P(scores), NP, G, N_NEW, N_NEW,
                      R, EOS, 0, 1.0)


CASES['attn_decode_beam-auto-lse'] = _attn_case(0, True)
CASES['attn_decode_beam-splits2-nolse'] = _attn_case(2, False)
CASES['decode_layer_beam-auto'] = (('plm_decode_layer_beam_bf16', 'plm_decode_layer_beam_workspace_bytes'), _layer_case)
CASES['beam_select-first-step'] = _select_case(50280, 1)
CASES['beam_select-V1000'] = _select_case(1000, G)
CASES['beam_advance'] = (('plm_beam_advance',), _advance_case)
CASES['beam_finalize'] = (('plm_beam_finalize',), _finalize_case)


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
