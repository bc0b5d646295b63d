"""Beam search on a real MI355X: plm_attn_decode_beam against an fp64 softmax over the gathered keys under
test_shared_gpu's bounds (control: plm_attn_decode_shared on a suffix cache gathered with torch) and its bit equalities; plm_beam_select_bf16
against an fp64 top-2G; the whole search on a table model against a plain Python beam search; generate_beam on the golden 2-layer model.

SELECT_ERR, the fp32 error of a candidate's score = score[g] + logp against fp64, from sample_common.h's stated weight error plus fp32
rounding: Z is within 1.2e-7 ln V of itself (the weights' two argument roundings) plus V * 2^-40 (a truncation below 2^-40 per weight,
Z >= 1), and its conversion to fp32 adds 2^-24, all relative to Z, so absolute in ln Z; logf is good to 2 ulp of |ln Z| <= ln V, i.e.
2^-22 ln V; x - x_max, its difference with ln Z, and the sum with score[g] each round once, 2^-24 of the largest magnitude involved."""

import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_decode_gpu as TD  # noqa: E402
import test_shared_gpu as TS  # noqa: E402

BF16 = torch.bfloat16
biteq, i32 = TD.biteq, TS.i32
NP, NH, TP, TSUF, GMAX = TS.NP, TS.NH, 300, 70, 32
LENS_P = (300, 256)  # one of them no multiple of 64


def SELECT_ERR(V, mag):
  return math.log(V) * (1.2e-7 + 2.0 ** -22) + V * 2.0 ** -40 + 2.0 ** -24 + 3 * 2.0 ** -24 * mag


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


_data = {}


def data(hd):
  """q [NP*GMAX, d], kv_p [NP, TP, 2d], kv_s [NP*GMAX, TSUF, 2d] bf16 on the GPU, drawn once per head dim and never modified."""
  if hd not in _data:
    g = torch.Generator().manual_seed(2300 + hd)
    d = NH * hd
    _data[hd] = tuple(torch.randn(*s, generator=g).to(BF16).cuda() for s in ((NP * GMAX, d), (NP, TP, 2 * d), (NP * GMAX, TSUF, 2 * d)))
  return _data[hd]


def ancestry(kind, G, rows, seed=0):
  """anc uint8 [NP*G, TSUF]: identity, every beam on one slot, or a random trie (random parents per step); 200 (no slot) beyond ``rows``."""
  rng = np.random.default_rng(seed)
  anc = np.full((NP, G, TSUF), 200, np.uint8)
  for p in range(NP):
    for j in range(rows):
      if kind == 'trie':
        anc[p, :, :j] = anc[p, rng.integers(0, G, G), :j]
      anc[p, :, j] = (p + 1) % G if kind == 'collapsed' else np.arange(G)
  return torch.from_numpy(anc.reshape(NP * G, TSUF)).cuda()


def gathered(kv_s, anc, G):
  """The suffix cache a re-parenting gather would hold: row j of beam i = row j of slot anc[i][j] (rows no beam reads: slot G - 1's)."""
  seq = (torch.arange(NP * G, device='cuda') // G * G)[:, None] + anc.clamp(max=G - 1).long()
  return kv_s[seq, torch.arange(TSUF, device='cuda')[None, :]].contiguous()


@pytest.mark.parametrize('kind', ['identity', 'collapsed', 'trie'])
@pytest.mark.parametrize('rows', [0, 1, 31, 33, 70])
@pytest.mark.parametrize('G', [1, 5, 32])
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_decode_beam_vs_fp64_and_the_gathered_control(ops, hd, G, rows, kind):
  q, kv_p, kv_s = data(hd)
  M = NP * G
  q, kv_s, anc, ls = q[:M], kv_s[:M], ancestry(kind, G, rows, seed=rows), [rows] * M
  gat = gathered(kv_s, anc, G)
  want_o, want_l = TS.reference(q, kv_p, LENS_P, gat, ls, G, hd)
  for ss in (0, 2):
    out, lse = ops.attn_decode_beam(q, kv_p, i32(LENS_P), kv_s, i32(ls), anc, NH, splits_s=ss, want_lse=True)
    TS.check_vs_fp64(f'beam hd={hd} G={G} rows={rows} {kind} splits_s={ss}', out, lse, want_o, want_l, hd)
  co, cl = ops.attn_decode_shared(q, kv_p, i32(LENS_P), gat, i32(ls), NH, want_lse=True)
  TS.check_vs_fp64(f'control hd={hd} G={G} rows={rows} {kind}', co, cl, want_o, want_l, hd)


@pytest.mark.parametrize('G', [5, 32])
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_decode_beam_bit_equalities(ops, hd, G):
  q0, kv_p, kv_s0 = data(hd)
  M, rows, i = NP * G, 33, G + 2  # beam 2 of prompt 1
  q, kv_s, anc, ls = q0[:M], kv_s0[:M], ancestry('trie', G, rows, seed=9), [rows] * M
  run = lambda q_, ks_, anc_: ops.attn_decode_beam(q_, kv_p, i32(LENS_P), ks_, i32(ls), anc_, NH, want_lse=True)  # noqa: E731
  out, lse = run(q, kv_s, anc)
  o2, l2 = run(q, kv_s, anc)
  assert biteq(o2, out) and torch.equal(l2, lse)
  other = torch.Generator().manual_seed(5)
  q3 = torch.randn(q.shape, generator=other).to(BF16).cuda()  # the other beams' queries
  q3[i] = q[i]
  o3, l3 = run(q3, kv_s, anc)
  assert biteq(o3[i], out[i]) and torch.equal(l3[i], lse[i])
  ks4, anc4 = kv_s.clone(), anc.clone()  # rows and table entries at and beyond lens_s: NaN, and a slot that exists
  ks4[:, rows:] = float('nan')
  anc4[:, rows:] = 0
  o4, l4 = run(q, ks4, anc4)
  assert biteq(o4, out) and torch.equal(l4, lse)
  ks5 = torch.randn(kv_s.shape, generator=other).to(BF16).cuda()  # other finite values in every row beam i does not attend
  seq = (i // G * G + anc[i, :rows].long())
  ks5[seq, torch.arange(rows, device='cuda')] = kv_s[seq, torch.arange(rows, device='cuda')]
  o5, l5 = run(q, ks5, anc)
  assert biteq(o5[i], out[i]) and torch.equal(l5[i], lse[i])


# ---- selection ---------------------------------------------------------------------------------------------------------------------------
def select_reference(logits, score, G, rpp):
  """fp64: per prompt the candidates (score, beam, token) of every finite logit of every beam with a finite score, in the stated order."""
  x = logits.double()
  fin = torch.isfinite(x)
  logp = x - torch.logsumexp(torch.where(fin, x, torch.full_like(x, -math.inf)), dim=1, keepdim=True)
  res = []
  for p in range(x.shape[0] // rpp):
    c = []
    for g in range(rpp):  # (a row's candidates below its own (2G + 1)-th value cannot be among the prompt's best 2G + 1)
      row = torch.where(fin[p * rpp + g], logp[p * rpp + g], torch.full_like(logp[0], -math.inf))
      kth = torch.topk(row, min(2 * G + 1, row.shape[0])).values[-1]
      if math.isfinite(score[p * rpp + g].item()):
        c += [(score[p * rpp + g].item() + row[v].item(), g, v) for v in torch.nonzero(fin[p * rpp + g] & (row >= kth))[:, 0].tolist()]
    res.append(sorted(c, key=lambda t: (-t[0], t[1], t[2]))[:2 * G + 1])
  return res


def select_rows(V, G, seed):
  """G rows per prompt, 2 prompts, ld > V: prompt 0 random rows and scores; prompt 1 rows of few distinct values (exact ties), two beams
  with one row and one score (ties across beams), a row holding NaN and +inf, and (G > 1) a beam at -inf."""
  g = torch.Generator().manual_seed(seed)
  x = (3 * torch.randn(2 * G, V + 8, generator=g)).to(BF16)
  x[G:] = (torch.randint(0, 5, (G, V + 8), generator=g).float() * 0.5).to(BF16)
  score = -10 * torch.rand(2 * G, generator=g)
  x[G, 3], x[G, 7] = float('nan'), float('inf')
  if G > 1:
    score[G] = 0.0  # the best beam of its prompt, and its twin
    x[2 * G - 1], score[2 * G - 1] = x[G], score[G]
    score[G + 1] = -math.inf
  return x, score.float()


@pytest.mark.parametrize('G', [1, 4, 32])
@pytest.mark.parametrize('V', [64, 1000, 50280])
def test_beam_select_vs_fp64(ops, V, G):
  x, score = select_rows(V, G, seed=8)
  cs, cb, ct = (t.cpu() for t in ops.beam_select(x.cuda()[:, :V], score.cuda(), G, G))
  cs2, cb2, ct2 = (t.cpu() for t in ops.beam_select(x.cuda()[:, :V], score.cuda(), G, G))
  assert torch.equal(cs, cs2) and torch.equal(cb, cb2) and torch.equal(ct, ct2)  # two runs
  err = SELECT_ERR(V, 40.0)
  for p, ref in enumerate(select_reference(x[:, :V], score, G, G)):
    gaps = [a[0] - b[0] for a, b in zip(ref, ref[1:])]
    assert all(d == 0 or d > 2 * err for d in gaps), (p, min(d for d in gaps if d > 0))  # the reference alone: exact ties or clear gaps
    n = min(len(ref), 2 * G)
    got = list(zip(cb[p, :n].tolist(), ct[p, :n].tolist()))
    assert got == [(g, v) for _, g, v in ref[:n]], (p, got, ref)
    worst = max(abs(cs[p, r].item() - ref[r][0]) for r in range(n))
    print(f'beam_select V={V} G={G} prompt {p}: |score - fp64| {worst:.2e} (bound {err:.2e})')
    assert worst <= err
    assert (cb[p, n:] == -1).all() and (ct[p, n:] == -1).all() and (cs[p, n:] == -math.inf).all()


# ---- the whole search on a table model --------------------------------------------------------------------------------------------------------
def python_beam_search(first, table, N, G, R, lp, early, eos):
  """Plain fp64 beam search of one prompt: first [V] and table [V, V] log-probabilities.  The pool and termination rules of plm_beam_advance."""
  beams, pool, done = [(0.0, [])], [], False  # (score, tokens)

  def keep(hyp):  # the G best by normalised score; an equal newcomer does not displace
    w = min(range(len(pool)), key=lambda e: pool[e][0]) if len(pool) >= G else None
    if w is None:
      pool.append(hyp)
    elif hyp[0] > pool[w][0]:
      pool[w] = hyp
  for t in range(N):
    rows = [first] if t == 0 else [table[b[1][-1]] for b in beams]
    cand = sorted(((beams[g][0] + rows[g][v], g, v) for g in range(len(beams)) for v in range(len(first))), key=lambda c: (-c[0], c[1], c[2]))[:2 * G]
    nxt = []
    for r, (sc, g, v) in enumerate(cand):
      if eos is not None and v == eos:
        if r < G and not done:
          keep((sc / (t + 1) ** lp, beams[g][1] + [v]))
        continue
      if len(nxt) < G:
        nxt.append((sc, beams[g][1] + [v]))
    beams = nxt
    if not done and len(pool) >= G and (early or not beams[0][0] / (t + 1) ** lp > min(h[0] for h in pool)):
      done = True
  if not done:
    for sc, toks in beams:
      keep((sc / N ** lp, toks))
  return sorted(pool, key=lambda h: -h[0])[:R]


_table = {}


def table_model():
  if not _table:
    g = torch.Generator().manual_seed(46)  # the fp64 search alone: no two candidates or hypotheses within 3e-4, equal logits of one beam excepted
    _table['t'] = (2 * torch.randn(64, 64, generator=g)).to(BF16)
    _table['f'] = (2 * torch.randn(2, 64, generator=g)).to(BF16)
    _table['lt'], _table['lf'] = (torch.log_softmax(_table[k].double(), dim=-1).tolist() for k in ('t', 'f'))
    _table['dev'] = _table['t'].cuda()
  return _table


@pytest.mark.parametrize('ret_all', [False, True])
@pytest.mark.parametrize('early', [False, True])
@pytest.mark.parametrize('lp', [0.0, 1.0, 2.0])
@pytest.mark.parametrize('eos', [None, 5])
@pytest.mark.parametrize('G', [1, 3, 8])
def test_beam_loop_on_a_table_model_vs_python(ops, G, eos, lp, early, ret_all):
  from plainlm_amd.generate import beam_loop
  T, N, R = table_model(), 12, G if ret_all else 1
  tokens, lengths, scores = (t.cpu() for t in beam_loop(T['f'].cuda(), lambda tok: T['dev'][tok], N, G, R, lp, early, eos, pad_id=63, check_every=4))
  assert tuple(tokens.shape) == (2, R, N) and tokens.dtype == torch.int64
  for p in range(2):
    want = python_beam_search(T['lf'][p], T['lt'], N, G, R, lp, early, eos)
    assert lengths[p].tolist() == [len(h[1]) for h in want], (p, lengths[p], want)
    for r, (sc, toks) in enumerate(want):
      assert tokens[p, r].tolist() == toks + [63] * (N - len(toks)), (p, r)
      assert abs(scores[p, r].item() - sc) <= N * SELECT_ERR(64, 64.0), (p, r, scores[p, r].item(), sc)


# ---- the model ------------------------------------------------------------------------------------------------------------------------------
from test_shared_gpu import mdl, model  # noqa: E402,F401  (the golden 2-layer model's fixtures)


@pytest.mark.parametrize('G', [1, 4])
def test_generate_beam_rescored_by_the_full_forward(ops, model, mdl, G):
  """Every returned hypothesis, re-scored by the full forward over prompt + hypothesis: the mean log-probability is the returned score under
  test_decode_gpu's teacher-forced bound (2e-2 of the largest logit, per logit: twice that per log-probability).  A wrong ancestor anywhere in
  the attention shows up here."""
  prompt, N = mdl['tokens'][:, :16].cuda(), 8
  res = {}
  with torch.no_grad():
    for fused in (False, True):
      res[fused] = model.generate_beam(prompt, N, G, num_return=G, fused=fused)
      again = model.generate_beam(prompt, N, G, num_return=G, fused=fused)
      assert all(torch.equal(a, b) for a, b in zip(res[fused], again))  # two calls, bit for bit
      tokens, lengths, scores = res[fused]
      assert tuple(tokens.shape) == (2, G, N) and (lengths == N).all() and (scores[:, :-1] >= scores[:, 1:]).all()
      for g in range(G):
        seq = torch.cat([prompt, tokens[:, g]], dim=1)
        bound = 2 * 2e-2 * model(seq, None).float().abs().max().item()
        lp = model.token_logprobs(seq, torch.cat([seq[:, 1:], seq[:, :1]], dim=1))[:, 15:15 + N].mean(dim=1)
        e = (lp - scores[:, g]).abs().max().item()
        print(f'generate_beam fused={fused} G={G} hypothesis {g}: |score - full forward| {e:.2e} (bound {bound:.2e})')
        assert e <= bound, (fused, g, e, bound)
  assert (res[True][2] - res[False][2]).abs().max().item() <= bound  # fused and unfused agree under that bound
