"""Draft-free speculative decoding on a real MI355X: plm_lookup_draft_i64 bit-equal to tests/lookup_ref.py,
plm_spec_verify_lookup_bf16 against the fp64 restatement of its rule, determinism and sequence independence of both, and
Transformer.generate_lookup on the 2-layer golden model.

Bounds of the acceptance kernel (derived from sample.hip's stated weight error as tests/test_spec_gpu.py derives its own, not measured;
the observed figures are printed and recorded in DESIGN.md section 16).  A fixed-point weight w (relative to the row maximum's 1) is
off by at most 1.2e-7 |ln w| of itself plus 2^-40 of truncation, and any sum of weights by 1.2e-7 ln V + V 2^-40 of Z (Z >= 1):
    e_w(w) = 1.2e-7 |ln w| + 2^-40 / w        e_Z = 1.2e-7 ln V + V 2^-40
  accept     alpha = w_x / Z carries ONE weight error and ONE Z error (the draft is one-hot: there is no q(x) and no second Z), and the
             integer test floor(u Z) < w_x is u Z < w_x exactly (w_x is an integer; the fp64 product u Z adds 2^-53).  So the kernel's
             alpha is within d = 2 * alpha * (e_w(w_x) + e_Z) of the reference's (2x slack, as test_spec_gpu.py takes it): row r must be
             accepted when u < alpha - d and rejected when u > alpha + d; in between - the band - either verdict is right and nothing is
             asserted.  alpha = 0 (token outside [0, V) or outside the kept set) is exact: d = 0.  The band may not hide the test: for the
             reference alone at most 5 % of the drafted rows of a case may lie inside it (BAND_SHARE), which is asserted.
  residual   the residual weight of a column is the column's own weight, so a partial sum C_i / Z carries the weights' sum error and
             Z's, delta = 2 e_Z, an ABSOLUTE error in units of probability; R = (Z - w_x) / Z carries the same.  The kernel's token
             satisfies C_prev <= u R < C_tok on its own integers, so on the reference's: C_prev - t <= u R <= C_tok + t with
             t = 2 * (delta + delta) = 4 delta (the sum's error and R's, 2x slack).  The kernel's R can be 0 only where the reference's
             R <= delta: the fallback (the target sampler's token) is accepted for R <= 4 delta.
  logp       within LOGP_TOL = 3e-5 nats of the fp64 log softmax (test_sample_gpu.py's bound), exactly 0 beyond n_accept.

"Rows at and beyond n_prop[b] are never loaded" is checked as the header states it: the proposal entries draft_tok[b, r], the uniforms
u_accept[r, b] and the verdict of every row r >= n_prop[b], and the logits, cutoff and sampler token of every chunk row beyond n_prop[b].
Chunk row n_prop[b] itself is a real row of the round (the chunk is [last | proposal]): the bonus token and its log-probability are
read from it."""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lookup_ref as LR  # noqa: E402
import sample_ref as R  # noqa: E402
import spec_ref as S  # noqa: E402
from test_sample_gpu import LOGIT_TOL, LOGP_MODEL_TOL, LOGP_TOL, TAUS  # noqa: E402

BF16, I32, I64 = torch.bfloat16, torch.int32, torch.int64
FIX = 2.0 ** -40
FILTERS = ((0, 1.0), (50, 0.95))  # an unfiltered and a filtered cutoff
BAND_SHARE = 0.05
SENTINEL = -(1 << 40)


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


# ================================================================================================================================================
# plm_lookup_draft_i64
# ================================================================================================================================================
LENS = (0, 1, 2, 3, 255, 256, 257, 300)
NGRAMS = ((1, 1), (2, 4), (1, 16))


def _history(rng, L, ld, alphabet, kind):
  h = rng.integers(0, alphabet, ld)
  if kind == 'first' and L >= 3:      # the only earlier occurrence of the last token is hist[0]: the winner is e = 1
    h[:L] = 1 + rng.integers(0, alphabet - 1, L) if alphabet > 2 else 1
    h[0] = h[L - 1] = 0
  if kind == 'last' and L >= 2:       # the last two tokens are equal: e = L - 1 is a candidate, and the most recent
    h[L - 2] = h[L - 1]
  return h


def _draft_case(B, L, k, n_add, with_add, seed):
  """Host arrays of one launch.  Sequence b has length L before the append (the last one L // 2, so a batch is ragged); the histories
  beyond it hold a sentinel."""
  rng = np.random.default_rng(seed)
  ld = L + 40
  lens = np.array([L if b < B - 1 or B == 1 else L // 2 for b in range(B)], dtype=np.int32)
  hist = np.full((B, ld), SENTINEL, dtype=np.int64)
  for b in range(B):
    alphabet = 2 + (b + seed) % 3
    hist[b, :lens[b]] = _history(rng, int(lens[b]), ld, alphabet, ('rand', 'first', 'last')[(b + seed // 3) % 3])[:lens[b]]
  add = rng.integers(0, 2 + seed % 3, (B, k + 1)) if with_add else None
  na = None
  if with_add and n_add is not None:
    na = np.full(B, n_add, dtype=np.int32)
    if B > 1:
      na[1] = k + 9       # clamped to the width of add_tok
      na[B - 1] = -3      # clamped to 0
  return hist, lens, add, na


def _launch_draft(ops, hist, lens, add, na, k, ngram):
  dev = lambda a, dt: None if a is None else torch.as_tensor(a).to(dt).cuda()  # noqa: E731
  h, ln = dev(hist, I64), dev(lens, I32)
  status = torch.zeros(1, dtype=I32, device='cuda')
  r = ops.lookup_draft(h, ln, dev(add, I64), dev(na, I32), k=k, ngram=ngram, status=status)
  return dict(hist=h.cpu().numpy(), lens=ln.cpu().numpy(), draft=r.draft_tokens.cpu().numpy(), n_prop=r.n_prop.cpu().numpy(),
              match_len=r.match_len.cpu().numpy(), status=int(status.item()))


def _same(got, want, tag):
  for name in ('hist', 'lens', 'draft', 'n_prop', 'match_len'):
    assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (tag, name, got[name], want[name])
  assert got['status'] == want['status'], tag


@pytest.mark.parametrize('B', [1, 5])
@pytest.mark.parametrize('L', LENS)
def test_lookup_draft_is_bit_equal_to_the_reference(ops, B, L):
  hits = winners_first = winners_last = 0
  for i, (k, ngram) in enumerate((k, g) for k in (1, 4, 31) for g in NGRAMS):
    for n_add, with_add in ((0, True), (1, True), (k + 1, True), (None, True), (None, False)):
      seed = 10 * L + i
      hist, lens, add, na = _draft_case(B, L, k, n_add, with_add, seed)
      want = LR.lookup(hist, lens, add, na, k, ngram)
      got = _launch_draft(ops, hist, lens, add, na, k, ngram)
      tag = (B, L, k, ngram, n_add, with_add)
      _same(got, want, tag)
      assert want['status'] == 0
      for b in range(B):   # beyond the append the sentinel is untouched (also part of the equality above)
        assert (got['hist'][b, want['lens'][b]:] == SENTINEL).all(), tag
        if want['n_prop'][b]:
          hits += 1
          e = int(want['lens'][b]) - 1
          winners_last += LR.match_len(want['hist'][b], e + 1, e, ngram[1]) == want['match_len'][b]
          winners_first += want['match_len'][b] == 1 and np.array_equal(want['draft'][b][:1], want['hist'][b][1:2]) and \
              not any(LR.match_len(want['hist'][b], e + 1, x, ngram[1]) >= ngram[0] for x in range(2, e + 1))
      assert _same(_launch_draft(ops, hist, lens, add, na, k, ngram), got, tag) is None   # two runs are bit-equal
  if L >= 3:
    assert hits > 0 and winners_last > 0, (hits, winners_last)
  if L >= 255:
    assert winners_first > 0


def test_lookup_draft_row_that_does_not_fit_and_sequence_independence(ops):
  B, k, ld = 5, 4, 64
  rng = np.random.default_rng(5)
  hist = np.full((B, ld), SENTINEL, dtype=np.int64)
  lens = np.array([10, 62, 30, 64, 3], dtype=np.int32)
  for b in range(B):
    hist[b, :lens[b]] = rng.integers(0, 3, lens[b])
  add = rng.integers(0, 3, (B, k + 1))
  na = np.array([k + 1, 3, 2, 1, 0], dtype=np.int32)   # sequence 1: 62 + 3 > 64, sequence 3: 64 + 1 > 64
  want = LR.lookup(hist, lens, add, na, k, (1, 4))
  got = _launch_draft(ops, hist, lens, add, na, k, (1, 4))
  _same(got, want, 'refused')
  assert got['status'] == 1 and got['lens'].tolist() == [15, 62, 32, 64, 3] and got['n_prop'][[1, 3]].tolist() == [0, 0]
  assert np.array_equal(got['hist'][[1, 3]], hist[[1, 3]]) and (got['draft'][[1, 3]] == 0).all()   # nothing stored
  # the other sequences do not see them: alone in fitting company, they give the same bits
  keep = [0, 2, 4]
  alone = _launch_draft(ops, hist[keep], lens[keep], add[keep], na[keep], k, (1, 4))
  assert alone['status'] == 0
  for name in ('hist', 'lens', 'draft', 'n_prop', 'match_len'):
    assert np.array_equal(alone[name], got[name][keep]), name
  # a negative length is refused as well
  lens2 = lens.copy()
  lens2[0] = -1
  got2 = _launch_draft(ops, hist, lens2, add, na, k, (1, 4))
  assert got2['status'] == 1 and got2['lens'][0] == -1 and np.array_equal(got2['hist'][0], hist[0]) and got2['n_prop'][0] == 0


def test_lookup_draft_refuses_what_the_wrapper_can_see(ops):
  z = lambda *s, dt=I64: torch.zeros(*s, dtype=dt, device='cuda')  # noqa: E731
  r = ops.lookup_draft(z(2, 8), z(2, dt=I32), k=3)
  assert r.n_prop.tolist() == [0, 0] and r.draft_tokens.tolist() == [[0] * 3] * 2 and r.match_len.tolist() == [0, 0]
  with pytest.raises(TypeError):
    ops.lookup_draft(z(2, 8, dt=I32), z(2, dt=I32), k=3)
  with pytest.raises(ValueError, match='lens'):
    ops.lookup_draft(z(2, 8), z(3, dt=I32), k=3)
  with pytest.raises(ValueError, match='n_add without add_tok'):
    ops.lookup_draft(z(2, 8), z(2, dt=I32), n_add=z(2, dt=I32), k=3)
  with pytest.raises(ValueError, match='add_tok'):
    ops.lookup_draft(z(2, 8), z(2, dt=I32), add_tok=z(3, 2), k=3)
  with pytest.raises(RuntimeError, match='drafted tokens'):
    ops.lookup_draft(z(2, 8), z(2, dt=I32), k=32)
  with pytest.raises(RuntimeError, match='ngram'):
    ops.lookup_draft(z(2, 8), z(2, dt=I32), k=3, ngram=(2, 1))


# ================================================================================================================================================
# plm_spec_verify_lookup_bf16
# ================================================================================================================================================
KINDS = ('rand1', 'peaked', 'rand8', 'ties', 'nonfinite', 'bad_tok', 'unkept')
VS, BS, KS = (1, 7, 257, 1000, 50280), (1, 5), (1, 4, 8)
observed = {'accept': 0.0, 'residual': 0.0, 'logp': 0.0, 'between': 0, 'rows': 0, 'accepted': 0, 'resid_draws': 0, 'fallbacks': 0,
            'drafted': 0, 'in_band': 0}


def e_w(lnw):
  return 1.2e-7 * abs(lnw) + FIX * np.exp(min(-lnw, 700.0))


def e_z(V):
  return 1.2e-7 * np.log(V) + V * FIX


def seq_rows(kind, V, k, g):
  """Target rows fp32 [k + 1, V] of one sequence of the named class."""
  rn = lambda s: torch.randn(k + 1, V, generator=g) * s  # noqa: E731
  if kind == 'rand8':
    return rn(8.0)
  if kind == 'ties':
    return torch.round(rn(2.0))
  if kind == 'peaked':  # p sits (almost) entirely on one column per row
    x = rn(1.0)
    x[torch.arange(k + 1), torch.randint(V, (k + 1,), generator=g)] += 60.0
    return x
  x = rn(1.0)
  if kind == 'nonfinite':
    m = torch.rand(x.shape, generator=g)
    x[m < 0.2] = float('-inf')
    x[m > 0.9] = float('nan')
  return x  # rand1, bad_tok, unkept


_cases = {}


def case(V, B, k, padded=0):
  key = (V, B, k, padded)
  if key not in _cases:
    g = torch.Generator().manual_seed(2000 * V + 10 * B + k)
    off = VS.index(V) + 2 * KS.index(k) if V in VS and k in KS else 0
    kinds = [KINDS[(b + off) % len(KINDS)] for b in range(B)]
    xp = torch.stack([seq_rows(kd, V, k, g) for kd in kinds]).to(BF16)  # [B, k + 1, V]
    n_prop = np.array([(k, 0, (k + 1) // 2, 1, k)[(b + off) % 5] for b in range(B)], dtype=np.int32)
    if B == 1:
      n_prop[:] = k
    if not padded:
      dp = xp.reshape(B * (k + 1), V).cuda()
    else:
      buf = torch.full((B * (k + 1), V + 13), float('nan'), dtype=BF16, device='cuda')
      buf[:, :V].copy_(xp.reshape(B * (k + 1), V))
      dp = buf[:, :V]
    _cases[key] = dict(V=V, B=B, k=k, kinds=kinds, xp=xp.double().numpy(), dp=dp, n_prop=n_prop)
  return _cases[key]


def prepare(ops, c, tau, top_k, top_p, rng):
  """The inputs as generate_lookup makes them: the sampler runs on the device and hands over its tokens and cutoffs.  The proposal:
  the row's most likely token at even rows (alpha is large), the sampler's own token or a random column at odd ones; then the planted
  tokens of the classes."""
  V, B, k = c['V'], c['B'], c['k']
  f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).cuda()  # noqa: E731
  st = ops.sample_logits(c['dp'], f32(rng.uniform(0, 1, B * (k + 1))), tau, top_k, top_p, want_stats=True)
  ptok = st.tokens.cpu().numpy().reshape(B, k + 1)
  tok = np.zeros((B, k), dtype=np.int64)
  for b, kind in enumerate(c['kinds']):
    for r in range(k):
      row = c['xp'][b, r]
      fin = np.where(np.isfinite(row), row, -np.inf)
      tok[b, r] = int(fin.argmax()) if r % 2 == 0 else (int(ptok[b, r]) if r % 4 == 1 else int(rng.integers(0, V)))
    if kind == 'bad_tok':
      tok[b, k // 2] = V + 3 if V % 2 else -1
    if kind == 'unkept':   # the lowest finite logit: outside the kept set under a filter, a tiny weight without one
      tok[b, 0] = int(np.where(np.isfinite(c['xp'][b, 0]), c['xp'][b, 0], np.inf).argmin())
  return dict(tok=torch.as_tensor(tok).cuda(), n_prop=torch.as_tensor(c['n_prop']).cuda(), pcut=st.cutoff, ptok=st.tokens)


def launch(ops, c, inp, ua, ures, tau):
  f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).cuda()  # noqa: E731
  r = ops.spec_verify_lookup(c['dp'], inp['tok'], inp['n_prop'], inp['pcut'], inp['ptok'], f32(ua), f32(ures), tau)
  return tuple(t.cpu().numpy() for t in r)


def same_bits(a, b):
  return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


def alpha_and_band(c, Pd, x):
  al = LR.alpha(Pd, x)
  exact = not 0 <= x < c['V'] or Pd.prob[x] == 0
  return al, (0.0 if exact else 2 * al * (e_w(Pd.lnw[x]) + e_z(c['V']))), exact


def uniforms_outside_the_band(c, dist_p, tok, n_prop, ua, rng):
  """The case's acceptance uniforms, chosen: a random uniform that lies inside the reference's band is drawn again (the special values
  stay what they are).  Returns (ua, rows drafted, rows inside the band for the reference alone)."""
  ua = np.array(ua, dtype=np.float64)
  drafted = inside = 0
  uc = R.clamp_u(ua.astype(np.float32))
  for b in range(c['B']):
    for r in range(int(np.clip(n_prop[b], 0, c['k']))):
      al, d, exact = alpha_and_band(c, dist_p(b, r), int(tok[b, r]))
      drafted += 1
      if not exact and abs(float(uc[r, b]) - al) <= d:
        if 0.0 < ua[r, b] < R.U_MAX and d < 0.25:
          while abs(float(np.float32(ua[r, b])) - al) <= d:
            ua[r, b] = rng.uniform(0, 1)
        else:
          inside += 1
  return ua, drafted, inside


def check(c, inp, ua, ures, tau, got, tag, dist_p):
  V, B, k = c['V'], c['B'], c['k']
  n_acc, nxt, logp = got
  tok, pcut, ptok, n_prop = (inp[n].cpu().numpy() for n in ('tok', 'pcut', 'ptok', 'n_prop'))
  ptok = ptok.reshape(B, k + 1)
  assert n_acc.dtype == np.int32 and nxt.dtype == np.int64 and logp.dtype == np.float32 and logp.shape == (B, k + 1)
  assert ((n_acc >= 0) & (n_acc <= np.clip(n_prop, 0, k))).all() and ((nxt >= 0) & (nxt < V)).all(), (tag, n_acc, n_prop, nxt)
  uc = R.clamp_u(np.asarray(ua, dtype=np.float32))
  delta = 2 * e_z(V)
  for b in range(B):
    t = tag + (b, c['kinds'][b])
    na, npb = int(n_acc[b]), int(np.clip(n_prop[b], 0, k))
    for r in range(min(na + 1, npb)):
      Pd = dist_p(b, r)
      x = int(tok[b, r])
      al, d, exact = alpha_and_band(c, Pd, x)
      u = float(uc[r, b])
      observed['rows'] += 1
      if r < na:   # the kernel accepted row r
        observed['accepted'] += 1
        assert not u > al + d, (t, r, 'accepted', u, al, d)
        miss = u - al
        ref = Pd.logp[x]
        assert abs(float(logp[b, r]) - ref) <= LOGP_TOL, (t, r, logp[b, r], ref)
        observed['logp'] = max(observed['logp'], abs(float(logp[b, r]) - ref))
      else:        # the kernel rejected row r
        assert not u < al - d, (t, r, 'rejected', u, al, d)
        miss = al - u
      if miss >= 0 and not exact:    # inside the band: how much of it was used
        observed['between'] += 1
        observed['accept'] = max(observed['accept'], miss / d if d > 0 else np.inf)
    Pd = dist_p(b, na)
    if na == npb:
      assert nxt[b] == ptok[b, na], (t, 'the bonus token is the target sampler\'s')
    else:
      res, Cr = LR.residual(Pd, int(tok[b, na]))
      Rr = Cr[-1]
      i = int(nxt[b])
      lo, hi = Cr[i] - res[i], Cr[i]
      uR = float(R.clamp_u(np.float32(ures[b]))) * Rr
      miss = max(lo - uR, uR - hi)
      if miss > 4 * delta or not res[i] > 0:
        assert i == ptok[b, na] and Rr <= 4 * delta, (t, 'residual draw', i, miss, delta, Rr, int(ptok[b, na]))
        observed['fallbacks'] += 1
      else:
        assert i != int(tok[b, na]), (t, 'the rejected token is never drawn')
        observed['resid_draws'] += 1
        observed['residual'] = max(observed['residual'], miss / delta)
    ref = Pd.logp[int(nxt[b])]
    if np.isnan(ref):
      assert np.isnan(logp[b, na]), (t, logp[b, na])
    else:
      assert abs(float(logp[b, na]) - ref) <= LOGP_TOL, (t, logp[b, na], ref)
      observed['logp'] = max(observed['logp'], abs(float(logp[b, na]) - ref))
    assert (logp[b, na + 1:].view(np.uint32) == 0).all(), (t, 'entries beyond n_accept are 0')
    if c['kinds'][b] == 'bad_tok':
      assert na <= k // 2, (t, 'a token outside [0, V) is never accepted')


def run_case(ops, c, taus=TAUS):
  V, B, k = c['V'], c['B'], c['k']
  rng = np.random.default_rng(V + 7 * B + k)
  drafted = inside = 0
  for tau in taus:
    for top_k, top_p in FILTERS:
      tag = (V, B, k, tau, top_k, top_p)
      inp = prepare(ops, c, tau, top_k, top_p, rng)
      tok, pcut, n_prop = inp['tok'].cpu().numpy(), inp['pcut'].cpu().numpy().reshape(B, k + 1), c['n_prop']
      memo = {}

      def dist_p(b, r):
        if (b, r) not in memo:
          memo[b, r] = S.Dist(c['xp'][b, r], tau, pcut[b, r])
        return memo[b, r]
      special = rng.uniform(0, 1, (k, B))
      sp = np.array([0.0, R.U_MAX, -1.0, 1.0, 2.0, np.nan, 0.5])
      for j in range(0, k * B, 3):   # every third entry is one of the values the clamp is there for
        special[j // B, j % B] = sp[(j // 3) % len(sp)]
      for ua, ures in ((rng.uniform(0, 1, (k, B)), rng.uniform(0, 1, B)), (special, np.resize(np.array([0.0, R.U_MAX, np.nan, 3.0]), B)),
                       (rng.uniform(0, 1, (k, B)) ** 4, rng.uniform(0, 1, B))):
        ua, n, m = uniforms_outside_the_band(c, dist_p, tok, n_prop, ua, rng)
        drafted += n
        inside += m
        check(c, inp, ua, ures, tau, launch(ops, c, inp, ua, ures, tau), tag, dist_p)
  observed['drafted'] += drafted
  observed['in_band'] += inside
  assert inside <= BAND_SHARE * max(drafted, 1), (V, B, k, 'rows inside the band for the reference alone', inside, drafted)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('B', BS)
@pytest.mark.parametrize('V', VS)
def test_spec_verify_lookup_vs_fp64_reference(ops, V, B, k):
  run_case(ops, case(V, B, k))
  o = observed
  print(f'spec_verify_lookup V={V} B={B} k={k}: so far {o["rows"]} rows judged ({o["accepted"]} accepted), {o["between"]} on the band\'s side of '
        f'alpha using at most {o["accept"]:.2e} of d; {o["in_band"]} of {o["drafted"]} drafted rows ({o["in_band"] / max(o["drafted"], 1):.4f}) '
        f'inside the band for the reference alone (allowed {BAND_SHARE}); {o["resid_draws"]} residual draws missing by at most '
        f'{o["residual"]:.2e} of delta, {o["fallbacks"]} fallbacks; |logp - fp64| {o["logp"]:.2e} (allowed {LOGP_TOL:.0e})')


def test_spec_verify_lookup_padded_rows_with_nan_in_the_pad(ops):
  run_case(ops, case(1000, 5, 4, padded=1), taus=(0.8,))
  run_case(ops, case(257, 5, 8, padded=1), taus=(0.8,))


@pytest.mark.parametrize('V,B,k', [(1000, 5, 4), (50280, 5, 8)])
def test_lookup_verify_is_exact_where_it_must_be(ops, V, B, k):
  """Two runs bit-equal; rows at and beyond n_prop[b] are never loaded; n_prop is clamped; sequences do not see each other."""
  c = case(V, B, k)
  rng = np.random.default_rng(3)
  for tau, (top_k, top_p) in ((0.8, FILTERS[0]), (0.8, FILTERS[1]), (50.0, FILTERS[0])):
    inp = prepare(ops, c, tau, top_k, top_p, rng)
    ua, ures = rng.uniform(0, 1, (k, B)) ** 2, rng.uniform(0, 1, B)
    a = launch(ops, c, inp, ua, ures, tau)
    assert same_bits(a, launch(ops, c, inp, ua, ures, tau)), (tau, top_k)
    n_prop = c['n_prop']
    assert (a[0] <= n_prop).all()
    # what lies at and beyond n_prop[b]: NaN logits, a NaN cutoff, wild tokens and uniforms - the outputs keep their bits
    c2 = dict(c, dp=c['dp'].clone())
    inp2 = {n: t.clone() for n, t in inp.items()}
    ua2 = ua.copy()
    for b in range(B):
      c2['dp'].view(B, k + 1, -1)[b, n_prop[b] + 1:] = float('nan')
      inp2['pcut'].view(B, k + 1)[b, n_prop[b] + 1:] = float('nan')
      inp2['ptok'].view(B, k + 1)[b, n_prop[b] + 1:] = -(1 << 50)
      inp2['tok'][b, n_prop[b]:] = (1 << 50) + b
      ua2[n_prop[b]:, b] = np.nan
    assert same_bits(a, launch(ops, c2, inp2, ua2, ures, tau)), (tau, top_k, 'rows beyond n_prop were read')
    # out-of-range n_prop is clamped on the device
    inp3 = dict(inp, n_prop=torch.where(inp['n_prop'] == k, inp['n_prop'] + 7, torch.where(inp['n_prop'] == 0, inp['n_prop'] - 5, inp['n_prop'])))
    assert same_bits(a, launch(ops, c, inp3, ua, ures, tau)), (tau, top_k, 'clamp')
    # sequence 2 gets other inputs throughout: the other sequences' outputs keep their bits
    c4 = dict(c, dp=c['dp'].clone())
    c4['dp'].view(B, k + 1, -1)[2] = c['dp'].view(B, k + 1, -1)[0]
    inp4 = {n: t.clone() for n, t in inp.items()}
    inp4['tok'][2] = inp['tok'][1]
    inp4['n_prop'][2] = k - int(inp['n_prop'][2])
    inp4['pcut'].view(B, k + 1)[2] = inp['pcut'].view(B, k + 1)[0]
    inp4['ptok'].view(B, k + 1)[2] = inp['ptok'].view(B, k + 1)[0]
    ua4, ures4 = ua.copy(), ures.copy()
    ua4[:, 2], ures4[2] = 0.123, 0.987
    other = launch(ops, c4, inp4, ua4, ures4, tau)
    keep = [b for b in range(B) if b != 2]
    assert same_bits(tuple(t[keep] for t in a), tuple(t[keep] for t in other)), (tau, top_k)


def test_spec_verify_lookup_refuses_what_the_wrapper_can_see(ops):
  B, k, V = 2, 2, 64
  z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')  # noqa: E731
  good = dict(tl=z(B * (k + 1), V, dt=BF16), tok=z(B, k, dt=I64), np=torch.full((B,), k, dtype=I32, device='cuda'), pc=z(B * (k + 1)),
              pt=z(B * (k + 1), dt=I64), ua=z(k, B), ur=z(B))
  call = lambda **kw: ops.spec_verify_lookup(*{**good, **kw}.values())  # noqa: E731
  r = call()
  assert isinstance(r, ops.SpecVerify) and r.n_accept.tolist() == [2, 2]  # equal logits: p(0) = 1 / 64 > u = 0
  assert call(np=z(B, dt=I32)).n_accept.tolist() == [0, 0]
  with pytest.raises(ValueError, match='target_logits'):
    call(tl=z(B * k, V, dt=BF16))
  with pytest.raises(ValueError, match='unit inner stride'):
    call(tl=z(V, B * (k + 1), dt=BF16).t())
  with pytest.raises(TypeError):
    call(tok=z(B, k, dt=I32))
  with pytest.raises(TypeError):
    call(np=z(B, dt=I64))
  with pytest.raises(ValueError, match='u_resid'):
    call(ur=z(B + 1))
  with pytest.raises(RuntimeError, match='temperature'):
    ops.spec_verify_lookup(*good.values(), temperature=0.0)
  with pytest.raises(RuntimeError, match='drafted tokens'):
    ops.spec_verify_lookup(z(33 * 2, V, dt=BF16), z(2, 32, dt=I64), z(2, dt=I32), z(66), z(66, dt=I64), z(32, 2), z(2))


# ================================================================================================================================================
# generate_lookup on the 2-layer golden model
# ================================================================================================================================================
@pytest.fixture(scope='module')
def mdl(golden_dir):
  z = np.load(os.path.join(golden_dir, 'model.npz'))
  return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.fixture(scope='module')
def model(ops, mdl):
  import plainlm_amd as P
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  m.load_state_dict({k[2:]: v for k, v in mdl.items() if k.startswith('w:')})
  return m.cuda()


T0, N, K = 16, 32, 4


def _against_the_full_forward(m, prompt, toks, lps, lens=None):
  """generate's criteria (tests/test_decode_gpu.py, as tests/test_spec_gpu.py applies them): every token's logit is within 4 eps of its
  row's maximum in the full forward, the log-probabilities are predict's within eps.  Returns (gap, eps)."""
  B = prompt.shape[0]
  lens = [T0] * B if lens is None else lens
  worst, eps = 0.0, None
  for b in range(B):
    seq = torch.cat([prompt[b:b + 1, :lens[b]], toks[b:b + 1]], dim=1)
    full = m(torch.nn.functional.pad(seq, (0, (-seq.shape[1]) % 4)), None).float()[:, :seq.shape[1]]
    eps = 2e-2 * full.abs().max().item()
    rows = full[:, lens[b] - 1:lens[b] - 1 + N]
    chosen = rows.gather(2, toks[b:b + 1, :, None])[:, :, 0]
    worst = max(worst, (rows.max(dim=-1).values - chosen).max().item())
    assert worst <= 4 * eps, (b, worst, eps)
    tg = torch.full((1, full.shape[1] + (-seq.shape[1]) % 4), -100, dtype=torch.int64, device=seq.device)
    tg[:, lens[b] - 1:lens[b] - 1 + N] = toks[b:b + 1]
    want = -m.predict(torch.nn.functional.pad(seq, (0, (-seq.shape[1]) % 4)), targets=tg).nll[:, lens[b] - 1:lens[b] - 1 + N]
    assert (lps[b:b + 1] - want).abs().max().item() <= eps, (b, (lps[b:b + 1] - want).abs().max().item(), eps)
  assert (lps <= 0).all()
  return worst, eps


def test_greedy_lookup_meets_generate_s_criteria_twice_and_rolls_back(model, mdl, monkeypatch):
  m = model
  prompt = mdl['tokens'][:, :T0].cuda()
  caches = []
  real = m.prefill
  monkeypatch.setattr(m, 'prefill', lambda *a, **k: caches.append(real(*a, **k)) or caches[-1])
  with torch.no_grad():
    toks, lps, stats = m.generate_lookup(prompt, N, n_draft=K, return_logprobs=True, return_stats=True)
    monkeypatch.undo()
    assert toks.dtype == torch.int64 and tuple(toks.shape) == (2, N) and lps.dtype == torch.float32 and tuple(lps.shape) == (2, N)
    gap, eps = _against_the_full_forward(m, prompt, toks, lps)
    d, a, rounds = stats['drafted'], stats['accepted'], stats['rounds']
    plain = m.generate(prompt, N)
    print(f'greedy lookup, k = {K}, ngram (1, 4): {rounds} rounds for {N} tokens, {a.sum().item()} of {d.sum().item()} proposals accepted; worst '
          f'(row max - chosen logit) {gap:.3e} against 4 eps = {4 * eps:.3e}; tokens equal to generate()\'s: {(plain == toks).float().mean().item():.4f}')
    assert d.dtype == torch.int64 and ((a <= d) & (d <= K * rounds)).all() and (d % K == 0).all() and 1 <= rounds <= N - 1
    # two calls are bit-equal; the plain result forms are generate's
    t2, l2 = m.generate_lookup(prompt, N, n_draft=K, return_logprobs=True)
    assert torch.equal(t2, toks) and torch.equal(l2.view(torch.int32), lps.view(torch.int32))
    assert torch.equal(m.generate_lookup(prompt, N, n_draft=K), toks)
    # the rollback: the cache holds the prompt and every generated token but the newest, with the bits of a fresh prefill
    cache = caches[0][0]
    cache.check()
    assert cache.lens.tolist() == [T0 + N - 1] * 2
    fresh, _ = m.prefill(torch.cat([prompt, toks], dim=1)[:, :T0 + N - 1].contiguous())
    for layer in range(len(cache.kv)):
      for b in range(2):
        n = T0 + N - 1
        assert torch.equal(cache.kv[layer][b, :n].view(torch.int16), fresh.kv[layer][b, :n].view(torch.int16)), (layer, b)


def test_lookup_ragged_prompts_and_eos(model, mdl):
  m = model
  prompt = mdl['tokens'][:, :T0].cuda()
  with torch.no_grad():
    for ngram in ((1, 4), (1, 1)):
      toks, lps = m.generate_lookup(prompt, N, n_draft=K, ngram=ngram, return_logprobs=True)
      lens = (16, 9)
      rt, rl = m.generate_lookup(prompt, N, n_draft=K, ngram=ngram, prompt_lens=lens, return_logprobs=True)
      assert torch.equal(rt[0], toks[0]) and torch.equal(rl[0].view(torch.int32), lps[0].view(torch.int32))  # sequence 0 does not see sequence 1
      _against_the_full_forward(m, prompt, rt, rl, lens)
      eos = int(toks[0, 5].item())
      te, le, stats = m.generate_lookup(prompt, N, n_draft=K, ngram=ngram, eos_id=eos, return_logprobs=True, return_stats=True)
      froze = 0
      for b in range(2):
        hit = (toks[b] == eos).nonzero()
        n = int(hit[0]) + 1 if len(hit) else N
        froze += N - n
        assert torch.equal(te[b, :n], toks[b, :n]) and torch.equal(le[b, :n].view(torch.int32), lps[b, :n].view(torch.int32)), b
        assert (te[b, n:] == eos).all() and (le[b, n:] == 0).all(), b
      assert froze > 0 and (stats['accepted'] <= stats['drafted']).all() and (stats['drafted'] <= K * stats['rounds']).all()


def test_sampled_lookup_is_reproducible_in_the_top_5_and_scores_as_predict(model, mdl):
  m = model
  prompt = mdl['tokens'][:, :T0].cuda()
  kw = dict(n_draft=K, temperature=0.8, top_k=5, return_logprobs=True)
  with torch.no_grad():
    for ngram in ((1, 4), (1, 1)):
      toks, lps, stats = m.generate_lookup(prompt, N, ngram=ngram, seed=21, return_stats=True, **kw)
      t2, l2 = m.generate_lookup(prompt, N, ngram=ngram, seed=21, **kw)
      assert torch.equal(t2, toks) and torch.equal(l2.view(torch.int32), lps.view(torch.int32))
      t3, _ = m.generate_lookup(prompt, N, ngram=ngram, seed=22, **kw)
      assert not torch.equal(t3, toks)
      seq = torch.cat([prompt, toks], dim=1)
      rows = m(seq, None).float()[:, T0 - 1:T0 - 1 + N]
      chosen = rows.gather(2, toks[:, :, None])[:, :, 0]
      gap = (rows.topk(5, dim=-1).values[..., 4] - chosen).max().item()
      want = torch.log_softmax(rows.double(), dim=-1).gather(2, toks[:, :, None])[:, :, 0]
      err = (lps.double() - want).abs().max().item()
      d, a, rounds = stats['drafted'], stats['accepted'], stats['rounds']
      print(f'sampled lookup (0.8 / top-5), ngram {ngram}: {rounds} rounds, {a.sum().item()} of {d.sum().item()} proposals accepted; worst (5th '
            f'largest full-forward logit - chosen) {gap:.3e} (allowed {LOGIT_TOL}); |logp - log softmax(full forward)| {err:.3e} (allowed '
            f'{LOGP_MODEL_TOL})')
      assert ((toks >= 0) & (toks < 256)).all() and gap <= LOGIT_TOL and err <= LOGP_MODEL_TOL and (lps <= 0).all()
      assert ((a <= d) & (d <= K * rounds)).all()


def test_a_repeated_block_is_proposed_in_round_0(model, mdl):
  """A prompt that is one 4-token block repeated: when the first generated token is one of the block's, round 0 finds it in the prompt
  and proposes k tokens - asserted through the statistics of a call with exactly one round, not through acceptance.  The block is
  searched among 256 candidates in one batch (the model decides its first token, the test only picks a block that contains it)."""
  m = model
  base = mdl['tokens'][0, :3].tolist()
  cand = torch.tensor([(base + [t]) * 4 for t in range(256)], dtype=torch.int64).cuda()
  with torch.no_grad():
    first = m.generate(cand, 1)[:, 0].cpu()
    inside = [t for t in range(256) if int(first[t]) in base + [t]]
    assert inside, 'no candidate block contains its own first generated token'
    rows = cand[inside[:2] + [t for t in range(256) if t not in inside][:1]]   # the last row is a block that lacks its first token, if any
    hit = len(inside[:2])
    toks, stats = m.generate_lookup(rows, 2, n_draft=K, ngram=(1, 4), return_stats=True)
    assert stats['rounds'] == 1 and stats['drafted'][:hit].tolist() == [K] * hit, stats
    assert torch.equal(toks[:, 0].cpu(), first[inside[:2] + [t for t in range(256) if t not in inside][:1]])
    if rows.shape[0] > hit:
      assert stats['drafted'][hit].item() == 0   # its first token occurs nowhere in the prompt
    assert (stats['accepted'] <= stats['drafted']).all()


def test_generate_lookup_refusals_on_the_device(model, mdl):
  m = model
  prompt = mdl['tokens'][:, :T0].cuda()
  with torch.no_grad():
    with pytest.raises(ValueError, match='n_draft'):
      m.generate_lookup(prompt, 8, n_draft=32)
    with pytest.raises(ValueError, match='ngram'):
      m.generate_lookup(prompt, 8, ngram=(3, 2))
    with pytest.raises(ValueError, match='seq_len'):
      m.generate_lookup(prompt, 44, n_draft=4)  # 16 + 44 + 4 + 1 > 64
    with pytest.raises(ValueError, match='top_p'):
      m.generate_lookup(prompt, 8, temperature=0.8, top_p=0.0)
    with pytest.raises(TypeError, match='int64'):
      m.generate_lookup(prompt.int(), 8)
  with pytest.raises(RuntimeError, match='forward-only'):
    m.generate_lookup(prompt, 8)
