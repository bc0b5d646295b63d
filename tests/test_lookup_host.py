"""CPU tests (no GPU) of draft-free speculative decoding: the draft rule of tests/lookup_ref.py against a brute-force
"longest suffix match, most recent" search; the one-hot acceptance rule leaves the target's distribution exact; generate._LookupSession
under generate.speculative_loop with a fake model, a fake cache and the reference as the draft kernel emits what generate.generate_loop
emits, keeps the cache and the history in step, and accepts everything on periodic text; the refusals of check_lookup and of the two
entry points (before any HIP call)."""

import ctypes as C
import inspect
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib, ops
from plainlm_amd import generate as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import lookup_ref as LR  # noqa: E402
import sample_ref as R  # noqa: E402
import spec_ref as S  # noqa: E402


# ---- (a) the draft rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alphabet', [2, 3, 4])
def test_draft_rule_is_the_longest_most_recent_suffix_match(alphabet):
  rng = np.random.default_rng(alphabet)
  hits = 0
  for trial in range(300):
    L = int(rng.integers(0, 40))
    h = rng.integers(0, alphabet, L + 5)
    k = int(rng.choice([1, 4, 31]))
    g_max = int(rng.choice([1, 2, 4, 16]))
    g_min = int(rng.integers(1, g_max + 1))
    got, want = LR.draft(h, L, k, g_min, g_max), LR.draft_brute(h, L, k, g_min, g_max)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (h[:L].tolist(), k, g_min, g_max, got, want)
    assert got[1] in (0, k) and (got[1] == 0) == (got[2] == 0) and (got[2] == 0 or g_min <= got[2] <= g_max)
    hits += got[1] > 0
  assert hits > 100


def test_draft_rule_on_hand_written_histories():
  d = lambda h, k, g=(1, 4): LR.draft(np.array(h), len(h), k, *g)  # noqa: E731
  assert d([], 3)[1:] == (0, 0) and d([5], 3)[1:] == (0, 0) and d([5, 6], 3)[1:] == (0, 0)   # L < 2, and no earlier occurrence
  assert d([5, 6], 3)[0].tolist() == [0, 0, 0]
  # period 1: a winner at e = L - 1 repeats the last token; the match is capped at min(g_max, e)
  t, n, m = d([7, 7], 4)
  assert t.tolist() == [7, 7, 7, 7] and (n, m) == (4, 1)
  t, n, m = d([7] * 9, 4)
  assert t.tolist() == [7] * 4 and (n, m) == (4, 4)
  # period 2 and period k - 1: the overlapped copy wraps
  t, n, m = d([1, 2, 1, 2, 1], 5)
  assert t.tolist() == [2, 1, 2, 1, 2] and (n, m) == (5, 3)
  k = 6
  t, n, m = d([9, 1, 2, 3, 4, 5, 1], k)   # the winner is e = 2 (after the first 1): period 5 = k - 1
  assert t.tolist() == [2, 3, 4, 5, 1, 2] and (n, m) == (k, 1)
  # the longest match beats a more recent shorter one; among equal lengths the most recent wins
  t, n, m = d([1, 2, 8, 3, 2, 9, 1, 2], 2)
  assert t.tolist() == [8, 3] and m == 2
  t, n, m = d([1, 2, 8, 1, 2, 9, 1, 2], 2)
  assert t.tolist() == [9, 1] and m == 2
  # a winner at e = 1
  t, n, m = d([4, 5, 6, 4], 3)
  assert t.tolist() == [5, 6, 4] and m == 1
  # g_min = 2: a one-token match is no candidate
  assert d([4, 5, 6, 4], 3, (2, 4))[1:] == (0, 0)


def test_reference_launch_appends_refuses_and_leaves_the_rest_alone():
  hist = np.full((3, 8), -7, dtype=np.int64)
  hist[0, :4] = [1, 2, 1, 2]
  hist[1, :7] = [3, 3, 3, 3, 3, 3, 3]
  hist[2, :2] = [5, 6]
  add = np.array([[1, 9], [3, 3], [5, 9]])
  r = LR.lookup(hist, [4, 7, 2], add, np.array([1, 2, 5], dtype=np.int32), 3, (1, 4))
  assert r['status'] == 1 and r['lens'].tolist() == [5, 7, 4]                       # sequence 1 does not fit: 7 + 2 > 8
  assert r['hist'][0].tolist() == [1, 2, 1, 2, 1, -7, -7, -7] and r['hist'][1].tolist() == [3] * 7 + [-7]
  assert r['hist'][2].tolist() == [5, 6, 5, 9, -7, -7, -7, -7]                     # n_add is clamped to the width of add_tok
  assert r['draft'].tolist() == [[2, 1, 2], [0, 0, 0], [0, 0, 0]] and r['n_prop'].tolist() == [3, 0, 0] and r['match_len'].tolist() == [3, 0, 0]
  assert hist[0, 4] == -7                                                            # the inputs are not modified


# ---- (b) the one-hot rule is exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('V', [5, 8])
@pytest.mark.parametrize('tau', [0.5, 1.0, 3.0])
def test_the_first_emitted_token_is_distributed_as_the_target(V, tau):
  rng = np.random.default_rng(V)
  x = rng.normal(0, 2, V)
  rows = [('random', x), ('ties', np.round(x)), ('p one-hot', np.where(np.arange(V) == 2, 0.0, -np.inf)),
          ('nonfinite', np.where(np.arange(V) % 3 == 0, np.nan, x))]
  seen_unkept = seen_all_on_x = 0
  for name, xp in rows:
    for top_k, top_p in ((0, 1.0), (3, 1.0), (0, 0.8)):
      cp = R.Rows(xp[None]).keep_set(tau, top_k, top_p)['cutoff'][0]
      Pd = S.Dist(xp, tau, cp)
      for tok in range(-1, V + 1):
        got = LR.first_token_distribution(Pd, tok)
        assert np.abs(got - Pd.prob).max() <= 1e-12, (name, top_k, top_p, tok, got, Pd.prob)
        assert abs(got.sum() - 1.0) <= 1e-12
        if 0 <= tok < V:
          seen_unkept += not Pd.keep[tok]
          seen_all_on_x += Pd.prob[tok] == 1.0
          assert LR.alpha(Pd, tok) == Pd.prob[tok] and (Pd.keep[tok] or LR.alpha(Pd, tok) == 0.0)
        else:
          assert LR.alpha(Pd, tok) == 0.0
  assert seen_unkept > 0 and seen_all_on_x > 0   # a drafted token outside the kept set, and a row where p sits entirely on x


def test_reference_verify_on_hand_written_rows():
  ln = np.log
  p = S.Dist(ln([0.5, 0.25, 0.25, 1e-300]), 1.0, -np.inf)
  assert abs(LR.alpha(p, 1) - 0.25) < 1e-15 and LR.alpha(p, -1) == 0.0 and LR.alpha(p, 4) == 0.0
  r, Cr = LR.residual(p, 0)
  assert np.allclose(r, [0, 0.25, 0.25, 0]) and LR.draw(Cr, 0.4) == 1 and LR.draw(Cr, 0.6) == 2
  # u = 0.3 >= alpha = 0.25: rejected at row 0; the residual is p without column 1: 0.5 | 0.25 of 0.75
  n, nxt, lp = LR.verify([p, p, p], [1, 0], 2, [2, 3, 0], [0.3, 0.0], 0.7)
  assert (n, nxt) == (0, 2) and abs(lp[0] - ln(0.25)) < 1e-12 and lp[1] == 0 and lp[2] == 0
  # accepted twice: the bonus token is the sampler's token of row 2
  n, nxt, lp = LR.verify([p, p, p], [1, 0], 2, [2, 3, 0], [0.2, 0.4], 0.7)
  assert (n, nxt) == (2, 0) and abs(lp[0] - ln(0.25)) < 1e-12 and abs(lp[1] - ln(0.5)) < 1e-12 and abs(lp[2] - ln(0.5)) < 1e-12
  # n_prop = 0: the plain next token, whatever the proposal row holds; n_prop = 1: row 1 is not looked at
  assert LR.verify([p, p, p], [1, 0], 0, [2, 3, 0], [0.0, 0.0], 0.7)[:2] == (0, 2)
  assert LR.verify([p, p, p], [1, 0], 1, [2, 3, 0], [0.0, 0.0], 0.7)[:2] == (1, 3)
  assert LR.verify([p, p, p], [1, 0], 9, [2, 3, 0], [0.0, 0.0], 0.7)[0] == 2     # clamped to k
  # p entirely on x: always accepted (u < 1); were it rejected, R = 0 falls back to the sampler's token
  one = S.Dist(ln([1e-300, 1.0, 1e-300, 1e-300]), 1.0, 0.0)
  assert LR.alpha(one, 1) == 1.0 and LR.draw(LR.residual(one, 1)[1], 0.5) is None
  # a token outside the kept set: rejected even at u = 0, the residual is p itself
  pk = S.Dist(ln([0.5, 0.25, 0.25, 1e-3]), 1.0, ln(0.25))
  n, nxt, _ = LR.verify([pk, pk], [3], 1, [2, 2], [0.0], 0.6)
  assert (n, nxt) == (0, 1)
  # no finite logit: nothing kept, the fallback, logp NaN
  e = S.Dist(np.full(4, np.nan), 1.0, np.nan)
  n, nxt, lp = LR.verify([e, e], [0], 1, [3, 0], [0.0], 0.5)
  assert (n, nxt) == (0, 3) and np.isnan(lp[0])


# ---- (c) the session under speculative_loop, with fakes -------------------------------------------------------------------------------------
VOC = 5
Pred = namedtuple('Pred', ['tokens', 'logprob'])


def lm_drift(ctx):
  """A toy model over 5 symbols: mostly a function of the last two tokens (so its text repeats and lookups hit), drifting every 7
  positions (so proposals get rejected)."""
  a, b = ctx[-1], (ctx[-2] if len(ctx) > 1 else 0)
  t = (2 * a + 3 * b + 1 + len(ctx) // 7) % VOC
  return t, -float((t * 37 + len(ctx)) % 101) / 64.0 - 0.015625


def lm_periodic(period):
  def lm(ctx):
    t = ctx[-period]
    return t, -float((t * 37 + len(ctx)) % 101) / 64.0 - 0.015625
  return lm


class FakeCache:
  def __init__(self, prompts):
    self.B = len(prompts)
    self.rows = [list(p) for p in prompts]
    self.lens = torch.tensor([len(p) for p in prompts], dtype=torch.int32)

  def set_lens(self, lens):
    self.lens = lens.clone()


class FakeModel:
  """extend() as Transformer.extend(all_rows=True) behaves: rows at and beyond token_lens[b] are padding and predict token 0 with a NaN
  log-probability - a zero-filled proposal row would "match" them if the session did not mask it."""

  def __init__(self, lm):
    self.lm = lm

  def extend(self, chunk, cache, token_lens=None, logits=False, all_rows=False):
    assert all_rows and not logits and token_lens.dtype == torch.int32
    B, n = chunk.shape
    toks, lps = torch.zeros((B, n), dtype=torch.int64), torch.full((B, n), float('nan'))
    for b in range(B):
      c, L = int(token_lens[b]), int(cache.lens[b])
      assert 0 <= c <= n
      cache.rows[b] = cache.rows[b][:L] + chunk[b, :c].tolist()   # rows beyond lens are overwritten: the rollback
      for r in range(c):
        toks[b, r], lps[b, r] = self.lm(cache.rows[b][:L + r + 1])
    cache.lens = cache.lens + token_lens
    return Pred(toks, lps)


def fake_lookup(hist, lens, add_tok=None, n_add=None, k=8, ngram=(1, 4), status=None):
  """ops.lookup_draft on CPU tensors, through the reference."""
  r = LR.lookup(hist.numpy(), lens.numpy(), None if add_tok is None else add_tok.numpy(), None if n_add is None else n_add.numpy(), k, ngram)
  hist.copy_(torch.from_numpy(r['hist']))
  lens.copy_(torch.from_numpy(r['lens']))
  if r['status']:
    status.fill_(1)
  return ops.LookupDraft(torch.from_numpy(r['draft']), torch.from_numpy(r['n_prop']), torch.from_numpy(r['match_len']))


PROMPTS = [[3, 1, 4, 1, 0], [2, 2, 1], [0, 3, 0, 3, 2, 1], [2, 4]]


def _padded(prompts):
  T = max(len(p) for p in prompts)
  return torch.tensor([p + [0] * (T - len(p)) for p in prompts], dtype=torch.int64)


def _first(lm, prompts):
  r = [lm(p) for p in prompts]
  return torch.tensor([t for t, _ in r]), torch.tensor([lp for _, lp in r], dtype=torch.float32)


def _reference(lm, prompts, N, eos_id=None):
  rows = [list(p) for p in prompts]

  def step(tok):
    out = []
    for b, t in enumerate(tok.tolist()):
      rows[b].append(t)
      out.append(lm(rows[b]))
    return torch.tensor([t for t, _ in out]), torch.tensor([lp for _, lp in out], dtype=torch.float32)
  return G.generate_loop(_first(lm, prompts), step, N, eos_id, check_every=1)


class Run:
  """One fake generate_lookup call; ``advance`` is wrapped to look at the state after every round."""

  def __init__(self, lm, prompts, N, k, ngram, eos_id=None):
    self.prompts, self.k = prompts, k
    self.cache = FakeCache(prompts)
    first = _first(lm, prompts)
    self.s = G._LookupSession(FakeModel(lm), self.cache, _padded(prompts), first[0], k, ngram, N, None, None, lookup=fake_lookup)
    self.rounds = []       # per round: (n_prop, n_accept, moved, live, history lengths at the draft)
    self.reads = 0
    self.toks, self.lps, self.stats = G.speculative_loop(first, self.s.draft_round, self.s.target_round, self.s.accept, N, k, eos_id,
                                                         self.advance, all_done=self.all_done, drafted_in_round=self.s.drafted)
    self.s.check()

  def all_done(self, done):
    self.reads += 1
    return bool(done.all())

  def advance(self, moved, live):
    s = self.s
    self.rounds.append((s.n_prop.tolist(), s.n_accept.tolist(), moved.tolist(), live.tolist(), s.hlen.tolist()))
    s.advance(moved, live)
    for b, p in enumerate(self.prompts):
      # the cache holds the sequence up to, not including, its newest token; the history and what the next launch appends hold all of it
      seq = s.hist[b, :int(s.hlen[b])].tolist() + s.add[b, :int(s.n_add[b])].tolist()
      assert seq[:len(p)] == p and int(self.cache.lens[b]) == len(seq) - 1, (b, seq)
      assert self.cache.rows[b][:len(seq) - 1] == seq[:-1], (b, 'the cache went out of step')


@pytest.mark.parametrize('ngram', [(1, 1), (2, 4)])
@pytest.mark.parametrize('k', [1, 4, 8])
def test_greedy_lookup_emits_what_generate_loop_emits(k, ngram):
  N = 30   # N - 1 = 29 is no multiple of k + 1 for k in 1, 4, 8 ... (2, 5, 9): 29 is prime
  want_t, want_l = _reference(lm_drift, PROMPTS, N)
  for eos in (None, int(want_t[0, 6]), int(want_t[2, 0]), int(want_t[1, N - 1])):
    wt, wl = (want_t, want_l) if eos is None else _reference(lm_drift, PROMPTS, N, eos)
    run = Run(lm_drift, PROMPTS, N, k, ngram, eos)
    assert torch.equal(run.toks, wt), (eos, run.toks, wt)
    assert torch.equal(run.lps, wl) and not torch.isnan(run.lps).any(), eos
    st = run.stats
    assert st['rounds'] == len(run.rounds) <= N - 1 and run.reads <= st['rounds'] + 1   # one read per round (and the one that ends the loop)
    drafted = [sum(r[0][b] for r in run.rounds if r[3][b]) for b in range(4)]
    accepted = [sum(r[1][b] for r in run.rounds if r[3][b]) for b in range(4)]
    assert st['drafted'].tolist() == drafted and st['accepted'].tolist() == accepted
    assert all(a <= d <= k * st['rounds'] for a, d in zip(accepted, drafted))
    for n_prop, n_acc, moved, live, _ in run.rounds:
      assert all(p in (0, k) and a <= p for p, a in zip(n_prop, n_acc))   # a zero-filled row never counts as a match
      assert all(m == 0 for m, lv in zip(moved, live) if not lv)
    if eos is None:
      assert sum(drafted) > 0 and 0 < sum(accepted) < sum(drafted)         # it hits, accepts and rejects
      assert any(p == 0 for r in run.rounds for p, lv in zip(r[0], r[3]) if lv) or ngram == (1, 1)


@pytest.mark.parametrize('period', [1, 2, 5])
@pytest.mark.parametrize('k', [1, 4, 8])
def test_periodic_text_is_accepted_in_full_after_the_first_period(period, k):
  """The acceptance guarantee no GPU test with random weights can give: once the history holds the period twice, the longest match
  continues it, all k proposals are accepted and a round yields k + 1 tokens."""
  block = [3, 1, 4, 1, 0][:period]
  prompts = [block, [2] + block, block * 2]
  N = 41
  lm = lm_periodic(period)
  want_t, want_l = _reference(lm, prompts, N)
  run = Run(lm, prompts, N, k, (1, 4))
  assert torch.equal(run.toks, want_t) and torch.equal(run.lps, want_l)
  full = 0
  count = [1, 1, 1]
  for n_prop, n_acc, moved, live, hlen in run.rounds:
    for b in range(3):
      if live[b] and hlen[b] >= 2 * period + 1:   # hlen: the history at the draft, the newest token included
        assert n_prop[b] == k and n_acc[b] == k and moved[b] == min(k + 1, N - count[b]), (b, n_prop, n_acc, moved, hlen)
        full += 1
      count[b] += moved[b]
  assert full >= 3 and count == [N] * 3
  assert run.stats['rounds'] <= 2 * period + 2 + -(-(N - 1) // (k + 1))
  # drafted counts the proposals made in the rounds a sequence was live in, not k per round
  assert run.stats['drafted'].tolist() == [sum(r[0][b] for r in run.rounds if r[3][b]) for b in range(3)]
  assert run.stats['accepted'].tolist() == [sum(r[1][b] for r in run.rounds if r[3][b]) for b in range(3)]
  assert (run.stats['accepted'] <= run.stats['drafted']).all() and (run.stats['drafted'] <= k * run.stats['rounds']).all()


def test_lookup_uniforms_are_drawn_once_and_no_entry_is_used_twice():
  N, k, B = 7, 3, 2
  u = G.lookup_uniforms(N, k, B, 'cpu', seed=9)
  assert G.lookup_uniforms_per_round(k) == 2 * k + 2
  assert tuple(u.shape) == (1 + (N - 1) * (2 * k + 2), B) and torch.equal(u, G.draw_uniforms(u.shape[0], B, 'cpu', seed=9))
  mark = torch.arange(u.numel(), dtype=torch.float32).view_as(u)
  seen = [mark[0]]
  for i in range(N - 1):
    ut, ua, ur = G.lookup_round_uniforms(mark, i, k)
    assert tuple(ut.shape) == (k + 1, B) and tuple(ua.shape) == (k, B) and tuple(ur.shape) == (B,)
    assert ua.is_contiguous() and ur.is_contiguous()
    seen += [ut.reshape(-1), ua.reshape(-1), ur]
  allv = torch.cat([s.reshape(-1) for s in seen])
  assert allv.numel() == u.numel() and allv.unique().numel() == u.numel()


def test_sampled_session_hands_the_verifier_the_round_s_rows():
  """The sampled path with stand-ins for the two kernels: the sampler sees the k + 1 chunk rows of every sequence with the round's
  uniforms in row order b * (k + 1) + r, the verifier gets the proposal, n_prop and the round's acceptance / residual uniforms."""
  B, k, N, V = 2, 3, 5, 4
  u = G.lookup_uniforms(N, k, B, 'cpu', seed=1)
  calls = {}

  class Cache:
    lens = torch.tensor([3, 3], dtype=torch.int32)
  St = namedtuple('St', ['tokens', 'logprob', 'n_kept', 'cutoff'])

  def sampler(rows, uu, t, tk, tp, want_stats=False):
    calls['sampler'] = (tuple(rows.shape), uu.clone(), (t, tk, tp), want_stats)
    return St(torch.arange(rows.shape[0]), None, None, torch.full((rows.shape[0],), 0.5))

  def verify(rows, draft_tok, n_prop, cutoff, tokens, ua, ures, t):
    calls['verify'] = (tuple(rows.shape), draft_tok, n_prop, cutoff, tokens, ua.clone(), ures.clone(), t)
    return ops.SpecVerify(torch.tensor([1, 0], dtype=torch.int32), torch.tensor([2, 3]), torch.zeros(B, k + 1))
  s = G._LookupSession(None, Cache(), torch.tensor([[1, 2, 1], [0, 1, 4]]), torch.tensor([2, 3]), k, (1, 4), N, (0.8, 5, 1.0), u,
                       lookup=fake_lookup, sampler=sampler, verify=verify)
  s.round = 2
  draft, _ = s.draft_round(torch.tensor([2, 3]), None, None, torch.tensor([True, True]))
  assert draft.tolist() == [[1, 2, 1], [0, 0, 0]] and s.n_prop.tolist() == [k, 0]
  res = s.accept(draft, None, torch.zeros(B, k + 1, V, dtype=torch.bfloat16))
  ut, ua, ur = G.lookup_round_uniforms(u, 2, k)
  assert calls['sampler'][0] == (B * (k + 1), V) and torch.equal(calls['sampler'][1], ut.t().reshape(-1)) and calls['sampler'][2:] == ((0.8, 5, 1.0), True)
  v = calls['verify']
  assert v[0] == (B * (k + 1), V) and v[1] is draft and v[2] is s.n_prop and torch.equal(v[5], ua) and torch.equal(v[6], ur) and v[7] == 0.8
  assert res[0].tolist() == [1, 0] and s.drafted() is s.n_prop


# ---- (d) refusals ----------------------------------------------------------------------------------------------------------------------------
Cfg = namedtuple('Cfg', ['vocab_size', 'seq_len'])


def test_check_lookup_refuses_and_normalises():
  cl = G.check_lookup
  cfg = Cfg(512, 128)
  assert cl(16, 32, 8, (1, 4), cfg) == (57, None)
  assert cl(16, 32, 4, [2, 2], cfg, 0.8, 5, None, 3) == (53, (0.8, 5, 1.0))
  assert cl(16, 32, 31, (16, 16), cfg, temperature=0) == (80, None)
  for n in (0, -1, 32, 100):
    with pytest.raises(ValueError, match='n_draft'):
      cl(16, 32, n, (1, 4), cfg)
  for n in (4.0, '4', None, True):
    with pytest.raises(TypeError, match='n_draft'):
      cl(16, 32, n, (1, 4), cfg)
  for g in ((0, 4), (3, 2), (1, 17), (-1, -1)):
    with pytest.raises(ValueError, match='ngram'):
      cl(16, 32, 4, g, cfg)
  for g in (4, (1,), (1, 2, 3), (1.0, 4), (1, None), (True, 4), '14'):
    with pytest.raises(TypeError, match='ngram'):
      cl(16, 32, 4, g, cfg)
  assert cl(16, 128 - 16 - 5, 4, (1, 4), cfg)[0] == 128
  with pytest.raises(ValueError, match='cfg.seq_len 128'):
    cl(16, 128 - 16 - 4, 4, (1, 4), cfg)
  with pytest.raises(ValueError, match='max_new_tokens'):
    cl(16, 0, 4, (1, 4), cfg)
  with pytest.raises(ValueError, match='empty prompt'):
    cl(0, 8, 4, (1, 4), cfg)
  assert 'sample' not in inspect.signature(cl).parameters
  for kw, word in ((dict(temperature=-1.0), 'temperature'), (dict(temperature=0, top_k=5), 'temperature 0 is greedy'), (dict(top_k=-2), 'top_k'),
                   (dict(temperature=1.0, top_p=0.0), 'top_p')):
    with pytest.raises(ValueError, match=word):
      cl(16, 8, 4, (1, 4), cfg, **kw)


def test_generate_lookup_signature_refusals_and_no_cpu_path():
  EC = dict(model='transformer', vocab_size=512, seq_len=128, d_model=128, expand='8/3', n_layers=2, n_heads=2, mlp_class='glu',
            tie_embeddings=False)
  model, _ = P.construct_model(namedtuple('Config', EC.keys())(**EC))
  ids = torch.zeros(1, 16, dtype=torch.int64)
  with pytest.raises(RuntimeError, match='MI355X'):  # the device check comes first, as in generate
    model.generate_lookup(ids, 8)
  sig = inspect.signature(model.generate_lookup)
  assert str(sig) == ('(prompt, max_new_tokens, n_draft=8, ngram=(1, 4), prompt_lens=None, eos_id=None, return_logprobs=False, temperature=None, '
                      'top_k=None, top_p=None, seed=None, return_stats=False)')
  assert inspect.unwrap(G.Generation.generate_lookup).__module__ == G.__name__
  body = inspect.getsource(G.Generation.generate_lookup).split('"""')[2]
  assert 'def ' not in body and 'lambda' not in body  # the round's state is _LookupSession's, not captured variables
  assert ops.LookupDraft._fields == ('draft_tokens', 'n_prop', 'match_len')
  assert str(inspect.signature(ops.lookup_draft)).startswith('(hist, lens, add_tok=None, n_add=None, k=') and \
      str(inspect.signature(ops.lookup_draft)).endswith('ngram=(1, 4), status=None)')
  z = torch.zeros
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.lookup_draft(z(2, 8, dtype=torch.int64), z(2, dtype=torch.int32), k=4)
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.spec_verify_lookup(z(6, 64, dtype=torch.bfloat16), z(2, 2, dtype=torch.int64), z(2, dtype=torch.int32), z(6), z(6, dtype=torch.int64),
                           z(2, 2), z(2))


def test_existing_callers_of_the_extended_helpers_get_what_they_got():
  d = torch.tensor([[5, 6, 7], [0, 0, 0], [0, 0, 0]])
  t = torch.tensor([[5, 6, 7, 8], [0, 0, 0, 9], [0, 0, 0, 9]])
  n, nxt = G.greedy_accept(d, t)
  assert n.tolist() == [3, 3, 3] and nxt.tolist() == [8, 9, 9]
  n, nxt = G.greedy_accept(d, t, torch.tensor([3, 0, 2], dtype=torch.int32))
  assert n.dtype == torch.int32 and n.tolist() == [3, 0, 2] and nxt.tolist() == [8, 0, 0]
  assert list(inspect.signature(G.speculative_loop).parameters)[:9] == ['first', 'draft_round', 'target_round', 'accept', 'max_new_tokens', 'n_draft',
                                                                        'eos_id', 'advance', 'all_done']
  assert inspect.signature(G.speculative_loop).parameters['drafted_in_round'].default is None


# ---- (e) the C entry points ------------------------------------------------------------------------------------------------------------------
def _lib_loaded():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


p = lambda: C.c_void_p(0x100000)  # noqa: E731  plausible, never dereferenced


def _refused(lib, name, *args):
  rc = getattr(lib, name)(*args)
  msg = (lib.plm_last_error_string() or b'').decode()
  assert rc == -1 and msg.startswith(name), (rc, msg)  # PLM_E_INVALID
  return msg


def test_the_header_declares_both_entry_points_and_the_abi_number_stays():
  lib = _lib_loaded()
  for name in ('plm_lookup_draft_i64', 'plm_spec_verify_lookup_bf16'):
    assert name in _lib.header_functions() and name in _lib.SIGNATURES and hasattr(lib, name)
  assert _lib.EXPECTED_ABI == 112 == lib.plm_version()


def test_lookup_draft_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  # hist, ld, lens, add_tok, ld_add, n_add, draft_tok, n_prop, match_len, status, B, k, g_min, g_max, stream
  ok = [p(), 64, p(), p(), 5, p(), p(), p(), p(), p(), 4, 4, 1, 4, None]
  for i in (0, 2, 6, 7, 9):  # every pointer that must be there
    a = list(ok)
    a[i] = None
    assert 'null pointer' in _refused(lib, 'plm_lookup_draft_i64', *a), i
  a = list(ok)
  a[3] = None
  assert 'n_add without add_tok' in _refused(lib, 'plm_lookup_draft_i64', *a)
  for v in (0, -1, 32, 1 << 20):
    a = list(ok)
    a[11] = v
    assert 'drafted tokens' in _refused(lib, 'plm_lookup_draft_i64', *a), v
  for g in ((0, 4), (3, 2), (1, 17), (17, 17)):
    a = list(ok)
    a[12], a[13] = g
    assert 'ngram' in _refused(lib, 'plm_lookup_draft_i64', *a), g
  for i, v in ((10, 0), (10, -3), (10, 1 << 31), (1, 0), (1, 1 << 31), (4, 0), (4, 1 << 31)):
    a = list(ok)
    a[i] = v
    assert 'bad shape' in _refused(lib, 'plm_lookup_draft_i64', *a), (i, v)
  for i in (0, 3, 6):
    a = list(ok)
    a[i] = C.c_void_p(0x100004)
    assert '8-byte aligned' in _refused(lib, 'plm_lookup_draft_i64', *a), i


def test_spec_verify_lookup_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  # p_logits, ldp, draft_tok, n_prop, p_cutoff, p_tok, u_accept, u_resid, temperature, n_accept, next_tok, logp, B, k, V, stream
  ok = [p(), 1008, p(), p(), p(), p(), p(), p(), 0.8, p(), p(), p(), 4, 4, 1000, None]
  for i in (0, 2, 3, 4, 5, 6, 7, 9, 10, 11):  # every pointer
    a = list(ok)
    a[i] = None
    assert 'null pointer' in _refused(lib, 'plm_spec_verify_lookup_bf16', *a), i
  for v in (0, -1, 32, 1 << 20):
    a = list(ok)
    a[13] = v
    assert 'drafted tokens' in _refused(lib, 'plm_spec_verify_lookup_bf16', *a), v
  for i, v in ((12, 0), (12, -3), (12, 1 << 26), (14, 0), (14, -1), (14, 1 << 31), (1, 999), (1, 0)):
    a = list(ok)
    a[i] = v
    if i == 14 and v > 1000:
      a[1] = v - 1
    assert 'bad shape' in _refused(lib, 'plm_spec_verify_lookup_bf16', *a), (i, v)
  a = list(ok)
  a[0] = C.c_void_p(0x100001)
  assert '2-byte aligned' in _refused(lib, 'plm_spec_verify_lookup_bf16', *a)
  for t in (0.0, -1.0, float('inf'), float('nan')):
    a = list(ok)
    a[8] = t
    assert 'temperature' in _refused(lib, 'plm_spec_verify_lookup_bf16', *a), t


# ---- (f) what the two wrappers hand the C ABI, against the recording fakes of tests/golden/make_ops_trace_parent.py ----------------------
def test_wrappers_hand_the_library_their_operands_and_refuse_before_any_launch():
  import importlib.util
  spec = importlib.util.spec_from_file_location('make_ops_trace_parent', os.path.join(ROOT, 'tests', 'golden', 'make_ops_trace_parent.py'))
  GEN = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(GEN)
  z, BF16, F32, I64, I32 = GEN.z, torch.bfloat16, torch.float32, torch.int64, torch.int32
  assert ops.lookup_draft.__module__ == 'plainlm_amd.ops_lookup' and ops.spec_verify_lookup.__module__ == 'plainlm_amd.ops_lookup'

  def run(call, **operands):
    rec = GEN.Recorder()
    for name, t in operands.items():
      rec.operand(name, t)
    with GEN.faked(rec):
      try:
        result = call(**operands)
      except (RuntimeError, TypeError, ValueError) as e:
        assert rec.launches() == 0, (type(e).__name__, str(e))
        return type(e).__name__, str(e)
      return rec.finish(result)
  B, ld, k, V = 3, 20, 4, 50
  draft = dict(hist=z((B, ld), I64), lens=z((B,), I32), add_tok=z((B, 5), I64), n_add=z((B,), I32), status=z((1,), I32))
  calls, ret = run(lambda **o: ops.lookup_draft(o['hist'], o['lens'], o['add_tok'], o['n_add'], k=k, ngram=(2, 4), status=o['status']), **draft)
  assert calls == [['plm_lookup_draft_i64', 'hist+0', ld, 'lens+0', 'add_tok+0', 5, 'n_add+0', 'ret0', 'ret1', 'ret2', 'status+0', B, k, 2, 4, 'stream']]
  assert ret == [f'int64[{B}, {k}]s[{k}, 1]', f'int32[{B}]s[1]', f'int32[{B}]s[1]']
  calls, ret = run(lambda **o: ops.lookup_draft(o['hist'], o['lens'], k=1), hist=draft['hist'], lens=draft['lens'])
  assert calls[0][4:7] == ['NULL', 0, 'NULL'] and calls[0][10] == 'scratch' and calls[0][11:] == [B, 1, 1, 4, 'stream']  # status made here
  for kw, kind, word in ((dict(hist=z((B, ld), I32)), 'TypeError', 'hist'), (dict(hist=z((B * ld,), I64)), 'ValueError', 'hist'),
                         (dict(lens=z((B + 1,), I32)), 'ValueError', 'lens'), (dict(lens=z((B,), I64)), 'TypeError', 'lens'),
                         (dict(add_tok=z((B + 1, 5), I64)), 'ValueError', 'add_tok'), (dict(add_tok=z((B, 5), I32)), 'TypeError', 'add_tok'),
                         (dict(n_add=z((B, 1), I32)), 'ValueError', 'n_add'), (dict(status=z((2,), I32)), 'ValueError', 'status'),
                         (dict(hist=torch.zeros(B, ld, dtype=I64)), 'RuntimeError', 'no CPU path'),
                         (dict(hist=z((B, 2 * ld), I64)[:, ::2]), 'ValueError', 'contiguous')):
    got = run(lambda **o: ops.lookup_draft(o['hist'], o['lens'], o['add_tok'], o['n_add'], k=k, status=o['status']), **{**draft, **kw})
    assert got[0] == kind and word in got[1], (kw.keys(), got)
  ver = dict(tl=z((B * (k + 1), V), BF16, ld=V + 6), tok=z((B, k), I64), np=z((B,), I32), pc=z((B * (k + 1),), F32), pt=z((B * (k + 1),), I64),
             ua=z((k, B), F32), ur=z((B,), F32))
  calls, ret = run(lambda **o: ops.spec_verify_lookup(*o.values(), temperature=0.5), **ver)
  assert calls == [['plm_spec_verify_lookup_bf16', 'tl+0', V + 6, 'tok+0', 'np+0', 'pc+0', 'pt+0', 'ua+0', 'ur+0', 0.5, 'ret0', 'ret1', 'ret2', B, k, V,
                    'stream']]
  assert ret == [f'int32[{B}]s[1]', f'int64[{B}]s[1]', f'float32[{B}, {k + 1}]s[{k + 1}, 1]']
  for kw, kind, word in ((dict(tl=z((B * k, V), BF16)), 'ValueError', 'target_logits'), (dict(tl=z((B * (k + 1), V), F32)), 'ValueError', 'target_logits'),
                         (dict(tok=z((B, k), I32)), 'TypeError', 'draft_tokens'), (dict(np=z((B + 1,), I32)), 'ValueError', 'n_prop'),
                         (dict(np=z((B,), I64)), 'TypeError', 'n_prop'), (dict(pc=z((B * k,), F32)), 'ValueError', 'target_cutoff'),
                         (dict(pt=z((B * (k + 1),), I32)), 'TypeError', 'target_tokens'), (dict(ua=z((k, B + 1), F32)), 'ValueError', 'u_accept'),
                         (dict(ur=z((B,), torch.float64)), 'TypeError', 'u_resid')):
    got = run(lambda **o: ops.spec_verify_lookup(*o.values()), **{**ver, **kw})
    assert got[0] == kind and word in got[1], (kw.keys(), got)
