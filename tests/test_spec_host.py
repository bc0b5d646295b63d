"""CPU tests (no GPU) of speculative decoding: the acceptance rule of tests/spec_ref.py leaves the target's
distribution exact; generate.speculative_loop over fake models emits what generate.generate_loop emits, moves the fake caches as the
real ones must move, and never shows the draft a token twice; the refusals of check_speculative and of plm_spec_verify_bf16 (before any
HIP call); greedy_accept and commit_round on hand-written cases."""

import ctypes as C
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib
from plainlm_amd import generate as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import sample_ref as R  # noqa: E402
import spec_ref as S  # noqa: E402


# ---- (a) the rule is exact ---------------------------------------------------------------------------------------------------------------
def _pairs(V):
  """(name, p logits, q logits) fp64 rows."""
  rng = np.random.default_rng(V)
  x = rng.normal(0, 2, V)
  even = np.where(np.arange(V) % 2 == 0, x, -np.inf)
  odd = np.where(np.arange(V) % 2 == 1, rng.normal(0, 2, V), -np.inf)
  return [('p = q', x, x.copy()), ('random', x, rng.normal(0, 2, V)), ('close', x, x + rng.normal(0, 0.1, V)), ('disjoint', even, odd),
          ('q one-hot', x, np.where(np.arange(V) == 1, 0.0, -np.inf)), ('p one-hot', np.where(np.arange(V) == V - 1, 0.0, -np.inf), x),
          ('ties', np.round(x), np.round(x[::-1]))]


@pytest.mark.parametrize('V', [5, 8])
@pytest.mark.parametrize('tau', [0.5, 1.0, 3.0])
def test_the_first_emitted_token_is_distributed_as_the_target(V, tau):
  for name, xp, xq in _pairs(V):
    for top_k, top_p in ((0, 1.0), (3, 1.0), (0, 0.8)):
      cp = R.Rows(xp[None]).keep_set(tau, top_k, top_p)['cutoff'][0]
      cq = R.Rows(xq[None]).keep_set(tau, top_k, top_p)['cutoff'][0]
      Pd, Qd = S.Dist(xp, tau, cp), S.Dist(xq, tau, cq)
      got = S.first_token_distribution(Pd, Qd)
      assert np.abs(got - Pd.prob).max() <= 1e-12, (name, top_k, top_p, got, Pd.prob)
      assert abs(got.sum() - 1.0) <= 1e-12


@pytest.mark.parametrize('V', [5, 8])
def test_k_1_and_k_2_rounds_emit_the_target_distribution_at_every_position(V):
  """k = 1: P(n_accept, next_tok) summed over the draft's draw gives p_0 for the first token and p_1 for the bonus after an accepted one.
  k = 2: given that row 0 accepted x, the second token (accepted d_2, or row 1's residual) is distributed as p_1."""
  rng = np.random.default_rng(V + 100)
  tau = 0.8
  for _ in range(4):
    xs = rng.normal(0, 2, (4, V))
    P0, P1, Q0, Q1 = (S.Dist(x, tau, -np.inf) for x in xs)
    # k = 1, by enumeration through verify(): u_acc on a fine grid is replaced by its exact measure alpha
    first = np.zeros(V)
    for x in range(V):
      a = S.alpha(P0, Q0, x)
      n, nxt, _ = S.verify([P0, P1], [Q0], [x], [0, 3], [0.0], 0.0)  # u = 0: accepted whenever alpha > 0
      assert n == (1 if a > 0 else 0) and (nxt == 3 if n == 1 else True)   # the bonus token is the target sampler's token of row 1
      first[x] += Q0.prob[x] * a
    r, Cr = S.residual(P0, Q0)
    first += (1.0 - first.sum()) * r / Cr[-1]
    assert np.abs(first - P0.prob).max() <= 1e-12
    assert np.abs(S.first_token_distribution(P1, Q1) - P1.prob).max() <= 1e-12  # k = 2: row 1 is the same rule on (p_1, q_1)
    # the residual draw walks the columns in ascending order
    for u in (0.0, 0.3, 0.999999):
      i = S.draw(Cr, u)
      assert Cr[i] > u * Cr[-1] and (i == 0 or Cr[i - 1] <= u * Cr[-1])


def test_reference_verify_on_hand_written_rows():
  V, tau = 4, 1.0
  ln = np.log
  p = S.Dist(ln([0.5, 0.25, 0.25, 1e-300]), tau, -np.inf)
  q = S.Dist(ln([0.25, 0.5, 0.25, 1e-300]), tau, -np.inf)
  assert S.alpha(p, q, 0) == 1.0 and abs(S.alpha(p, q, 1) - 0.5) < 1e-15 and S.alpha(p, q, 2) == 1.0
  assert S.alpha(p, q, -1) == 0.0 and S.alpha(p, q, V) == 0.0
  r, Cr = S.residual(p, q)
  assert np.allclose(r, [0.25, 0, 0, 0]) and S.draw(Cr, 0.7) == 0
  # token 1, u = 0.6 >= alpha = 0.5: rejected at row 0, the residual is all on column 0
  n, nxt, lp = S.verify([p, p], [q], [1], [2, 3], [0.6], 0.9)
  assert (n, nxt) == (0, 0) and abs(lp[0] - ln(0.5)) < 1e-12 and lp[1] == 0
  # u = 0.4 < alpha: accepted, the bonus token is p_tok[1]
  n, nxt, lp = S.verify([p, p], [q], [1], [2, 3], [0.4], 0.9)
  assert (n, nxt) == (1, 3) and abs(lp[0] - ln(0.25)) < 1e-12 and lp[1] < -600
  # a kept set: cutoff ln 0.25 keeps three columns of p; token 3 is outside it
  pk = S.Dist(ln([0.5, 0.25, 0.25, 1e-3]), tau, ln(0.25))
  assert pk.keep.tolist() == [True, True, True, False] and S.alpha(pk, q, 3) == 0.0
  qk = S.Dist(ln([0.25, 0.5, 0.25, 1e-3]), tau, ln(0.5))
  assert S.alpha(pk, qk, 0) == 1.0  # q(0) = 0 < p(0)
  # p = q: R = 0, the fallback is the target sampler's token
  assert S.draw(S.residual(p, p)[1], 0.5) is None
  assert S.verify([p, p], [p], [9], [2, 3], [0.0], 0.5)[:2] == (0, 2)
  # NaN cutoff / no finite logit: nothing kept
  e = S.Dist(np.full(V, np.nan), tau, np.nan)
  assert e.Z == 0 and S.alpha(e, q, 0) == 0.0 and np.isnan(S.verify([e, e], [q], [0], [0, 0], [0.0], 0.5)[2][0])


# ---- (b) speculative_loop against generate_loop ----------------------------------------------------------------------------------------------
VOC = 23


def lm_next(ctx):
  """The toy language model: the next token and its log-probability as a function of the whole context (position included)."""
  t = (sum((i + 1) * c for i, c in enumerate(ctx[-3:])) + 7 * len(ctx)) % VOC
  return t, -float((t * 37 + len(ctx)) % 101) / 64.0 - 0.015625


class FakePair:
  """A fake target and a fake draft with list-of-token caches.  draft kinds per sequence: 'perfect', 'wrong', 'random'."""

  def __init__(self, prompts, kinds, k, seed=0):
    self.k, self.kinds = k, kinds
    self.tcache = [list(p) for p in prompts]
    self.dcache = [list(p) for p in prompts]
    self.rng = np.random.default_rng(seed)
    self.fed = [list(p) for p in prompts]  # every token the draft was ever shown, in order, rollbacks removed
    self.round_rows = None

  def first(self):
    r = [lm_next(c) for c in self.tcache]
    return torch.tensor([t for t, _ in r]), torch.tensor([lp for _, lp in r], dtype=torch.float32)

  def step(self, tok):  # generate_loop's decode step on the target
    out = []
    for b, t in enumerate(tok.tolist()):
      self.tcache[b].append(t)
      out.append(lm_next(self.tcache[b]))
    return torch.tensor([t for t, _ in out]), torch.tensor([lp for _, lp in out], dtype=torch.float32)

  def guess(self, b, ctx):
    t = lm_next(ctx)[0]
    kind = self.kinds[b]
    if kind == 'wrong' or (kind == 'random' and self.rng.random() < 0.4):
      t = (t + 1 + int(self.rng.integers(0, VOC - 1))) % VOC
    return t

  def draft_round(self, last, carry_tok, carry, live):
    toks, self.round_rows = [], []
    for b in range(len(self.dcache)):
      if not bool(live[b]):
        toks.append([0] * self.k)
        self.round_rows.append([])
        continue
      # the draft holds the sequence up to, not including, its newest token - less the carried one
      assert self.dcache[b] + ([int(carry_tok[b])] if bool(carry[b]) else []) == self.tcache[b], (b, 'the draft cache went out of step')
      fed = ([int(carry_tok[b])] if bool(carry[b]) else []) + [int(last[b])]
      ctx = self.dcache[b] + fed
      row = []
      for i in range(self.k):
        row.append(self.guess(b, ctx))
        if i < self.k - 1:
          fed.append(row[-1])
          ctx = ctx + [row[-1]]
      self.dcache[b] = self.dcache[b] + fed
      self.round_rows.append(fed)
      toks.append(row)
    return torch.tensor(toks), None

  def target_round(self, last, draft_tok, live):
    pred, lp = [], []
    self.chunks = []
    for b in range(len(self.tcache)):
      chunk = [int(last[b])] + draft_tok[b].tolist()
      self.chunks.append(chunk)
      r = [lm_next(self.tcache[b] + chunk[:i + 1]) for i in range(self.k + 1)] if bool(live[b]) else [(0, 0.0)] * (self.k + 1)
      pred.append([t for t, _ in r])
      lp.append([x for _, x in r])
    return torch.tensor(pred), torch.tensor(lp, dtype=torch.float32)

  @staticmethod
  def accept(draft_tok, _, out):
    return G.greedy_accept(draft_tok, out[0]) + (out[1],)

  def advance(self, moved, live):
    for b, m in enumerate(moved.tolist()):
      if not bool(live[b]):
        assert m == 0
        continue
      self.tcache[b] = self.tcache[b] + self.chunks[b][:m]
      rows = self.round_rows[b]
      carried = len(rows) - self.k            # 1 when the round began with the carried token
      keep = carried + min(m, self.k)
      self.dcache[b] = self.dcache[b][:len(self.dcache[b]) - len(rows) + keep]
      self.fed[b] = self.fed[b] + rows[:keep]


PROMPTS = [[3, 1, 4, 1, 5], [9, 2, 6], [5, 3, 5, 8, 9, 7], [2, 7]]


def _reference(N, eos_id=None):
  f = FakePair(PROMPTS, ['perfect'] * 4, 1)
  return G.generate_loop(f.first(), f.step, N, eos_id, check_every=1)


@pytest.mark.parametrize('k', [1, 3, 8])
@pytest.mark.parametrize('kinds', [['perfect'] * 4, ['wrong'] * 4, ['random'] * 4, ['perfect', 'wrong', 'random', 'perfect']])
def test_speculative_loop_emits_what_generate_loop_emits(k, kinds):
  N = 21
  want_t, want_l = _reference(N)
  eos_cases = [None, int(want_t[0, 5]), int(want_t[2, 0]), int(want_t[1, N - 1])]  # mid-round, the very first token, the last column
  for eos in eos_cases:
    wt, wl = (want_t, want_l) if eos is None else _reference(N, eos)
    f = FakePair(PROMPTS, kinds, k, seed=k)
    reads = []
    toks, lps, stats = G.speculative_loop(f.first(), f.draft_round, f.target_round, f.accept, N, k, eos, f.advance,
                                          all_done=lambda d: reads.append(1) or bool(d.all()))
    assert torch.equal(toks, wt), (eos, toks, wt)
    assert torch.equal(lps, wl), eos
    assert stats['rounds'] <= N - 1 and len(reads) <= stats['rounds'] + 1  # one read per round (and the one that ends the loop)
    for b in range(4):
      hit = (wt[b] == eos).nonzero() if eos is not None else []
      count = int(hit[0]) + 1 if len(hit) else N
      # the caches hold the prompt and every emitted token but the newest; the draft has seen each of them once, or lacks the last one
      seq = PROMPTS[b] + wt[b, :count - 1].tolist()
      assert f.tcache[b] == seq, (b, eos)
      assert f.dcache[b] in (seq, seq[:-1]) and f.fed[b] == f.dcache[b], (b, eos)
    d, a = stats['drafted'].tolist(), stats['accepted'].tolist()
    assert all(x % k == 0 and 0 <= y <= x for x, y in zip(d, a))
    if eos is None:
      if kinds[0] == 'perfect':
        assert a[0] == d[0] and stats['rounds'] == -(-(N - 1) // (k + 1)) if len(set(kinds)) == 1 else a[0] == d[0]
      if kinds[1] == 'wrong':
        assert a[1] == 0 and stats['rounds'] == N - 1 and d[1] == k * (N - 1)


def test_speculative_loop_one_token_and_all_finished_at_once():
  f = FakePair(PROMPTS, ['perfect'] * 4, 3)
  toks, lps, stats = G.speculative_loop(f.first(), f.draft_round, f.target_round, f.accept, 1, 3)
  assert tuple(toks.shape) == (4, 1) and stats['rounds'] == 0 and torch.equal(toks[:, 0], f.first()[0])
  # every sequence emits eos_id at once: no round runs, the rest is frozen
  first = (torch.tensor([4, 4]), torch.tensor([-1.0, -2.0]))
  boom = lambda *a: (_ for _ in ()).throw(AssertionError('a round ran'))  # noqa: E731
  toks, lps, stats = G.speculative_loop(first, boom, boom, boom, 6, 2, eos_id=4)
  assert toks.tolist() == [[4] * 6] * 2 and lps[:, 0].tolist() == [-1.0, -2.0] and (lps[:, 1:] == 0).all() and stats['rounds'] == 0


# ---- (c) check_speculative -------------------------------------------------------------------------------------------------------------------
Cfg = namedtuple('Cfg', ['vocab_size', 'seq_len'])


def test_check_speculative_refuses_and_normalises():
  cs = G.check_speculative
  big, small = Cfg(512, 128), Cfg(512, 64)
  assert cs(16, 32, 4, big, big) == (53, None)
  assert cs(16, 32, 4, big, small, 'cpu', 'cpu', 0.8, 5, None, 3) == (53, (0.8, 5, 1.0))
  assert cs(16, 32, 4, big, big, temperature=0) == (53, None) and cs(16, 32, 31, big, big)[0] == 80
  for n in (0, -1, 32, 100):
    with pytest.raises(ValueError, match='n_draft'):
      cs(16, 32, n, big, big)
  for n in (4.0, '4', None, True):
    with pytest.raises(TypeError, match='n_draft'):
      cs(16, 32, n, big, big)
  assert cs(16, 128 - 16 - 5, 4, big, big)[0] == 128
  with pytest.raises(ValueError, match="the target's cfg.seq_len 128"):
    cs(16, 128 - 16 - 4, 4, big, big)
  with pytest.raises(ValueError, match="the draft's cfg.seq_len 64"):
    cs(16, 44, 4, big, small)
  assert cs(16, 43, 4, big, small)[0] == 64
  with pytest.raises(ValueError, match='vocab_size'):
    cs(16, 8, 4, big, Cfg(256, 128))
  with pytest.raises(ValueError, match='the draft is on'):
    cs(16, 8, 4, big, big, 'cpu', 'meta')
  with pytest.raises(ValueError, match='sample='):
    cs(16, 8, 4, big, big, sample=lambda lf: lf.argmax(-1))
  with pytest.raises(ValueError, match='max_new_tokens'):
    cs(16, 0, 4, big, big)
  with pytest.raises(ValueError, match='empty prompt'):
    cs(0, 8, 4, big, big)
  # the sampling-argument rules are check_sampling's
  for kw, word in ((dict(temperature=-1.0), 'temperature'), (dict(temperature=0, top_k=5), 'temperature 0 is greedy'), (dict(top_k=-2), 'top_k'),
                   (dict(temperature=1.0, top_p=0.0), 'top_p')):
    with pytest.raises(ValueError, match=word):
      cs(16, 8, 4, big, big, **kw)


def test_generate_speculative_refuses_before_any_launch_and_ops_has_no_cpu_path():
  EC = dict(model='transformer', vocab_size=512, seq_len=128, d_model=128, expand='8/3', n_layers=2, n_heads=2, mlp_class='glu',
            tie_embeddings=False)
  model, _ = P.construct_model(namedtuple('Config', EC.keys())(**EC))
  ids = torch.zeros(1, 16, dtype=torch.int64)
  with pytest.raises(RuntimeError, match='MI355X'):  # the device check comes first, as in generate
    model.generate_speculative(ids, 8, model)
  import inspect
  names = list(inspect.signature(model.generate_speculative).parameters)
  assert names == ['prompt', 'max_new_tokens', 'draft', 'n_draft', 'prompt_lens', 'eos_id', 'return_logprobs', 'temperature', 'top_k', 'top_p',
                   'seed', 'return_stats']
  assert inspect.signature(model.generate_speculative).parameters['n_draft'].default == 4
  from plainlm_amd import ops
  assert ops.SpecVerify._fields == ('n_accept', 'next_token', 'logprob')
  z = torch.zeros
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.spec_verify(z(6, 64, dtype=torch.bfloat16), z(4, 64, dtype=torch.bfloat16), z(2, 2, dtype=torch.int64), z(6), z(4),
                    z(6, dtype=torch.int64), z(2, 2), z(2))


def test_uniforms_of_a_call_are_drawn_once_and_no_entry_is_used_twice():
  N, k, B = 7, 3, 2
  u = G.speculative_uniforms(N, k, B, 'cpu', seed=9)
  assert tuple(u.shape) == (1 + (N - 1) * (3 * k + 2), B) and torch.equal(u, G.speculative_uniforms(N, k, B, 'cpu', seed=9))
  assert torch.equal(u, G.draw_uniforms(u.shape[0], B, 'cpu', seed=9))  # draw_uniforms as it is
  mark = torch.arange(u.numel(), dtype=torch.float32).view_as(u)
  seen = [mark[0]]
  for i in range(N - 1):
    ud, ut, ua, ur = G.round_uniforms(mark, i, k)
    assert tuple(ud.shape) == (k, B) and tuple(ut.shape) == (k + 1, B) and tuple(ua.shape) == (k, B) and tuple(ur.shape) == (B,)
    assert ud.is_contiguous() and ua.is_contiguous() and ur.is_contiguous()
    seen += [ud.reshape(-1), ut.reshape(-1), ua.reshape(-1), ur]
  allv = torch.cat([s.reshape(-1) for s in seen])
  assert allv.numel() == u.numel() and allv.unique().numel() == u.numel()


# ---- (d) the C entry point -------------------------------------------------------------------------------------------------------------------
def _lib_loaded():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


p = lambda: C.c_void_p(0x100000)  # noqa: E731  plausible, never dereferenced


def test_spec_verify_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()

  def refused(*args):
    rc = lib.plm_spec_verify_bf16(*args)
    msg = (lib.plm_last_error_string() or b'').decode()
    assert rc == -1 and 'plm_spec_verify_bf16' in msg, (rc, msg)  # PLM_E_INVALID
    return msg
  # p_logits, ldp, q_logits, ldq, draft_tok, p_cutoff, q_cutoff, p_tok, u_accept, u_resid, temperature, n_accept, next_tok, logp, B, k, V, stream
  ok = [p(), 1000, p(), 1008, p(), p(), p(), p(), p(), p(), 0.8, p(), p(), p(), 4, 4, 1000, None]
  for i in (0, 2, 4, 5, 6, 7, 8, 9, 11, 12, 13):  # every pointer
    a = list(ok)
    a[i] = None
    assert 'null pointer' in refused(*a), i
  for v in (0, -1, 32, 1 << 20):
    a = list(ok)
    a[15] = v
    assert 'drafted tokens' in refused(*a), v
  for i, v in ((14, 0), (14, -3), (14, 1 << 26), (16, 0), (16, -1), (16, 1 << 31), (1, 999), (3, 999), (1, 0)):  # B, V, ldp < V, ldq < V
    a = list(ok)
    a[i] = v
    if i == 16 and v > 1000:
      a[1] = a[3] = v
    assert 'bad shape' in refused(*a), (i, v)
  for i in (0, 2):
    a = list(ok)
    a[i] = C.c_void_p(0x100001)
    assert '2-byte aligned' in refused(*a), i
  for t in (0.0, -1.0, float('inf'), float('nan')):
    a = list(ok)
    a[10] = t
    assert 'temperature' in refused(*a), t
  assert 'plm_spec_verify_bf16' in _lib.header_functions() and _lib.EXPECTED_ABI == 112 == lib.plm_version()


# ---- (e) greedy_accept and commit_round ------------------------------------------------------------------------------------------------------
def test_greedy_accept_counts_leading_matches():
  d = torch.tensor([[5, 6, 7], [5, 6, 7], [5, 6, 7], [5, 6, 7], [1, 1, 1]])
  t = torch.tensor([[5, 6, 7, 8], [5, 9, 7, 8], [4, 6, 7, 8], [5, 6, 9, 8], [1, 1, 1, 1]])
  n, nxt = G.greedy_accept(d, t)
  assert n.dtype == torch.int32 and nxt.dtype == torch.int64
  assert n.tolist() == [3, 1, 0, 2, 3] and nxt.tolist() == [8, 9, 4, 9, 1]  # a later match after a mismatch does not count
  n, nxt = G.greedy_accept(torch.tensor([[2]]), torch.tensor([[2, 3]]))
  assert n.tolist() == [1] and nxt.tolist() == [3]


def test_commit_round_scatters_truncates_and_freezes():
  N, k = 8, 3
  out_t = torch.full((5, N), -1, dtype=torch.int64)
  out_l = torch.full((5, N), 9.0)
  count = torch.tensor([1, 6, 3, 2, 8], dtype=torch.int32)
  done = torch.tensor([False, False, False, True, True])
  draft = torch.tensor([[10, 11, 12], [20, 21, 22], [30, 99, 32], [40, 41, 42], [50, 51, 52]])
  n_acc = torch.tensor([3, 3, 2, 3, 0], dtype=torch.int32)
  nxt = torch.tensor([13, 23, 33, 43, 53])
  lp = -torch.arange(20, dtype=torch.float32).view(5, 4) - 1
  c, d, moved = G.commit_round(out_t, out_l, count, done, draft, n_acc, nxt, lp, eos_id=99)
  assert moved.dtype == torch.int32 and moved.tolist() == [4, 2, 2, 0, 0]
  assert c.tolist() == [5, 8, 5, 2, 8] and d.tolist() == [False, True, True, True, True]
  assert count.tolist() == [1, 6, 3, 2, 8] and done.tolist() == [False, False, False, True, True]  # the inputs are not modified
  assert out_t[0].tolist() == [-1, 10, 11, 12, 13, -1, -1, -1] and out_l[0].tolist() == [9, -1, -2, -3, -4, 9, 9, 9]
  assert out_t[1].tolist() == [-1] * 6 + [20, 21] and out_l[1, 6:].tolist() == [-5, -6]          # cut at N
  assert out_t[2].tolist() == [-1, -1, -1, 30, 99, 99, 99, 99] and out_l[2].tolist() == [9, 9, 9, -9, -10, 0, 0, 0]  # cut after eos_id, frozen
  assert out_t[3].tolist() == [-1, -1, 99, 99, 99, 99, 99, 99] and out_l[3, 2:].tolist() == [0] * 6   # finished before: takes nothing
  assert out_t[4].tolist() == [-1] * N                                                               # full: no column left
  # without eos_id nothing is frozen; a rejected-at-once round takes next_token alone
  out_t = torch.zeros((1, 4), dtype=torch.int64)
  out_l = torch.zeros((1, 4))
  c, d, moved = G.commit_round(out_t, out_l, torch.tensor([1]), torch.tensor([False]), torch.tensor([[7, 7]]), torch.tensor([0]),
                               torch.tensor([5]), torch.tensor([[-0.5, -1.5, -2.5]]))
  assert out_t.tolist() == [[0, 5, 0, 0]] and out_l.tolist() == [[0, -0.5, 0, 0]] and c.tolist() == [2] and not d.any() and moved.tolist() == [1]
