"""Speculative decoding on a real MI355X: plm_spec_verify_bf16 against the fp64 restatement of its rule (tests/spec_ref.py), determinism
and sequence independence, and Transformer.generate_speculative on the 2-layer golden model.

Bounds (derived from sample.hip's stated weight error, not measured; the observed figures are printed and recorded in DESIGN.md section
15).  A fixed-point weight w (relative to the row maximum's 1) is off by at most 1.2e-7 |d / tau| = 1.2e-7 |ln w| of itself (the
exponential's argument carries two roundings) plus 2^-40 of truncation, and a sum of them by 1.2e-7 ln V + V 2^-40 of Z (the softmax
mean of |d / tau| is at most ln V; Z >= 1):
    e_w(w) = 1.2e-7 |ln w| + 2^-40 / w        e_Z = 1.2e-7 ln V + V 2^-40
  accept     alpha = (wp_x / Zp) / (wq_x / Zq) carries the four relative errors, so the kernel's alpha is within
             d = 2 * min(1, alpha) * (e_w(wp_x) + e_w(wq_x) + 2 e_Z) of the reference's (2x slack, as test_sample_gpu.py takes it): row r must
             be accepted when u < alpha - d and rejected when u > alpha + d; in between either verdict is right.  A weight near the
             fixed point's 2^-40 makes d exceed 1 by itself: nothing is asserted about a token that neither sampler could have drawn.
             alpha = 0 (token outside [0, V) or outside p's kept set) and alpha = 1 by q(x) = 0 are exact: d = 0.
  residual   p_i = wp_i / Zp is off by p_i (e_w + e_Z), so any partial sum of max(0, p_i - q_i) is off by at most
             delta = 4 e_Z + V 2^-40 (both distributions' weight and Z errors, and the residual's own truncation) - an ABSOLUTE error,
             in units of probability, however small R is.  The kernel's token satisfies C_prev <= u R < C_tok on its own sums, so on the
             reference's: C_prev - d R <= u R <= C_tok + d R with d R = 4 delta (the sum's error and R's, 2x slack).  The kernel's R can
             be 0 only where the reference's R <= delta: the fallback (the target sampler's token) is accepted for R <= 4 delta.
  logp       within LOGP_TOL = 3e-5 nats of the fp64 log softmax (test_sample_gpu.py's bound), exactly 0 beyond n_accept."""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_ref as R  # noqa: E402
import spec_ref as S  # noqa: E402
from test_sample_gpu import LOGIT_TOL, LOGP_MODEL_TOL, LOGP_TOL, TAUS  # noqa: E402

BF16 = torch.bfloat16
FIX = 2.0 ** -40
FILTERS = ((0, 1.0), (50, 0.95))  # an unfiltered and a filtered cutoff
KINDS = ('same', 'disjoint', 'rand1', 'rand8', 'ties', 'nonfinite', 'bad_tok', 'unkept')
VS, BS, KS = (1, 7, 257, 1000, 50280), (1, 5), (1, 4, 8)
observed = {'accept': 0.0, 'residual': 0.0, 'logp': 0.0, 'between': 0, 'rows': 0, 'accepted': 0, 'resid_draws': 0, 'fallbacks': 0}


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


def e_w(lnw):
  return 1.2e-7 * abs(lnw) + FIX * np.exp(min(-lnw, 700.0))


def e_z(V):
  return 1.2e-7 * np.log(V) + V * FIX


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def seq_rows(kind, V, k, g):
  """(target rows fp32 [k + 1, V], draft rows fp32 [k, V]) of one sequence of the named class."""
  rn = lambda n, s: torch.randn(n, V, generator=g) * s  # noqa: E731
  if kind == 'same':
    xp = rn(k + 1, 2.0)
    return xp, xp[:k].clone()
  if kind == 'disjoint':  # p lives on the even columns, q on the odd ones
    xp, xq = rn(k + 1, 2.0), rn(k, 2.0)
    xp[:, 1::2] = float('-inf')
    xq[:, 0::2] = float('-inf')
    return xp, xq
  if kind == 'rand8':
    xp = rn(k + 1, 8.0)
    return xp, xp[:k] + rn(k, 2.0)
  if kind == 'ties':
    return torch.round(rn(k + 1, 2.0)), torch.round(rn(k, 2.0))
  xp = rn(k + 1, 1.0)
  xq = xp[:k] + rn(k, 0.5)
  if kind == 'nonfinite':
    for x in (xp, xq):
      m = torch.rand(x.shape, generator=g)
      x[m < 0.2] = float('-inf')
      x[m > 0.9] = float('nan')
  return xp, xq  # rand1, bad_tok, unkept


_cases = {}


def case(V, B, k, padded=0):
  key = (V, B, k, padded)
  if key not in _cases:
    g = torch.Generator().manual_seed(1000 * V + 10 * B + k)
    off = VS.index(V) + 2 * KS.index(k) if V in VS and k in KS else 0
    kinds = [KINDS[(b + off) % len(KINDS)] for b in range(B)]
    rows = [seq_rows(kd, V, k, g) for kd in kinds]
    xp = torch.stack([r[0] for r in rows]).to(BF16)                  # [B, k + 1, V]
    xq = torch.stack([r[1] for r in rows], dim=1).to(BF16)           # [k, B, V]: step-major
    if 'unkept' in kinds:  # the drafted token of row 0 will be p's argmax; q does not hold it
      b = kinds.index('unkept')
      xq[0, b, int(xp[b, 0].float().argmax())] = float('-inf')

    def dev(x, rows_):
      if not padded:
        return x.reshape(rows_, V).cuda()
      buf = torch.full((rows_, V + 13), float('nan'), dtype=BF16, device='cuda')
      buf[:, :V].copy_(x.reshape(rows_, V))
      return buf[:, :V]
    _cases[key] = dict(V=V, B=B, k=k, kinds=kinds, xp=xp.double().numpy(), xq=xq.double().numpy(), dp=dev(xp, B * (k + 1)), dq=dev(xq, k * B))
  return _cases[key]


def prepare(ops, c, tau, top_k, top_p, rng):
  """The inputs as generate_speculative makes them: both samplers run on the device and hand over their tokens and cutoffs; then the
  planted tokens.  Returns the device inputs and their host copies."""
  V, B, k = c['V'], c['B'], c['k']
  f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).cuda()  # noqa: E731
  st = ops.sample_logits(c['dp'], f32(rng.uniform(0, 1, B * (k + 1))), tau, top_k, top_p, want_stats=True)
  sq = ops.sample_logits(c['dq'], f32(rng.uniform(0, 1, k * B)), tau, top_k, top_p, want_stats=True)
  tok = sq.tokens.view(k, B).clone()
  for b, kind in enumerate(c['kinds']):
    if kind == 'bad_tok':
      tok[k // 2, b] = V + 3 if V % 2 else -1
    if kind == 'unkept':
      tok[0, b] = int(np.nanargmax(np.where(np.isfinite(c['xp'][b, 0]), c['xp'][b, 0], -np.inf)))
  return dict(tok=tok, pcut=st.cutoff, qcut=sq.cutoff.view(k, B), ptok=st.tokens)


def launch(ops, c, inp, ua, ures, tau):
  f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32)).cuda()  # noqa: E731
  r = ops.spec_verify(c['dp'], c['dq'], inp['tok'], inp['pcut'], inp['qcut'].reshape(-1), inp['ptok'], f32(ua), f32(ures), tau)
  return tuple(t.cpu().numpy() for t in r)


def same_bits(a, b):
  return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ---- the check -----------------------------------------------------------------------------------------------------------------------------
def check(c, inp, ua, ures, tau, got, tag, memo):
  """memo: the reference distributions of this (tau, filter) setting, built once per row and shared by its launches."""
  V, B, k = c['V'], c['B'], c['k']
  n_acc, nxt, logp = got
  tok, pcut, qcut, ptok = (inp[n].cpu().numpy() for n in ('tok', 'pcut', 'qcut', 'ptok'))
  ptok = ptok.reshape(B, k + 1)
  pcut = pcut.reshape(B, k + 1)

  def dist_p(b, r):
    if ('p', b, r) not in memo:
      memo['p', b, r] = S.Dist(c['xp'][b, r], tau, pcut[b, r])
    return memo['p', b, r]

  def dist_q(b, r):
    if ('q', b, r) not in memo:
      memo['q', b, r] = S.Dist(c['xq'][r, b], tau, qcut[r, b])
    return memo['q', b, r]
  assert n_acc.dtype == np.int32 and nxt.dtype == np.int64 and logp.dtype == np.float32 and logp.shape == (B, k + 1)
  assert ((n_acc >= 0) & (n_acc <= k)).all() and ((nxt >= 0) & (nxt < V)).all(), (tag, n_acc, nxt)
  uc = R.clamp_u(np.asarray(ua, dtype=np.float32))
  delta = 4 * e_z(V) + V * FIX
  for b in range(B):
    t = tag + (b, c['kinds'][b])
    na = int(n_acc[b])
    for r in range(min(na + 1, k)):
      Pd, Qd = dist_p(b, r), dist_q(b, r)
      x = int(tok[r, b])
      al = S.alpha(Pd, Qd, x)
      exact = not 0 <= x < V or Pd.prob[x] == 0 or Qd.prob[x] == 0
      d = 0.0 if exact else 2 * al * (e_w(Pd.lnw[x]) + e_w(Qd.lnw[x]) + 2 * e_z(V))
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
    if na == k:
      assert nxt[b] == ptok[b, k], (t, 'the bonus token is the target sampler\'s')
    else:
      Qd = dist_q(b, na)
      res, Cr = S.residual(Pd, Qd)
      Rr = Cr[-1]
      i = int(nxt[b])
      lo, hi = Cr[i] - res[i], Cr[i]
      uR = float(R.clamp_u(np.float32(ures[b]))) * Rr
      miss = max(lo - uR, uR - hi)
      if miss > 4 * delta or not Pd.prob[i] > 0:
        assert i == ptok[b, na] and Rr <= 4 * delta, (t, 'residual draw', i, miss, delta, Rr, int(ptok[b, na]))
        observed['fallbacks'] += 1
      else:
        observed['resid_draws'] += 1
        observed['residual'] = max(observed['residual'], miss / delta)
    ref = Pd.logp[int(nxt[b])]
    if np.isnan(ref):
      assert np.isnan(logp[b, na]), (t, logp[b, na])
    else:
      assert abs(float(logp[b, na]) - ref) <= LOGP_TOL, (t, logp[b, na], ref)
      observed['logp'] = max(observed['logp'], abs(float(logp[b, na]) - ref))
    assert (logp[b, na + 1:].view(np.uint32) == 0).all(), (t, 'entries beyond n_accept are 0')
    # the classes' own outcomes
    kind = c['kinds'][b]
    if kind == 'same':
      assert na == k, (t, 'q is bit-equal to p: every row is accepted')
    if kind == 'disjoint' and V > 1:
      assert na == 0 and nxt[b] % 2 == 0, (t, 'disjoint kept sets: rejected at row 0, the residual is p')
    if kind == 'bad_tok':
      assert na <= k // 2, (t, 'a token outside [0, V) is never accepted')
    if kind == 'unkept' and np.isfinite(c['xp'][b, 0]).any():
      assert na >= 1, (t, 'q(x) = 0 < p(x): alpha = 1')


def run_case(ops, c, taus=TAUS):
  V, B, k = c['V'], c['B'], c['k']
  rng = np.random.default_rng(V + 7 * B + k)
  for tau in taus:
    for top_k, top_p in FILTERS:
      tag = (V, B, k, tau, top_k, top_p)
      inp = prepare(ops, c, tau, top_k, top_p, rng)
      memo = {}
      special = np.resize(np.array([0.0, R.U_MAX, -1.0, 1.0, 2.0, np.nan, 0.5]), (k, B))
      for ua, ures in ((rng.uniform(0, 1, (k, B)), rng.uniform(0, 1, B)), (special, np.resize(np.array([0.0, R.U_MAX, np.nan, 3.0]), B)),
                       (rng.uniform(0, 1, (k, B)) ** 4, rng.uniform(0, 1, B))):
        check(c, inp, ua, ures, tau, launch(ops, c, inp, ua, ures, tau), tag, memo)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('B', BS)
@pytest.mark.parametrize('V', VS)
def test_spec_verify_vs_fp64_reference(ops, V, B, k):
  run_case(ops, case(V, B, k))
  o = observed
  print(f'spec_verify V={V} B={B} k={k}: so far {o["rows"]} rows judged ({o["accepted"]} accepted), {o["between"]} inside a band using at most '
        f'{o["accept"]:.2e} of d; {o["resid_draws"]} residual draws missing by at most {o["residual"]:.2e} of delta, {o["fallbacks"]} fallbacks; '
        f'|logp - fp64| {o["logp"]:.2e} (allowed {LOGP_TOL:.0e})')


def test_spec_verify_padded_rows_with_nan_in_the_pad(ops):
  run_case(ops, case(1000, 5, 4, padded=1), taus=(0.8,))
  run_case(ops, case(257, 5, 8, padded=1), taus=(0.8,))


@pytest.mark.parametrize('V,B,k', [(1000, 5, 4), (50280, 5, 8)])
def test_two_runs_are_bit_equal_and_sequences_do_not_see_each_other(ops, V, B, k):
  c = case(V, B, k)
  rng = np.random.default_rng(3)
  for tau, (top_k, top_p) in ((0.8, FILTERS[0]), (0.8, FILTERS[1]), (50.0, FILTERS[0])):
    inp = prepare(ops, c, tau, top_k, top_p, rng)
    ua, ures = rng.uniform(0, 1, (k, B)) ** 2, rng.uniform(0, 1, B)
    a = launch(ops, c, inp, ua, ures, tau)
    assert same_bits(a, launch(ops, c, inp, ua, ures, tau)), (tau, top_k)
    # sequence 2 gets other inputs throughout: the other sequences' outputs keep their bits
    c2 = dict(c, dp=c['dp'].clone(), dq=c['dq'].clone())
    c2['dp'].view(B, k + 1, -1)[2] = c['dp'].view(B, k + 1, -1)[0]
    c2['dq'].view(k, B, -1)[:, 2] = c['dq'].view(k, B, -1)[:, 1]
    inp2 = {n: t.clone() for n, t in inp.items()}
    inp2['tok'][:, 2] = inp['tok'][:, 1]
    inp2['pcut'].view(B, k + 1)[2] = inp['pcut'].view(B, k + 1)[0]
    inp2['qcut'][:, 2] = inp['qcut'][:, 1]
    inp2['ptok'].view(B, k + 1)[2] = inp['ptok'].view(B, k + 1)[0]
    ua2, ures2 = ua.copy(), ures.copy()
    ua2[:, 2], ures2[2] = 0.123, 0.987
    other = launch(ops, c2, inp2, ua2, ures2, tau)
    keep = [b for b in range(B) if b != 2]
    assert same_bits(tuple(t[keep] for t in a), tuple(t[keep] for t in other)), (tau, top_k)


def test_spec_verify_refuses_what_the_wrapper_can_see(ops):
  B, k, V = 2, 2, 64
  z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device='cuda')  # noqa: E731
  good = dict(tl=z(B * (k + 1), V, dt=BF16), dl=z(k * B, V, dt=BF16), tok=z(k, B, dt=torch.int64), pc=z(B * (k + 1)), qc=z(k * B),
              pt=z(B * (k + 1), dt=torch.int64), ua=z(k, B), ur=z(B))
  call = lambda **kw: ops.spec_verify(*{**good, **kw}.values())  # noqa: E731
  assert call().n_accept.tolist() == [2, 2]  # equal rows: everything is accepted
  with pytest.raises(ValueError, match='target_logits'):
    call(tl=z(B * k, V, dt=BF16))
  with pytest.raises(ValueError, match='unit inner stride'):
    call(dl=z(V, k * B, dt=BF16).t())
  with pytest.raises(ValueError, match='columns'):
    call(dl=z(k * B, V + 8, dt=BF16))
  with pytest.raises(TypeError):
    call(tok=z(k, B, dt=torch.int32))
  with pytest.raises(ValueError, match='u_resid'):
    call(ur=z(B + 1))
  with pytest.raises(TypeError):
    call(pc=z(B * (k + 1), dt=torch.float64))
  with pytest.raises(RuntimeError, match='temperature'):
    ops.spec_verify(*good.values(), temperature=0.0)
  with pytest.raises(RuntimeError, match='drafted tokens'):
    ops.spec_verify(z(33 * 2, V, dt=BF16), z(32 * 2, V, dt=BF16), z(32, 2, dt=torch.int64), z(66), z(64), z(66, dt=torch.int64), z(32, 2), z(2))


# ---- generate_speculative on the 2-layer golden model ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mdl(golden_dir):
  z = np.load(os.path.join(golden_dir, 'model.npz'))
  return {k: torch.from_numpy(z[k]) for k in z.files}


def _small(P, mdl):
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  m.load_state_dict({k[2:]: v for k, v in mdl.items() if k.startswith('w:')})
  return m.cuda()


@pytest.fixture(scope='module')
def models(ops, mdl):
  """(target, self-draft = the target's own weights in another module, mismatched draft = a 1-layer random model with other heads and
  another MLP class)."""
  import plainlm_amd as P
  torch.manual_seed(5)
  other = P.Transformer(OTHER(P)).cuda()
  return _small(P, mdl), _small(P, mdl), other


T0, N, K = 16, 32, 4


def OTHER(P, **kw):
  return P.ModelConfig(**{**dict(vocab_size=256, seq_len=64, dim=128, expand=2.0, n_layers=1, n_heads=4, mlp='mlp_relu_sq'), **kw})


def _against_the_full_forward(m, prompt, toks, lps, lens=None):
  """generate's criteria (tests/test_decode_gpu.py): every token's logit is within 4 eps of its row's maximum in the full forward, the
  log-probabilities are predict's within eps.  Returns (gap, eps)."""
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


def _wrap_prefill(monkeypatch, *ms):
  caches = {}
  for i, m in enumerate(ms):
    real = m.prefill
    monkeypatch.setattr(m, 'prefill', lambda *a, _r=real, _i=i, **k: caches.setdefault(_i, _r(*a, **k)))
  return caches


def test_greedy_self_draft(models, mdl, monkeypatch):
  m, twin, _ = models
  prompt = mdl['tokens'][:, :T0].cuda()
  with torch.no_grad():
    toks, lps, stats = m.generate_speculative(prompt, N, twin, n_draft=K, return_logprobs=True, return_stats=True)
    assert toks.dtype == torch.int64 and tuple(toks.shape) == (2, N) and lps.dtype == torch.float32 and tuple(lps.shape) == (2, N)
    gap, eps = _against_the_full_forward(m, prompt, toks, lps)
    d, a = stats['drafted'].sum().item(), stats['accepted'].sum().item()
    print(f'greedy, self-draft, k = {K}: {stats["rounds"]} rounds for {N} tokens, {a} of {d} drafted tokens accepted ({a / d:.3f}); worst (row max '
          f'- chosen logit) {gap:.3e} against 4 eps = {4 * eps:.3e}')
    assert stats['rounds'] < N - 1  # something was accepted
    plain = m.generate(prompt, N)
    print(f'                      tokens equal to generate()\'s: {(plain == toks).float().mean().item():.4f}')
    # two calls are bit-equal; the plain result forms are generate's
    t2, l2 = m.generate_speculative(prompt, N, twin, n_draft=K, return_logprobs=True)
    assert torch.equal(t2, toks) and torch.equal(l2.view(torch.int32), lps.view(torch.int32))
    assert torch.equal(m.generate_speculative(prompt, N, twin, n_draft=K), toks)


def test_greedy_mismatched_draft_rollback_and_cache_bits(models, mdl, monkeypatch):
  m, _, other = models
  prompt = mdl['tokens'][:, :T0].cuda()
  caches = _wrap_prefill(monkeypatch, m, other)
  with torch.no_grad():
    toks, lps, stats = m.generate_speculative(prompt, N, other, n_draft=K, return_logprobs=True, return_stats=True)
    monkeypatch.undo()
    gap, eps = _against_the_full_forward(m, prompt, toks, lps)
    d, a = stats['drafted'].sum().item(), stats['accepted'].sum().item()
    print(f'greedy, 1-layer random draft, k = {K}: {stats["rounds"]} rounds, {a} of {d} drafted tokens accepted; gap {gap:.3e} (4 eps {4 * eps:.3e})')
    assert a < d  # it does reject
    tc, dc = caches[0][0], caches[1][0]
    tc.check()
    dc.check()
    # both caches hold the prompt and every generated token but the newest (the draft may still lack the one before it)
    seq = torch.cat([prompt, toks], dim=1)
    assert tc.lens.tolist() == [T0 + N - 1] * 2
    for cache, model in ((tc, m), (dc, other)):
      lens = cache.lens.tolist()
      assert all(n in (T0 + N - 1, T0 + N - 2) for n in lens), lens
      fresh, _ = model.prefill(seq[:, :T0 + N - 1].contiguous())
      for layer in range(len(cache.kv)):
        for b, n in enumerate(lens):
          assert torch.equal(cache.kv[layer][b, :n].view(torch.int16), fresh.kv[layer][b, :n].view(torch.int16)), (layer, b)


def test_ragged_prompts_and_eos(models, mdl):
  m, twin, other = models
  prompt = mdl['tokens'][:, :T0].cuda()
  with torch.no_grad():
    toks, lps = m.generate_speculative(prompt, N, other, n_draft=K, return_logprobs=True)
    lens = (16, 9)
    rt, rl = m.generate_speculative(prompt, N, other, n_draft=K, prompt_lens=lens, return_logprobs=True)
    assert torch.equal(rt[0], toks[0]) and torch.equal(rl[0].view(torch.int32), lps[0].view(torch.int32))  # sequence 0 does not see sequence 1
    _against_the_full_forward(m, prompt, rt, rl, lens)
    for draft in (twin, other):
      base, bl = m.generate_speculative(prompt, N, draft, n_draft=K, return_logprobs=True)
      eos = int(base[0, 5].item())
      te, le, stats = m.generate_speculative(prompt, N, draft, n_draft=K, eos_id=eos, return_logprobs=True, return_stats=True)
      froze = 0
      for b in range(2):
        hit = (base[b] == eos).nonzero()
        n = int(hit[0]) + 1 if len(hit) else N
        froze += N - n
        assert torch.equal(te[b, :n], base[b, :n]) and torch.equal(le[b, :n].view(torch.int32), bl[b, :n].view(torch.int32)), b
        assert (te[b, n:] == eos).all() and (le[b, n:] == 0).all(), b
      assert froze > 0


def test_sampled_is_reproducible_in_the_top_5_and_scores_as_predict(models, mdl):
  m, twin, other = models
  prompt = mdl['tokens'][:, :T0].cuda()
  kw = dict(n_draft=K, temperature=0.8, top_k=5, return_logprobs=True)
  with torch.no_grad():
    for name, draft in (('1-layer random draft', other), ('self-draft', twin)):
      toks, lps, stats = m.generate_speculative(prompt, N, draft, seed=21, return_stats=True, **kw)
      t2, l2 = m.generate_speculative(prompt, N, draft, seed=21, **kw)
      assert torch.equal(t2, toks) and torch.equal(l2.view(torch.int32), lps.view(torch.int32))
      t3, _ = m.generate_speculative(prompt, N, draft, seed=22, **kw)
      assert not torch.equal(t3, toks)
      seq = torch.cat([prompt, toks], dim=1)
      rows = m(seq, None).float()[:, T0 - 1:T0 - 1 + N]
      chosen = rows.gather(2, toks[:, :, None])[:, :, 0]
      gap = (rows.topk(5, dim=-1).values[..., 4] - chosen).max().item()
      want = torch.log_softmax(rows.double(), dim=-1).gather(2, toks[:, :, None])[:, :, 0]
      err = (lps.double() - want).abs().max().item()
      d, a = stats['drafted'].sum().item(), stats['accepted'].sum().item()
      print(f'sampled (0.8 / top-5), {name}: {stats["rounds"]} rounds, {a} of {d} accepted ({a / d:.3f}); worst (5th largest full-forward logit - '
            f'chosen) {gap:.3e} (allowed {LOGIT_TOL}); |logp - log softmax(full forward)| {err:.3e} (allowed {LOGP_MODEL_TOL})')
      assert ((toks >= 0) & (toks < 256)).all() and gap <= LOGIT_TOL and err <= LOGP_MODEL_TOL and (lps <= 0).all()


def test_generate_speculative_refusals_on_the_device(models, mdl):
  import plainlm_amd as P
  m, twin, other = models
  prompt = mdl['tokens'][:, :T0].cuda()
  with pytest.raises(TypeError, match='draft must be'):
    m.generate_speculative(prompt, 8, None)
  with torch.no_grad():
    with pytest.raises(ValueError, match='n_draft'):
      m.generate_speculative(prompt, 8, twin, n_draft=32)
    with pytest.raises(ValueError, match='seq_len'):
      m.generate_speculative(prompt, 44, twin, n_draft=4)  # 16 + 44 + 4 + 1 > 64
    cpu_draft = P.Transformer(OTHER(P))
    with pytest.raises(ValueError, match='the draft is on'):
      m.generate_speculative(prompt, 8, cpu_draft)
    wide = P.Transformer(OTHER(P, vocab_size=264)).cuda()
    with pytest.raises(ValueError, match='vocab_size'):
      m.generate_speculative(prompt, 8, wide)
    with pytest.raises(ValueError, match='top_p'):
      m.generate_speculative(prompt, 8, twin, temperature=0.8, top_p=0.0)
  with pytest.raises(RuntimeError, match='forward-only'):
    m.generate_speculative(prompt, 8, twin)
