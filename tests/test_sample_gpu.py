"""On-device sampling on a real MI355X: plm_sample_logits_bf16 against the fp64 restatement of its rule (tests/sample_ref.py) - the kept
set, the draw, the log-probability, determinism and row independence - and Transformer.generate with temperature / top_k / top_p / seed
on the 2-layer golden model.

Bounds (derived, not measured; the observed figures are printed and recorded in DESIGN.md section 13):
  keep set   top_p = 1: (n_kept, cutoff) equal the reference exactly.  top_p < 1: they equal the reference's answer for some p' in
             [top_p - 1e-5, top_p + 1e-5]: an fp32 tree sum of up to 2^17 positive terms carries about 20 roundings of 2^-24, 1.2e-6,
             the device exp a few ulp more; the slack is 2x on top.
  draw       with the kernel's own (verified) cutoff and the fp64 running sums C over that set: the token is kept, has w > 0 and
             C_prev(tok) - d Z <= u Z <= C_tok + d Z with d = 4e-6 (same derivation; a sequential fp32 scan fails it by design).
  logp       within 3e-5 nats of the fp64 log softmax(x)[tok] (the bound the head-prediction tests hold logp to)."""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_ref as R  # noqa: E402

BF16 = torch.bfloat16
P_SLACK, DRAW_DELTA, LOGP_TOL = 1e-5, 4e-6, 3e-5
TAUS = (0.05, 0.8, 50.0)
FILTERS = ((0, 1.0), (1, 1.0), (50, 1.0), (0, 0.9), (50, 0.95), ('V+5', 0.5))
# every V with every B; 65544 is above any 16-bit count or index; 7 and 257 leave every row but the first unaligned; the last three once
# more with ld = V + 13 and NaN in the pad.  The largest batch is 33 x 65544 elements.
SHAPES = [(V, B, 0) for V in (1, 7, 255, 256, 257, 1000, 50280, 65544) for B in (1, 5, 33)] + [(257, 5, 1), (1000, 33, 1), (50280, 5, 1)]
observed = {'p_slack': 0.0, 'draw': 0.0, 'logp': 0.0}


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


# ---- rows ------------------------------------------------------------------------------------------------------------------------------
def _rand(g, V, scale):
  return torch.randn(V, generator=g) * scale


def row_of(kind, V, g):
  """One fp32 row [V] of the named class (rounded to bf16 by the caller)."""
  if kind == 'rand1':
    return _rand(g, V, 1.0)
  if kind == 'rand8':
    return _rand(g, V, 8.0)
  if kind == 'equal':
    return torch.full((V,), 1.25)
  if kind == 'dominant':
    x = _rand(g, V, 1.0)
    x[int(torch.randint(V, (1,), generator=g))] = 40.0
    return x
  if kind == 'twolevel':  # two values, the upper one on a third of the columns
    x = torch.full((V,), -1.5)
    x[torch.randperm(V, generator=g)[:max(1, V // 3)]] = 2.0
    return x
  if kind == 'tie40':     # 30 distinct values on top, then one value on 40 columns (the 50th largest is among them), the rest below
    x = -3.0 - torch.rand(V, generator=g)
    perm = torch.randperm(V, generator=g)
    top = min(30, V // 3)
    x[perm[:top]] = 4.0 + torch.arange(top) * 0.0625
    x[perm[top:top + min(40, V // 2)]] = 1.0
    return x
  if kind == 'nonfinite':  # -inf and NaN entries among random ones
    x = _rand(g, V, 2.0)
    perm = torch.randperm(V, generator=g)
    x[perm[:V // 4]] = float('-inf')
    x[perm[V // 4:V // 4 + max(1, V // 5)]] = float('nan')
    return x
  if kind == 'allnan':
    return torch.full((V,), float('nan'))
  if kind == 'asc':
    return torch.linspace(-4.0, 4.0, V)
  if kind == 'desc':
    return torch.linspace(4.0, -4.0, V)
  if kind == 'zeros':      # +0 and -0 are one value class; small values of both signs around them
    x = torch.zeros(V)
    x[1::2] = -0.0
    x[::5] = _rand(g, V, 0.01)[::5]
    return x
  raise KeyError(kind)


KINDS = ('rand1', 'tie40', 'nonfinite', 'twolevel', 'allnan', 'rand8', 'equal', 'dominant', 'asc', 'desc', 'zeros')
_cases = {}


def case(V, B, padded=0):
  """bf16 rows [B, V] (row b is of class KINDS[(b + V) % 11], so that the single-row batches differ in class), their fp64 reference
  rows - sorted once, shared by every test that uses the shape, never modified - and the device tensor (with ld = V + 13 and NaN in
  the pad when padded)."""
  key = (V, B, padded)
  if key not in _cases:
    g = torch.Generator().manual_seed(1000 * V + B)
    kinds = [KINDS[(b + V) % len(KINDS)] for b in range(B)]
    xb = torch.stack([row_of(k, V, g) for k in kinds]).to(BF16)
    if padded:
      buf = torch.full((B, V + 13), float('nan'), dtype=BF16, device='cuda')
      dev = buf[:, :V]
      dev.copy_(xb)
    else:
      dev = xb.cuda()
    _cases[key] = dict(V=V, B=B, kinds=kinds, xb=xb, rows=R.Rows(xb.double().numpy()), dev=dev)
  return _cases[key]


def launch(ops, c, u, tau, k, p, dev=None):
  r = ops.sample_logits(c['dev'] if dev is None else dev, torch.as_tensor(np.asarray(u, dtype=np.float32)).cuda(), tau, k, p, want_stats=True)
  return tuple(t.cpu().numpy() for t in r)


def same_bits(a, b):
  return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ---- checks ----------------------------------------------------------------------------------------------------------------------------
def check_keep(c, tau, k, p, w, n_kept, cutoff, tag):
  """(n_kept, cutoff) against the reference; returns the kernel's kept set [B, V] (from its cutoff) for the draw check."""
  rows = c['rows']
  B = rows.B
  ks = rows.keep_set(tau, k, p, w=w)
  if p >= 1:
    assert np.array_equal(n_kept, ks['n_kept']), (tag, n_kept, ks['n_kept'])
    assert np.array_equal(cutoff, ks['cutoff'], equal_nan=True), (tag, cutoff, ks['cutoff'])
    return ks['keep']
  small = rows.keep_set(tau, k, p - P_SLACK, w=w)                                 # the higher cutoff
  large = rows.keep_set(tau, k, p + P_SLACK if p + P_SLACK < 1 else 1.0, w=w)     # the lower cutoff
  empty = rows.nvalid == 0
  assert np.array_equal(np.isnan(cutoff), empty) and (n_kept[empty] == 0).all(), (tag, cutoff, n_kept)
  ok = ~empty
  assert (cutoff[ok] <= small['cutoff'][ok]).all() and (cutoff[ok] >= large['cutoff'][ok]).all(), \
      (tag, cutoff, small['cutoff'], large['cutoff'], ks['cutoff'])
  with np.errstate(invalid='ignore'):
    keep = ks['surv'] & (rows.x >= cutoff[:, None])
    present = (ks['surv'] & (rows.x == cutoff[:, None])).any(1)
  assert present[ok].all(), (tag, 'the cutoff is not a value of the row')
  assert np.array_equal(n_kept, keep.sum(1)), (tag, n_kept, keep.sum(1))
  # the slack this row needed: how far top_p has to move for the reference to give the kernel's answer (0 when they agree)
  off = ok & (cutoff != ks['cutoff'])
  if off.any():
    wk = np.where(ks['surv'], w, 0.0)
    with np.errstate(invalid='ignore'):
      mass_at = np.where(keep, wk, 0.0).sum(1) / wk.sum(1)        # mass(t) of the kernel's cutoff
      mass_ref = np.where(ks['keep'], wk, 0.0).sum(1) / wk.sum(1)
    need = np.where(off, np.minimum(np.abs(mass_at - p), np.abs(mass_ref - p)), 0.0).max()
    observed['p_slack'] = max(observed['p_slack'], float(need))
  return keep


def check_draw(c, keep, w, C, u, tok, logp, tag, exact=None):
  rows = c['rows']
  B, V = rows.B, rows.V
  ar = np.arange(B)
  assert tok.dtype == np.int64 and ((tok >= 0) & (tok < V)).all(), (tag, tok)
  empty = rows.nvalid == 0
  assert (tok[empty] == 0).all() and np.isnan(logp[empty]).all(), (tag, tok, logp)
  ok = ~empty
  assert keep[ar, tok][ok].all(), (tag, 'a token outside the kept set', tok)
  assert (w[ar, tok][ok] > 0).all(), (tag, 'a token of weight 0')
  Z = C[:, -1]
  uz = R.clamp_u(u) * Z
  hi = C[ar, tok]
  lo = hi - np.where(keep[ar, tok], w[ar, tok], 0.0)
  with np.errstate(invalid='ignore', divide='ignore'):
    miss = np.where(ok, np.maximum(lo - uz, uz - hi) / Z, 0.0)
  observed['draw'] = max(observed['draw'], float(miss.max()))
  assert (miss <= DRAW_DELTA).all(), (tag, miss.max(), tok, u)
  if exact is not None:
    sel = ok & exact
    assert np.array_equal(tok[sel], R.draw(keep, w, C, u)[sel]), (tag, 'planted u inside an interval wider than 1e-3')
  err = np.abs(logp[ok].astype(np.float64) - rows.logp[ar, tok][ok])
  if err.size:
    observed['logp'] = max(observed['logp'], float(err.max()))
    assert (err <= LOGP_TOL).all(), (tag, err.max())


@pytest.mark.parametrize('tau', TAUS)
@pytest.mark.parametrize('V,B,padded', SHAPES)
def test_sample_logits_vs_fp64_reference(ops, V, B, padded, tau):
  c = case(V, B, padded)
  rows = c['rows']
  w = rows.weights(tau)
  rng = np.random.default_rng(V + B)
  for k, p in FILTERS:
    k = V + 5 if k == 'V+5' else k
    tag = (V, B, padded, tau, k, p)
    base = launch(ops, c, np.zeros(B), tau, k, p)
    keep = check_keep(c, tau, k, p, w, base[2], base[3], tag)
    C = rows.running(keep, w)
    Z = C[:, -1]
    n = keep.sum(1)
    us = [(np.zeros(B), None), (np.full(B, R.U_MAX), None), (np.resize(np.array([-1.0, 1.0, 2.0, np.nan]), B), None),
          (rng.uniform(0, 1, B), None)]
    # rows with at most 8 kept tokens: u at the midpoint of every kept interval (each wider than 1e-3 of Z: the token must be exact)
    few = (n >= 1) & (n <= 8)
    if few.any():
      for j in range(int(n[few].max())):
        u, exact = rng.uniform(0, 1, B), np.zeros(B, dtype=bool)
        for b in np.flatnonzero(few & (n > j)):
          i = np.flatnonzero(keep[b])[j]
          if w[b, i] / Z[b] > 1e-3:
            u[b] = (C[b, i] - 0.5 * w[b, i]) / Z[b]
            exact[b] = True
        us.append((u, exact))
    for u, exact in us:
      got = launch(ops, c, u, tau, k, p)
      assert same_bits(got[2:], base[2:]), (tag, 'the kept set depends on u')
      check_draw(c, keep, w, C, u, got[0], got[1], tag, exact)
  print(f'sample V={V} B={B} tau={tau}: worst so far: top_p slack {observed["p_slack"]:.2e} (allowed {P_SLACK:.0e}), draw miss '
        f'{observed["draw"]:.2e} of Z (allowed {DRAW_DELTA:.0e}), |logp - fp64| {observed["logp"]:.2e} (allowed {LOGP_TOL:.0e})')


class Tiled:
  """One reference row seen as a batch of n equal rows (what check_draw reads of a Rows)."""

  def __init__(self, r, n):
    self.B, self.V, self.nvalid, self.logp = n, r.V, np.repeat(r.nvalid, n), np.broadcast_to(r.logp, (n, r.V))


@pytest.mark.parametrize('V', [257, 1000])
def test_256_ascending_u_per_row_class_draw_bound_and_monotone_rank(ops, V):
  """Every row class 256 times in one batch (rows are independent), u ascending: the draw bound holds for each u and the chosen token's
  rank in kept-index order never decreases."""
  n = 256
  u = np.sort(np.random.default_rng(V).uniform(0, 1, n))
  g = torch.Generator().manual_seed(V)
  for kind in KINDS:
    xb = row_of(kind, V, g).to(BF16)
    c1 = dict(rows=R.Rows(xb.double().numpy()[None]), dev=xb[None].repeat(n, 1).cuda())
    tiled = dict(rows=Tiled(c1['rows'], n))
    for tau in TAUS:
      w = c1['rows'].weights(tau)
      for k, p in FILTERS:
        k = V + 5 if k == 'V+5' else k
        tag = (kind, V, tau, k, p)
        got = launch(ops, c1, u, tau, k, p)
        assert (got[2] == got[2][0]).all() and np.array_equal(got[3], np.full(n, got[3][0]), equal_nan=True), tag
        keep = check_keep(c1, tau, k, p, w, got[2][:1], got[3][:1], tag)
        C = c1['rows'].running(keep, w)
        check_draw(tiled, np.broadcast_to(keep, (n, V)), np.broadcast_to(w, (n, V)), np.broadcast_to(C, (n, V)), u, got[0], got[1], tag)
        assert (np.diff(got[0]) >= 0).all(), (tag, 'the token went back as u went up')  # index order = rank order within one kept set


@pytest.mark.parametrize('V,B,padded', [(1000, 33, 0), (1000, 33, 1), (50280, 5, 0), (65544, 33, 0)])
def test_two_runs_are_bit_equal_and_rows_do_not_see_each_other(ops, V, B, padded):
  c = case(V, B, padded)
  rng = np.random.default_rng(B)
  u = rng.uniform(0, 1, B)
  perm = rng.permutation(B)
  dev_perm = c['dev'][torch.as_tensor(perm).cuda()].contiguous()
  for tau, k, p in ((0.8, 50, 0.95), (1.0, 0, 1.0), (0.05, 0, 0.9), (50.0, 1, 1.0)):
    a = launch(ops, c, u, tau, k, p)
    assert same_bits(a, launch(ops, c, u, tau, k, p)), (tau, k, p)
    pa = launch(ops, c, u[perm], tau, k, p, dev=dev_perm)
    assert same_bits(pa, tuple(t[perm] for t in a)), (tau, k, p)
    one = launch(ops, c, u[B // 2:B // 2 + 1], tau, k, p, dev=c['dev'][B // 2:B // 2 + 1])  # a row alone: what it gives inside the batch
    assert same_bits(one, tuple(t[B // 2:B // 2 + 1] for t in a)), (tau, k, p)
  # without the statistics: the same tokens
  r = ops.sample_logits(c['dev'], torch.as_tensor(u.astype(np.float32)).cuda(), 0.8, 50, 0.95)
  assert r.n_kept is None and r.cutoff is None
  a = launch(ops, c, u, 0.8, 50, 0.95)
  assert np.array_equal(r.tokens.cpu().numpy(), a[0]) and same_bits((r.logprob.cpu().numpy(),), (a[1],))


def test_sample_logits_refuses_what_the_wrapper_can_see(ops):
  x = torch.zeros(4, 64, dtype=BF16, device='cuda')
  u = torch.zeros(4, device='cuda')
  with pytest.raises(ValueError, match='does not fit'):
    ops.sample_logits(x, u[:3].contiguous())
  with pytest.raises(ValueError, match='unit inner stride'):
    ops.sample_logits(x.t(), u)
  with pytest.raises(TypeError):
    ops.sample_logits(x, u.double())
  for kw, word in ((dict(temperature=0.0), 'temperature'), (dict(top_k=-1), 'top_k'), (dict(top_p=0.0), 'top_p'), (dict(top_p=1.5), 'top_p')):
    with pytest.raises(RuntimeError, match=word):
      ops.sample_logits(x, u, **kw)


# ---- generate on the 2-layer golden model ------------------------------------------------------------------------------------------------
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


N = 32
LOGIT_TOL = 7.8e-2  # the cached-vs-full allowance of the greedy generate test: 4 bf16 eps of this model's logits
LOGP_MODEL_TOL = 2e-2


def _prompt4(mdl):
  t = mdl['tokens']
  return torch.cat([t[:, :16], t[:, 16:32]], dim=0).cuda()  # 4 sequences


def _full_rows(m, prompt, toks):
  """fp32 full-forward logits [B, N, V] of the rows that predict the generated tokens."""
  seq = torch.cat([prompt, toks], dim=1)
  T0 = prompt.shape[1]
  return m(seq, None).float()[:, T0 - 1:T0 - 1 + toks.shape[1]]


def test_generate_top_k_1_is_greedy_where_the_top_2_margin_is_not_zero(model, mdl):
  prompt = _prompt4(mdl)
  with torch.no_grad():
    toks, lps = model.generate(prompt, N, return_logprobs=True)
    ts, ls = model.generate(prompt, N, temperature=1, top_k=1, seed=3, return_logprobs=True)
    assert ts.dtype == torch.int64 and tuple(ts.shape) == (4, N) and ls.dtype == torch.float32 and tuple(ls.shape) == (4, N)
    top = _full_rows(model, prompt, toks).topk(2, dim=-1).values
    clear = (top[..., 0] - top[..., 1]) != 0
    # a tie at the top may go either way, and what follows it is another sequence: compare up to the first tie of every sequence
    upto = torch.where(clear.all(1), N, (~clear).int().argmax(1))
    compared = 0
    for b in range(4):
      n = int(upto[b])
      compared += n
      assert torch.equal(ts[b, :n], toks[b, :n]), b
      assert (ls[b, :n] - lps[b, :n]).abs().max().item() <= LOGP_MODEL_TOL if n else True
    print(f'top_k = 1 against greedy: {compared} of {4 * N} positions before the first top-2 tie of their sequence')
    assert compared > 2 * N


def test_generate_is_bit_reproducible_under_a_seed_and_seeds_differ(model, mdl):
  prompt = _prompt4(mdl)
  with torch.no_grad():
    a = model.generate(prompt, N, temperature=1.0, seed=11, return_logprobs=True)
    b = model.generate(prompt, N, temperature=1.0, seed=11, return_logprobs=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    c = model.generate(prompt, N, temperature=1.0, seed=12)
    assert not torch.equal(a[0], c)
    assert torch.equal(model.generate(prompt, N, temperature=1.0, seed=11), a[0])
    # seed=None: torch's default generator
    torch.manual_seed(5)
    d = model.generate(prompt, N, temperature=1.0)
    torch.manual_seed(5)
    assert torch.equal(model.generate(prompt, N, temperature=1.0), d)


def test_generate_top_k_5_tokens_and_log_probabilities_against_the_full_forward(model, mdl):
  prompt = _prompt4(mdl)
  with torch.no_grad():
    toks, lps = model.generate(prompt, N, temperature=1.0, top_k=5, seed=21, return_logprobs=True)
    rows = _full_rows(model, prompt, toks)
    chosen = rows.gather(2, toks[:, :, None])[:, :, 0]
    fifth = rows.topk(5, dim=-1).values[..., 4]
    gap = (fifth - chosen).max().item()
    want = torch.log_softmax(rows.double(), dim=-1).gather(2, toks[:, :, None])[:, :, 0]
    err = (lps.double() - want).abs().max().item()
    print(f'top_k = 5: worst (5th largest full-forward logit - chosen logit) {gap:.3e} (allowed {LOGIT_TOL}); '
          f'|logp - log softmax(full forward)| {err:.3e} (allowed {LOGP_MODEL_TOL}); distinct tokens {toks.unique().numel()}')
    assert gap <= LOGIT_TOL
    assert err <= LOGP_MODEL_TOL and (lps <= 0).all()
    assert (toks != model.generate(prompt, N)).any()  # it does sample
    # nucleus and temperature together run too, and every token is in range
    t2 = model.generate(prompt, N, temperature=0.8, top_k=50, top_p=0.95, seed=1)
    assert ((t2 >= 0) & (t2 < 256)).all()


def test_generate_sampling_with_ragged_prompts_eos_and_refusals(model, mdl):
  prompt = mdl['tokens'][:, :16].cuda()
  kw = dict(temperature=1.0, top_k=5, seed=4)
  with torch.no_grad():
    toks, lps = model.generate(prompt, N, return_logprobs=True, **kw)
    ragged = model.generate(prompt, 8, prompt_lens=(16, 9), **kw)
    assert torch.equal(ragged[0], toks[0, :8])  # sequence 0 sees neither what sequence 1 holds nor another uniform
    eos = int(toks[0, 5].item())
    te, le = model.generate(prompt, N, eos_id=eos, return_logprobs=True, **kw)
    froze = 0
    for b in range(2):
      hit = (toks[b] == eos).nonzero()
      n = int(hit[0]) + 1 if len(hit) else N
      froze += N - n
      assert torch.equal(te[b, :n], toks[b, :n]) and torch.equal(le[b, :n], lps[b, :n]), b
      assert (te[b, n:] == eos).all() and (le[b, n:] == 0).all(), b
    assert froze > 0
    with pytest.raises(ValueError, match='sample='):
      model.generate(prompt, 4, sample=lambda lf: lf.argmax(-1), temperature=0.8)
    with pytest.raises(ValueError, match='top_p'):
      model.generate(prompt, 4, temperature=0.8, top_p=0.0)
    # temperature None / 0 stay on the fused greedy head: no logits are built
    from plainlm_amd import ops as O
    calls = []
    real = O.sample_logits
    O.sample_logits = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
      g0 = model.generate(prompt, 8)
      assert torch.equal(model.generate(prompt, 8, temperature=0), g0) and torch.equal(model.generate(prompt, 8, temperature=None, seed=3), g0)
      assert calls == []
      model.generate(prompt, 8, **kw)
      assert len(calls) == 8  # one sampling launch per token
    finally:
      O.sample_logits = real
