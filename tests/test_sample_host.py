"""CPU tests (no GPU) of on-device sampling: tests/sample_ref.py against the customary sort-based top-k / top-p code where no tie sits
on a boundary, and its own tie rule where one does; plm_sample_logits_bf16 refuses bad arguments before any HIP call (the header, the
binding table and the library are compared in tests/test_host_logic.py); and the host logic of generate's sampling arguments
(plainlm_amd/generate.py) with a fake step and a fake sampler."""

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


def _lib_loaded():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def customary(x, u, tau, top_k, top_p):
  """The usual sort-based code on one fp64 row: (kept mask, token).  top-k through `scores < topk[-1]`, nucleus through a descending
  sort and a cumulative softmax (a token stays while the mass BEFORE it is below top_p), the draw by inverting the CDF in index order."""
  z = torch.from_numpy(x) / tau
  if 0 < top_k < z.numel():
    z = z.masked_fill(z < torch.topk(z, top_k).values[-1], -float('inf'))
  if top_p < 1:
    sz, idx = torch.sort(z, descending=True)
    pr = torch.softmax(sz, dim=-1)
    before = torch.cumsum(pr, dim=-1) - pr
    drop = torch.zeros_like(z, dtype=torch.bool).scatter(0, idx, before >= top_p)
    z = z.masked_fill(drop, -float('inf'))
  pr = torch.softmax(z, dim=-1)
  cdf = torch.cumsum(pr, dim=-1)
  tok = int(torch.searchsorted(cdf, torch.tensor(float(u) * float(cdf[-1]), dtype=torch.float64), right=True))
  return (z > -float('inf')).numpy(), tok


def distinct_rows(B, V, seed):
  """fp64 rows of distinct values (a permutation of a jittered ramp): no tie anywhere, so no boundary can hold one."""
  rng = np.random.default_rng(seed)
  base = np.linspace(-6.0, 6.0, V) + rng.uniform(-0.4, 0.4, V) * (12.0 / V)
  return np.stack([rng.permutation(base) for _ in range(B)])


@pytest.mark.parametrize('tau', [0.5, 1.0, 3.0])
@pytest.mark.parametrize('top_k,top_p', [(0, 1.0), (1, 1.0), (17, 1.0), (0, 0.9), (17, 0.95), (0, 0.3), (400, 0.5)])
def test_reference_is_the_customary_code_where_no_tie_sits_on_a_boundary(tau, top_k, top_p):
  B, V = 6, 300
  x = distinct_rows(B, V, 7)
  u = np.random.default_rng(1).uniform(0, 1, B)
  u[0], u[1] = 0.0, R.U_MAX
  got = R.sample(x, u, tau, top_k, top_p)
  for b in range(B):
    keep, tok = customary(x[b], u[b], tau, top_k, top_p)
    assert np.array_equal(got['keep'][b], keep), (b, got['n_kept'][b], keep.sum())
    assert got['tok'][b] == tok, b
    assert got['cutoff'][b] == x[b][keep].min() and got['n_kept'][b] == keep.sum()
  if top_k == 17 and top_p == 1.0:
    assert (got['n_kept'] == 17).all()


def test_reference_keeps_whole_tie_classes():
  V = 200
  x = distinct_rows(1, V, 3)[0]
  order = np.argsort(-x)
  # top-k: the 10th .. 14th largest share one value: k = 10, 11 .. 14 all keep 14; k = 9 keeps 9
  xk = x.copy()
  xk[order[9:14]] = x[order[9]]
  for k, want in ((9, 9), (10, 14), (12, 14), (14, 14), (15, 15)):
    ks = R.Rows(xk[None]).keep_set(1.0, k, 1.0)
    assert ks['n_kept'][0] == want and ks['cutoff'][0] == xk[order[want - 1]], (k, ks['n_kept'][0])
    assert np.array_equal(np.flatnonzero(ks['keep'][0]), np.sort(order[:want]))
  # top-p: two columns tie at the top with 0.4 of the mass each; any top_p in (0, 0.8] keeps both, never one of them
  xp = np.full(V, -30.0)
  xp[[5, 150]] = 2.0
  xp[77] = 2.0 + np.log(0.25)  # 0.1 of the mass
  xp[3] = 2.0 + np.log(0.25)
  r = R.Rows(xp[None])
  for p, want in ((0.05, [5, 150]), (0.4, [5, 150]), (0.79, [5, 150]), (0.81, [3, 5, 77, 150]), (0.999, [3, 5, 77, 150])):
    ks = r.keep_set(1.0, 0, p)
    assert np.flatnonzero(ks['keep'][0]).tolist() == want, (p, np.flatnonzero(ks['keep'][0]))
  assert r.keep_set(1.0, 0, 1.0)['n_kept'][0] == V
  # an all-equal row: every filter keeps all V; the draw walks the columns in index order
  xe = np.full((1, V), 1.25)
  for k, p in ((0, 1.0), (1, 1.0), (50, 0.95), (0, 0.01)):
    assert R.Rows(xe).keep_set(0.7, k, p)['n_kept'][0] == V
  assert R.sample(xe, [0.0], 1.0)['tok'][0] == 0 and R.sample(xe, [R.U_MAX], 1.0)['tok'][0] == V - 1
  assert R.sample(xe, [0.5 + 0.25 / V], 1.0)['tok'][0] == V // 2


def test_reference_top_k_1_is_the_argmax_and_non_finite_logits_never_count():
  x = distinct_rows(4, 97, 11)
  for u in (0.0, 0.3, R.U_MAX, 5.0, -2.0, float('nan')):
    for tau in (0.05, 1.0, 50.0):
      got = R.sample(x, np.full(4, u), tau, 1, 1.0)
      assert np.array_equal(got['tok'], x.argmax(1)) and (got['n_kept'] == 1).all()
  # NaN and -inf: weight 0, never kept, never chosen; logp is over the finite logits
  y = x.copy()
  y[0, :50] = np.nan
  y[1, ::2] = -np.inf
  y[2, :] = np.nan
  got = R.sample(y, np.array([0.0, R.U_MAX, 0.5, 0.5]), 1.0, 0, 1.0)
  assert got['n_kept'].tolist() == [47, 48, 0, 97] and got['tok'][0] >= 50 and got['tok'][1] % 2 == 1
  assert got['tok'][2] == 0 and np.isnan(got['logp'][2]) and np.isnan(got['cutoff'][2])
  want = torch.log_softmax(torch.from_numpy(np.where(np.isfinite(y[1]), y[1], -np.inf)), -1)[got['tok'][1]].item()
  assert abs(got['logp'][1] - want) < 1e-12
  # the clamp of u
  assert np.array_equal(R.clamp_u([-1.0, float('nan'), 1.0, 2.0, 0.25]), [0.0, 0.0, R.U_MAX, R.U_MAX, 0.25])


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
p = lambda: C.c_void_p(0x100000)  # noqa: E731  plausible, never dereferenced


def test_sample_logits_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()

  def refused(*args):
    rc = lib.plm_sample_logits_bf16(*args)
    msg = (lib.plm_last_error_string() or b'').decode()
    assert rc == -1 and 'plm_sample_logits_bf16' in msg, (rc, msg)  # PLM_E_INVALID
    return msg
  # logits, ld, u, temperature, top_k, top_p, tok, logp, n_kept, cutoff, B, V, stream
  ok = [p(), 1000, p(), 0.8, 50, 0.95, p(), p(), None, None, 4, 1000, None]
  for i in (0, 2, 6, 7):  # every pointer but n_kept and cutoff
    a = list(ok)
    a[i] = None
    assert 'null pointer' in refused(*a), i
  for i, v in ((10, 0), (10, -3), (11, 0), (11, -1), (11, 1 << 31), (1, 999), (1, 0)):  # B < 1, V < 1, V too large, ld < V
    a = list(ok)
    a[i] = v
    if i == 11 and v > 1000:
      a[1] = v
    assert 'bad shape' in refused(*a), (i, v)
  a = list(ok)
  a[0] = C.c_void_p(0x100001)
  assert '2-byte aligned' in refused(*a)
  for t in (0.0, -1.0, float('inf'), float('nan')):
    a = list(ok)
    a[3] = t
    assert 'temperature' in refused(*a), t
  a = list(ok)
  a[4] = -1
  assert 'top_k' in refused(*a)
  for tp in (0.0, -0.5, 1.0001, float('nan')):
    a = list(ok)
    a[5] = tp
    assert 'top_p' in refused(*a), tp


# ---- generate's sampling arguments -----------------------------------------------------------------------------------------------------
def test_check_sampling_normalises_and_refuses():
  cs = G.check_sampling
  for t in (None, 0, 0.0):  # greedy: the fused prediction head
    assert cs(t, None, None, None, None) is None
    assert cs(t, 0, 1.0, None, 123) is None
    assert cs(t, None, 1, None, None) is None
  assert cs() is None
  assert cs(0.8, None, None) == (0.8, 0, 1.0)
  assert cs(0.8, 50, 0.95, None, 7) == (0.8, 50, 0.95)
  assert cs(None, 50, None) == (1.0, 50, 1.0) and cs(None, None, 0.9) == (1.0, 0, 0.9)
  assert cs(1, 1) == (1.0, 1, 1.0) and isinstance(cs(1, 1)[0], float) and isinstance(cs(2.0, 3.0)[1], int)
  fn = lambda lf: lf.argmax(-1)  # noqa: E731
  assert cs(None, None, None, fn, None) is None
  for kw in (dict(temperature=0.8), dict(top_k=5), dict(top_p=0.9), dict(seed=3), dict(temperature=0), dict(temperature=1.0, top_k=5, seed=1)):
    with pytest.raises(ValueError, match='sample='):
      cs(sample=fn, **kw)
  for t in (-0.5, -1, float('nan'), float('inf')):
    with pytest.raises(ValueError, match='temperature'):
      cs(t)
  for kw in (dict(top_k=5), dict(top_p=0.9)):
    with pytest.raises(ValueError, match='temperature 0 is greedy'):
      cs(0, **kw)
  with pytest.raises(ValueError, match='top_k'):
    cs(1.0, -1)
  for tp in (0, 0.0, -0.1, 1.5, float('nan')):
    with pytest.raises(ValueError, match='top_p'):
      cs(1.0, 0, tp)


def test_draw_uniforms_once_per_call_and_reproducible_under_a_seed():
  u = G.draw_uniforms(9, 3, 'cpu', seed=5)
  assert u.dtype == torch.float32 and tuple(u.shape) == (9, 3) and u.is_contiguous() and (u >= 0).all() and (u < 1).all()
  assert torch.equal(u, G.draw_uniforms(9, 3, 'cpu', seed=5)) and not torch.equal(u, G.draw_uniforms(9, 3, 'cpu', seed=6))
  torch.manual_seed(11)
  a = G.draw_uniforms(4, 2, 'cpu')  # seed=None: torch's default generator
  torch.manual_seed(11)
  assert torch.equal(a, torch.rand(4, 2))
  assert u[2].is_contiguous() and tuple(u[2].shape) == (3,)  # step n hands row n to the kernel as it is


def test_step_n_consumes_row_n_of_u_and_eos_freezing_still_holds():
  V, N = 11, 9
  u = G.draw_uniforms(N, 3, 'cpu', seed=1)
  seen = []

  def sampler(logits, un, temperature, top_k, top_p):  # stands in for ops.sample_logits: the token is the logits row's first entry
    seen.append((un.clone(), temperature, top_k, top_p))
    return logits[:, 0].long(), -(logits[:, 0] + 1.0), None, None
  pick = G.sampling_pick(u, 0.8, 50, 0.95, sampler=sampler)

  def step(tok):  # a fake decode step: "logits" whose first entry is the next token of the chain t -> 3 t + 1 mod V
    return torch.stack([((tok * 3 + 1) % V).float()] * 4, dim=1)
  first = pick(torch.tensor([[2.0] * 4, [5.0] * 4, [4.0] * 4]))
  toks, lps = G.generate_loop(first, lambda t: pick(step(t)), N)
  assert len(seen) == N and all(torch.equal(s[0], u[n]) and s[1:] == (0.8, 50, 0.95) for n, s in enumerate(seen))
  want = [2]
  for _ in range(N - 1):
    want.append((want[-1] * 3 + 1) % V)
  assert toks[0].tolist() == want and lps[0, 1].item() == -(want[1] + 1.0)
  # eos = 4: sequence 0 (2, 7, 0, 1, 4, ...) emits it at index 4 and is frozen from there; every step still consumes its row of u
  seen.clear()
  pick = G.sampling_pick(u, 0.8, 50, 0.95, sampler=sampler)
  first = pick(torch.tensor([[2.0] * 4, [5.0] * 4, [4.0] * 4]))
  te, le = G.generate_loop(first, lambda t: pick(step(t)), N, eos_id=4)
  assert te[0].tolist() == want[:5] + [4] * 4 and (le[0, 5:] == 0).all() and torch.equal(le[0, :5], lps[0, :5])
  assert torch.equal(te[1], toks[1]) and te[2].tolist() == [4] * N and (le[2, 1:] == 0).all()
  assert len(seen) == N and all(torch.equal(s[0], u[n]) for n, s in enumerate(seen))


def test_generate_refuses_mixed_sampling_arguments_before_any_launch_and_ops_has_no_cpu_path():
  EC = dict(model='transformer', vocab_size=512, seq_len=128, d_model=128, expand='8/3', n_layers=2, n_heads=2, mlp_class='glu',
            tie_embeddings=False)
  model, _ = P.construct_model(namedtuple('Config', EC.keys())(**EC))
  ids = torch.zeros(1, 16, dtype=torch.int64)
  with pytest.raises(RuntimeError, match='MI355X'):  # the device check still comes first
    model.generate(ids, 8, temperature=0.8, top_k=5, seed=0)
  from plainlm_amd import ops
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.sample_logits(torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(2))
  assert ops.SampleLogits._fields == ('tokens', 'logprob', 'n_kept', 'cutoff')
  import inspect
  names = list(inspect.signature(model.generate).parameters)
  assert names == ['prompt', 'max_new_tokens', 'prompt_lens', 'eos_id', 'sample', 'return_logprobs', 'temperature', 'top_k', 'top_p', 'seed']
