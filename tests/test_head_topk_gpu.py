"""Top-k head on MI355X (ops.head_topk, Transformer.predict_topk) against tests/topk_ref.py, the fp64 contract
applied to the bf16 logits ops.gemm_nt stores for the same operands.  tok and rank are compared EXACTLY (ties at the k-th place included:
the large-V cases assert that they have some), logp and lse within ROW = BOUNDS['ce_loss'] = 3e-5 nats, the bound head_predict's row
kernel is held to."""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as R  # noqa: E402
from oracle import parity_ops as PO  # noqa: E402

ROW = PO.BOUNDS['ce_loss']
BF16 = torch.bfloat16
INF, NAN = float('inf'), float('nan')
KS = (1, 5, 64)
# small V; the LDS-resident row at the real vocabulary; a row beyond the LDS budget (ROW_IN_LDS = false); a chunk edge (M = chunk + 3);
# the largest row that is staged in LDS and the smallest that is not
SHAPES = {'small': (5, 1000, 64), 'vocab': (3, 50280, 64), 'wide': (2, 90000, 64), 'chunk': (None, 264, 64),
          'lds-last': (2, 65536, 64), 'lds-past': (2, 65544, 64)}
# seeds chosen on the CPU (fp32 product of the same operands) so that two rows of each large-V case tie at the 64th place, one at the 5th
SEEDS = {'small': 1000, 'vocab': 50280, 'wide': 90003, 'chunk': 264, 'lds-last': 65536, 'lds-past': 65544}


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops
  return ops


@pytest.fixture(scope='module')
def cases(ops):
  """name -> (Y, W, targets, the bf16 logits of gemm_nt on the CPU): made once, never changed."""
  out = {}
  for name, (M, V, K) in SHAPES.items():
    M = ops.head_topk_chunk_rows() + 3 if M is None else M
    g = torch.Generator().manual_seed(SEEDS[name])
    Y = torch.randn(M, K, generator=g).to(BF16).cuda()
    W = torch.randn(V, K, generator=g).to(BF16).cuda()
    t = torch.randint(0, V, (M,), generator=g)
    t[0] = -100
    out[name] = (Y, W, t.cuda(), ops.gemm_nt(Y, W).cpu())
  return out


def _err(got, ref):
  both_ninf = (got.double().cpu() == -INF) & (ref == -INF)
  return torch.where(both_ninf, torch.zeros_like(ref), (got.double().cpu() - ref).abs()).nan_to_num(nan=INF).max().item()


def _check(r, ref, what):
  assert r.tok.dtype == torch.int64 and r.logp.dtype == torch.float32
  assert torch.equal(r.tok.cpu(), ref['tok']), what
  le = _err(r.logp, ref['logp'])
  se = _err(r.lse, ref['lse']) if r.lse is not None else 0.0
  print(f'head_topk {what}: logp err {le:.2e} lse err {se:.2e} (bound {ROW:.1e})')
  assert le <= ROW and se <= ROW, what
  if ref['rank'] is not None:
    assert r.rank.dtype == torch.int32 and torch.equal(r.rank.cpu(), ref['rank']), what


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name', list(SHAPES))
def test_against_the_reference_on_the_gemm_logits(ops, cases, name, k):
  Y, W, t, logits = cases[name]
  ref = R.topk_reference(logits, k, t)
  ties = int(R.kth_place_ties(logits, k).sum())
  print(f'head_topk {name} k={k}: {ties} of {logits.shape[0]} rows have a tie at the k-th place')
  if name in ('vocab', 'wide') and k == 64:
    assert ties >= 1  # exactness covers the index rule, not by luck of the data
  r = ops.head_topk(Y, W, k, t, want_lse=True)
  _check(r, ref, f'{name} k={k}')
  q = ops.head_topk(Y, W, k)  # fewer outputs: the others keep their bits
  assert q.lse is None and q.rank is None and torch.equal(q.tok, r.tok) and torch.equal(q.logp, r.logp)


@pytest.mark.parametrize('k', KS)
def test_planted_rows(ops, k):
  """Y = e_0, W = (the row | 0): Y W^T is exactly the row (one product with 1, sums with 0 * 0; a row per call, since 0 * NaN would reach
  its neighbours).  Every row class, compared exactly (logp and lse within ROW)."""
  V, K = 1000, 64
  g = torch.Generator().manual_seed(k)
  L = torch.randn(9, V, generator=g).to(BF16).float()
  t = torch.randint(0, V, (9,), generator=g)
  L[0, 3:] = NAN                                   # fewer than k finite logits (3, at k > 3)
  L[0, 1] = L[0, 2]
  L[1] = 1.5                                       # all equal
  L[2] = NAN                                       # all NaN
  L[3, 17] = INF                                   # +inf present: absent, not the maximum
  L[3, 500] = -INF
  t[3] = 17                                        # ... and the target: ranks V
  t[4] = -100                                      # ignored target
  t[5] = int((L[5] == L[5].max()).nonzero()[0])    # the target is the maximum (the first of equal ones)
  t[6] = int((L[6] == L[6].min()).nonzero()[-1])   # the target is the minimum (the last of equal ones)
  L[7, :] = 1.0                                    # two values: hundreds of ties above and at the k-th place
  L[7, 2::3] = 2.0
  L[8, V - 8:] = 9.0                               # the k-th place inside the last vector
  ref = R.topk_reference(L, k, t)
  assert ref['rank'].tolist()[2:7] == [V, V, -1, 0, V - 1] and ref['tok'][2].tolist() == [-1] * k
  Y = torch.zeros(1, K, dtype=BF16)
  Y[0, 0] = 1.0
  Y = Y.cuda()
  for i in range(9):
    W = torch.zeros(V, K, dtype=BF16)
    W[:, 0] = L[i].to(BF16)
    W = W.cuda()
    assert torch.equal(ops.gemm_nt(Y, W).cpu()[0].float().nan_to_num(nan=123.), L[i].nan_to_num(nan=123.))
    _check(ops.head_topk(Y, W, k, t[i:i + 1].cuda(), want_lse=True), {key: v[i:i + 1] for key, v in ref.items()}, f'planted row {i} k={k}')


@pytest.mark.parametrize('name', ['small', 'vocab'])
def test_k1_is_head_predict(ops, cases, name):
  Y, W, t, _ = cases[name]
  r, p = ops.head_topk(Y, W, 1, want_lse=True), ops.head_predict(Y, W, want_lse=True)
  assert torch.equal(r.tok[:, 0], p.pred)
  le, se = _err(r.logp[:, 0], p.logp.double().cpu()), _err(r.lse, p.lse.double().cpu())
  print(f'head_topk k=1 vs head_predict {name}: logp {le:.2e} lse {se:.2e}')
  assert le <= ROW and se <= ROW


def test_predict_topk_on_the_golden_model(golden_dir):
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  import plainlm_amd as P
  z = np.load(os.path.join(golden_dir, 'model.npz'))
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')})
  m = m.cuda()
  tok = torch.from_numpy(z['tokens'])
  ids, tgt = tok[:, :64].cuda(), tok[:, 1:65].clone()
  tgt[0, 5] = -100
  tgt = tgt.cuda()
  with torch.no_grad():
    r = m.predict_topk(ids, 5, targets=tgt)
    p = m.predict(ids, targets=tgt)
    logits = m(ids).view(-1, 256)
    last = m.predict_topk(ids, 5, targets=tgt, last_only=True)
  B, T = ids.shape
  assert tuple(r.tokens.shape) == tuple(r.logprobs.shape) == (B, T, 5) and tuple(r.lse.shape) == tuple(r.rank.shape) == (B, T)
  ref = R.topk_reference(logits, 5, tgt.view(-1))
  assert torch.equal(r.tokens.view(-1, 5).cpu(), ref['tok']) and torch.equal(r.rank.view(-1).cpu(), ref['rank'])
  assert _err(r.logprobs.view(-1, 5), ref['logp']) <= 2 * ROW  # the logits come from a second launch of the model, as in predict's test
  assert torch.equal(r.rank == 0, (p.tokens == tgt))
  assert tuple(last.tokens.shape) == (B, 5) and torch.equal(last.tokens, r.tokens[:, -1]) and torch.equal(last.rank, r.rank[:, -1])
  with pytest.raises(RuntimeError, match=r'loss\(\)'):
    m.predict_topk(ids, 5)  # grad enabled, parameters require grad
