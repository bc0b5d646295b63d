"""Prediction head on MI355X (ops.head_predict, Transformer.predict, HipEngine.eval_metrics): argmax, its log-probability and the
entropy of softmax(bf16(Y W^T)) without the logits buffer.

pred is compared EXACTLY, against the explicit first-index argmax (tests/predict_ref.py) of the logits plm_gemm_bf16_nt stores.
logp and entropy are compared with their fp64 definitions on those bf16 logits within ROW = BOUNDS['ce_loss'] (oracle/parity_ops.py,
3e-5 nats - the bound the per-row losses have; a plain fp32 restatement of the tile-wise arithmetic uses a seventh of it, see
test_planted_row_classes), twice that where the logits come from a second GPU launch of the model.  nll and lse are compared with
ops.head_score bit for bit."""

import os
import statistics
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import predict_ref as R  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402
from oracle import parity_ops as PO  # noqa: E402

ROW = PO.BOUNDS['ce_loss']
BF16 = torch.bfloat16
HEAD = (32768, 50280, 768)  # the bench shape of the head
K0 = 768


@pytest.fixture(scope='module')
def P():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  import plainlm_amd
  return plainlm_amd


@pytest.fixture(scope='module')
def mdl(golden_dir):
  z = np.load(os.path.join(golden_dir, 'model.npz'))
  return {k: torch.from_numpy(z[k]) for k in z.files}


def _weights(mdl):
  return {k[2:]: v for k, v in mdl.items() if k.startswith('w:')}


def _planted(L, t=None, **kw):
  """head_predict on Y = I_K, W = L^T padded to K columns: row i of Y W^T is exactly row i of L (products with 1, sums with 0); the rows
  behind the planted ones are all-zero logits.  M = K = 768 takes the persistent path.  Returns (the result, Y, W, targets) on the GPU."""
  from plainlm_amd import ops
  M, V = L.shape
  assert M <= K0
  W = torch.zeros(V, K0, dtype=BF16)
  W[:, :M] = L.to(BF16).t()
  tt = None
  if t is not None:
    tt = torch.full((K0,), -100, dtype=torch.int64)
    tt[:M] = t
    tt = tt.cuda()
  Y, W = torch.eye(K0, dtype=BF16).cuda(), W.cuda()
  return ops.head_predict(Y, W, tt, **kw), Y, W, tt


def _err(got, ref):
  return (got.detach().double().cpu() - ref.cpu()).abs().nan_to_num(nan=float('inf')).max().item()


# ---- 1. planted logits, exact ----------------------------------------------------------------------------------------------------
def _tie_rows(V):
  """(rows [n, V] fp32, expected pred [n]): zeros except the listed columns."""
  pairs = [(0, 1),                                                    # the same lane
           (3, 4),                                                    # across the four lanes of a row
           (5, 21),                                                   # across 16-column blocks
           (10, 74), (10, 106),                                       # across waves (64- and 96-column wave tiles)
           (127, 128), (191, 192), (255, 256), (100, 356), (7, V - 1)]  # across tile columns of every width
  rows, want = [], []
  for a, b in pairs:     # equal values: the lower column wins
    r = torch.zeros(V)
    r[a] = r[b] = 5.0
    rows.append(r)
    want.append(a)
  for a, b in pairs:     # the larger value on the higher column: that column wins
    r = torch.zeros(V)
    r[a], r[b] = 5.0, 6.0
    rows.append(r)
    want.append(b)
  r = torch.zeros(V)     # all of the last 8 columns equal (the ragged edge tile: its clamped duplicates must not win)
  r[V - 8:] = 7.0
  rows.append(r)
  want.append(V - 8)
  r = torch.zeros(V)     # the maximum only in the last column
  r[V - 1] = 3.0
  rows.append(r)
  want.append(V - 1)
  r = torch.full((V,), -2.0)  # negative logits: nothing the kernel pads with (0, or a duplicate) may beat -1
  r[V - 3] = r[300] = -1.0
  rows.append(r)
  want.append(300)
  return torch.stack(rows), torch.tensor(want, dtype=torch.int64)


@pytest.mark.parametrize('V', [776, 50280])
def test_planted_ties_at_every_level_of_the_reduction(P, V):
  """V = 776 is ragged for 128-, 192- and 256-column tiles.  Equal maxima that meet inside a lane, across the four lanes of a row,
  across 16-column blocks, across waves, and across tile columns of every tile width: pred is exact."""
  L, want = _tie_rows(V)
  n = L.shape[0]
  r, _, _, _ = _planted(L)
  pred = r.pred.cpu()
  bad = [(i, int(pred[i]), int(want[i])) for i in range(n) if pred[i] != want[i]]
  print(f'head_predict planted ties V={V}: {n} rows, mismatches (row, got, want) {bad}')
  assert not bad
  assert r.nll is None and r.lse is None and r.entropy is not None
  assert int(pred.min()) >= 0 and int(pred.max()) < V
  ref = R.predict_reference(L.to(BF16))
  le, ee = _err(r.logp[:n], ref['logp']), _err(r.entropy[:n], ref['entropy'])
  # the all-zero rows behind the planted ones: uniform
  assert torch.all(pred[n:] == 0)
  pl = (r.logp[n:].cpu().double() + np.log(V)).abs().max().item()
  pe = (r.entropy[n:].cpu().double() - np.log(V)).abs().max().item()
  print(f'head_predict planted ties V={V}: logp err {le:.2e} entropy err {ee:.2e}; zero rows: logp {pl:.2e} entropy {pe:.2e} (bound {ROW:.1e})')
  assert le <= ROW and ee <= ROW and pl <= ROW and pe <= ROW
  assert torch.all(r.logp <= 0)


# ---- 2. planted row classes ----------------------------------------------------------------------------------------------------
PLANTED_CASES = sorted({(M, V) for M, V, _ in PO.CE_CASES if V % 8 == 0 and M <= 768})


@pytest.mark.parametrize('M,V', PLANTED_CASES)
def test_planted_row_classes(P, M, V):
  """Every row class of the cross-entropy parity inputs.  The fp32 tile-wise restatement of tests/predict_ref.py on the same rows is
  checked to be within ROW / 7 of fp64 (measured: 1.3e-6 logp, 3.4e-6 entropy at worst over these cases): the bound leaves the kernel
  a factor of 7 over its own arithmetic."""
  from plainlm_amd import ops
  L, t = PO.ce_inputs(M, V, seed=1000 + V)
  ref = R.predict_reference(L)
  cpu = R.tilewise_fp32(L, 128)
  cl, ce = _err(cpu['logp'], ref['logp']), _err(cpu['entropy'], ref['entropy'])
  assert torch.equal(cpu['pred'], ref['pred']) and cl <= ROW / 7 and ce <= ROW / 7, (cl, ce)
  r, Y, W, tt = _planted(L, t, want_lse=True)
  le, ee = _err(r.logp[:M], ref['logp']), _err(r.entropy[:M], ref['entropy'])
  print(f'head_predict planted M={M} V={V}: logp err {le:.2e} entropy err {ee:.2e} (bound {ROW:.1e}; fp32 restatement {cl:.2e} / {ce:.2e}), '
        f'{int(R.tied_rows(L).sum())} rows with a tied maximum')
  assert torch.equal(r.pred[:M].cpu(), ref['pred'].cpu())
  assert int(r.pred.min()) >= 0 and int(r.pred.max()) < V
  assert le <= ROW and ee <= ROW
  nll, lse = ops.head_score(Y, W, tt, want_lse=True)
  assert torch.equal(r.nll, nll) and torch.equal(r.lse, lse)


# ---- 3. the same logits as the GEMM ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,V,K', [(1000, 50280, 768), (4096, 32000, 1024), (300, 1000, 128)])
def test_same_logits_as_the_gemm(P, M, V, K):
  from plainlm_amd import ops
  g = torch.Generator().manual_seed(M + V)
  Y = torch.randn(M, K, generator=g).to(BF16).cuda()
  W = (0.02 * torch.randn(V, K, generator=g)).to(BF16).cuda()
  t = torch.randint(0, V, (M,), generator=g)
  t[torch.rand(M, generator=g) < 0.05] = -100
  t = t.cuda()
  logits = ops.gemm_nt(Y, W)  # the parent's unchanged kernel: the yardstick
  want = R.first_argmax(logits)
  tied = int(R.tied_rows(logits).sum())
  r = ops.head_predict(Y, W, t, want_lse=True)
  r2 = ops.head_predict(Y, W, t, want_lse=True)
  for a, b in zip(r, r2):
    assert torch.equal(a, b)  # deterministic
  wrong = int((r.pred != want).sum())
  print(f'head_predict vs gemm_nt logits M={M} V={V} K={K}: {tied} of {M} rows have a tied maximum, {wrong} predictions differ')
  assert torch.equal(r.pred, want)
  if (M, V, K) == (1000, 50280, 768):
    assert tied >= 10  # the exactness claim covers ties (the CPU's fp32 product of these operands has 53)
  ref = R.predict_reference(logits)
  le, ee = _err(r.logp, ref['logp']), _err(r.entropy, ref['entropy'])
  print(f'head_predict vs gemm_nt logits M={M} V={V} K={K}: logp err {le:.2e} entropy err {ee:.2e} (bound {ROW:.1e})')
  assert le <= ROW and ee <= ROW
  nll, lse = ops.head_score(Y, W, t, want_lse=True)
  assert torch.equal(r.nll, nll) and torch.equal(r.lse, lse)
  assert int((r.nll == 0).sum()) >= int((t < 0).sum()) > 0
  # fewer outputs: the remaining ones keep their bits
  a = ops.head_predict(Y, W)
  assert a.nll is None and a.lse is None and torch.equal(a.pred, r.pred) and torch.equal(a.logp, r.logp) and torch.equal(a.entropy, r.entropy)
  b = ops.head_predict(Y, W, t, want_entropy=False)
  assert b.entropy is None and b.lse is None and torch.equal(b.pred, r.pred) and torch.equal(b.logp, r.logp) and torch.equal(b.nll, r.nll)
  c = ops.head_predict(Y, W, None, want_entropy=False, want_lse=True)
  assert c.entropy is None and c.nll is None and torch.equal(c.pred, r.pred) and torch.equal(c.lse, r.lse)


# ---- 4. bench shape ------------------------------------------------------------------------------------------------------------
def _head_operands(seed=5):
  M, V, K = HEAD
  g = torch.Generator(device='cuda').manual_seed(seed)
  Y = torch.randn(M, K, generator=g, device='cuda').to(BF16)
  W = (0.02 * torch.randn(V, K, generator=g, device='cuda')).to(BF16)
  t = torch.randint(0, V, (M,), generator=g, device='cuda')
  return Y, W, t


def _parent_logits(ops, Y, W, out_pad):
  M, V = Y.shape[0], W.shape[0]
  buf = torch.empty((M, out_pad), dtype=BF16, device=Y.device)
  ops.gemm_nt(Y, W, out=buf[:, :V])
  return buf


def test_bench_shape_predictions_and_memory(P):
  from plainlm_amd import ops
  M, V, K = HEAD
  Y, W, t = _head_operands()
  ops.release_workspaces()  # the workspace is part of the cost
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  r = ops.head_predict(Y, W, t)
  torch.cuda.synchronize()
  rise = torch.cuda.max_memory_allocated() - base
  logits = M * 50304 * 2
  print(f'head_predict bench shape: peak memory rises by {rise / 2**20:.1f} MiB = {100.0 * rise / logits:.2f} % of the {logits / 2**20:.0f} MiB logits buffer')
  assert rise <= 0.08 * logits, f'peak memory rose by {rise} bytes = {100.0 * rise / logits:.2f} % of the logits buffer ({logits} bytes)'
  buf = _parent_logits(ops, Y, W, 50304)
  want = torch.cat([R.first_argmax(buf[r0:r0 + 1024, :V]) for r0 in range(0, M, 1024)])
  wrong = int((r.pred != want).sum())
  print(f'head_predict bench shape: {wrong} of {M} predictions differ from the first-index argmax of the gemm_nt logits')
  assert torch.equal(r.pred, want)


def test_bench_shape_time_vs_parent_path(P):
  """Interleaved in one process, random operands: A = gemm_nt into a fresh [M, out_pad] buffer + torch.argmax + ce_fwd_bwd_ + mean
  (today's route to loss and prediction; entropy left out, in A's favour), B = head_predict (entropy included) + mean.
  median(B) <= median(A); both are printed with their min-max."""
  from plainlm_amd import ops
  M, V, K = HEAD
  Y, W, t = _head_operands()
  def run(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)
  def fa():
    buf = _parent_logits(ops, Y, W, 50304)
    pred = torch.argmax(buf[:, :V], dim=-1)
    return pred, ops.mean(ops.ce_fwd_bwd_(buf, t, 1.0 / M, V=V))
  def fb():
    r = ops.head_predict(Y, W, t)
    return r.pred, ops.mean(r.nll)
  for _ in range(3):
    run(fa), run(fb)
  ta, tb = [], []
  for _ in range(12):
    ta.append(run(fa))
    tb.append(run(fb))
  ma, mb = statistics.median(ta), statistics.median(tb)
  print(f'head_predict bench shape time: A (gemm_nt + argmax + ce + mean) median {ma:.3f} ms [min {min(ta):.3f} max {max(ta):.3f}], '
        f'B (head_predict + mean) median {mb:.3f} ms [min {min(tb):.3f} max {max(tb):.3f}], B / A = {mb / ma:.3f}')
  assert mb <= ma


# ---- 5. model ------------------------------------------------------------------------------------------------------------------
def _small(P, mdl):
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  m.load_state_dict(_weights(mdl))
  return m.cuda()


def _predict_checks(m, ids, tgt, V, mask=None):
  with torch.no_grad():
    p = m.predict(ids, mask, targets=tgt)
    q = m.predict(ids, mask)
    logits = m(ids, mask)
    nll = m.score(ids, tgt, mask)
    last = m.predict(ids, mask, targets=tgt, last_only=True)
  B, T = ids.shape
  assert p.tokens.dtype == torch.int64 and p.logprob.dtype == torch.float32 and p.entropy.dtype == torch.float32
  assert tuple(p.tokens.shape) == tuple(p.logprob.shape) == tuple(p.entropy.shape) == tuple(p.nll.shape) == (B, T)
  assert q.nll is None and torch.equal(q.tokens, p.tokens) and torch.equal(q.logprob, p.logprob) and torch.equal(q.entropy, p.entropy)
  flat = logits.view(-1, V)
  ref = R.predict_reference(flat)
  assert torch.equal(p.tokens.view(-1), R.first_argmax(flat))
  le, ee = _err(p.logprob.view(-1), ref['logp']), _err(p.entropy.view(-1), ref['entropy'])
  print(f'predict vs forward() logits: logprob err {le:.2e} entropy err {ee:.2e} (bound {2 * ROW:.1e})')
  assert le <= 2 * ROW and ee <= 2 * ROW
  assert torch.equal(p.nll, nll)
  assert tuple(last.tokens.shape) == (B,)
  assert torch.equal(last.tokens, p.tokens[:, -1]) and torch.equal(last.logprob, p.logprob[:, -1])
  assert torch.equal(last.entropy, p.entropy[:, -1]) and torch.equal(last.nll, p.nll[:, -1])


def test_predict_on_the_golden_model(P, mdl):
  from plainlm_amd import functional as Fn
  m = _small(P, mdl)
  tok = mdl['tokens']
  ids, tgt = tok[:, :64].cuda(), tok[:, 1:65].clone()
  tgt[0, 5] = tgt[1, 63] = -100  # an ignored target inside, and in the last column
  tgt = tgt.cuda()
  _predict_checks(m, ids, tgt, 256)
  docs = [[int(v) for v in row if v > 0] for row in mdl['docs_lengths']]
  ds = O.doc_start_from_lengths(docs, 64)
  _predict_checks(m, ids, tgt, 256, mask=ds.cuda())
  g = torch.Generator().manual_seed(11)
  dense = torch.tril(torch.rand(2, 64, 64, generator=g) < 0.7) | torch.eye(64, dtype=torch.bool)
  _predict_checks(m, ids, tgt, 256, mask=Fn.DenseMask(dense.cuda(), 2))
  with pytest.raises(RuntimeError, match=r'loss\(\)'):
    m.predict(ids)  # grad enabled, parameters require grad
  with torch.no_grad(), pytest.raises(ValueError, match='targets'):
    m.predict(ids, targets=tgt[:, :10])


def test_predict_160m_shape_tokens(P):
  """M = 2 x 1024 = 2048 rows: the persistent path inside a model.  tokens against the first-index argmax of forward()'s logits."""
  ocfg = O.OracleConfig(vocab_size=50280, seq_len=1024, dim=768, n_layers=12, n_heads=12)
  w = O.init_params(ocfg, seed=7)
  rng = np.random.default_rng(1234)
  ids = torch.from_numpy(rng.integers(0, 50280, size=(2, 1024))).cuda()
  m = P.Transformer(P.ModelConfig(vocab_size=50280, seq_len=1024, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu'))
  m.load_state_dict(w)
  m = m.cuda()
  with torch.no_grad():
    p = m.predict(ids)
    logits = m(ids).view(-1, 50280)
    last = m.predict(ids, last_only=True)
  assert torch.equal(p.tokens.view(-1), R.first_argmax(logits))
  assert torch.all(p.logprob <= 0) and torch.all(p.entropy >= 0) and p.nll is None
  # the next-token call: 2 rows through the 128x128 path (another kernel's accumulation order: no bit comparison with the full call)
  assert tuple(last.tokens.shape) == (2,) and int(last.tokens.min()) >= 0 and int(last.tokens.max()) < 50280 and torch.all(last.logprob <= 0)


# ---- 6. engine -----------------------------------------------------------------------------------------------------------------
def _engine_cfg(**over):
  EC = dict(model='transformer', vocab_size=256, seq_len=64, d_model=128, expand='8/3', n_layers=2, n_heads=2,
            mlp_class='glu', tie_embeddings=False, torch_compile=False, micro_batch_size=1, grad_accumulation_steps=1,
            dtype='bfloat16', optim='adamw', fused_optim=True, lr=3e-3, weight_decay=0.1, beta1=0.9, beta2=0.95,
            grad_clip=1.0, scheduler='warmup_cosine', warmup_steps=2, cooldown_steps=None, lr_start=0.0, lr_end=1e-5,
            lr_end_pct=None, steps_budget=8, resume=False, seed=100)
  EC.update(over)
  return namedtuple('Config', EC.keys())(**EC)


def _engine(P, mdl, **over):
  cfg = _engine_cfg(**over)
  model, _ = P.construct_model(cfg)
  model.load_state_dict(_weights(mdl))
  return P.TorchEngine(model, cfg, 'cuda', None, None)


def test_engine_eval_metrics(P, mdl):
  tok = mdl['tokens']
  batches = [{'input_ids': tok[:1]}, {'input_ids': tok[1:]}]
  eng = _engine(P, mdl, eval_head='fused')
  val = eng.eval(batches)
  got = eng.eval_metrics(batches)
  assert set(got) == {'loss', 'accuracy', 'entropy', 'tokens'}
  assert got['loss'] == val, (got['loss'], val)  # equal floats: the same per-batch means, summed in the same order
  with torch.no_grad():
    logits = torch.cat([eng.model(tok[i:i + 1, :64].cuda()).view(-1, 256) for i in range(2)])
  tgt = torch.cat([tok[i, 1:65] for i in range(2)])
  ref = R.predict_reference(logits)
  acc = (R.first_argmax(logits).cpu() == tgt).double().mean().item()
  ent = ref['entropy'].mean().item()  # fp64
  print(f"eval_metrics: {got}; from forward() logits: accuracy {acc:.6f} entropy {ent:.6f}")
  assert got['tokens'] == tgt.numel() == 128
  assert got['accuracy'] == acc
  assert abs(got['entropy'] - ent) <= 2 * ROW
  # training state untouched: the steps after the call are bit-identical to a run without it
  plain = _engine(P, mdl, eval_head='fused')
  a = [eng.step({'input_ids': tok[i % 2:i % 2 + 1]}).item() for i in range(3)]
  b = [plain.step({'input_ids': tok[i % 2:i % 2 + 1]}).item() for i in range(3)]
  assert a == b, (a, b)


def test_engine_eval_metrics_schedule_free_swap(P, mdl):
  tok = mdl['tokens']
  eng = _engine(P, mdl, optim='sfo_adamw')
  eng.step({'input_ids': tok[:1]})
  got = eng.eval_metrics([{'input_ids': tok[1:]}])
  assert np.isfinite(got['loss']) and 0.0 <= got['accuracy'] <= 1.0 and got['entropy'] >= 0 and got['tokens'] == 64
  assert all(not g['train_mode'] for g in eng.optimizer.param_groups)  # evaluated at the averaged iterate; step() swaps back
  eng.step({'input_ids': tok[:1]})
  assert all(g['train_mode'] for g in eng.optimizer.param_groups)
