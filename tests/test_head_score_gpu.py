"""Forward-only scoring head on MI355X (ops.head_score, Transformer.score / token_logprobs, HipEngine eval_head='fused').

Bounds are the project's own: BOUNDS['ce_loss'] (oracle/parity_ops.py, 3e-5 nats against the fp64 lse - x_t of the bf16 logits) for
per-row numbers, LOSS_RTOL (1e-4 relative, tests/test_model_gpu.py:17) against the fp32 oracle.  Where two GPU paths that are each
within the row bound of the same fp64 value are compared, the bound is twice it; the relative bound on means derived from that is
MEAN_RTOL = 1e-6 (6e-5 nats at a loss near 11, with slack for the two means' fp32 round-off)."""

import os
import statistics
from collections import namedtuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity_ops as PO  # noqa: E402

LOSS_RTOL = 1e-4  # tests/test_model_gpu.py:17
MEAN_RTOL = 1e-6
ROW = PO.BOUNDS['ce_loss']
BF16 = torch.bfloat16
HEAD = (32768, 50280, 768)  # the bench shape of the head


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


def _planted(P, L, t, K=768):
  """head_score on Y = I_K, W = L^T padded to K columns: row i of Y W^T is exactly row i of L (products with 1, sums with 0)."""
  from plainlm_amd import ops
  M, V = L.shape
  assert M <= K
  W = torch.zeros(V, K, dtype=BF16)
  W[:, :M] = L.t()
  tt = torch.full((K,), -100, dtype=torch.int64)
  tt[:M] = t
  nll, lse = ops.head_score(torch.eye(K, dtype=BF16).cuda(), W.cuda(), tt.cuda(), want_lse=True)
  return nll.cpu().double(), lse.cpu().double()


PLANTED_CASES = sorted({(M, V) for M, V, _ in PO.CE_CASES if V % 8 == 0 and M <= 768})


@pytest.mark.parametrize('M,V', PLANTED_CASES)
def test_planted_logits_every_row_class(P, M, V):
  L, t = PO.ce_inputs(M, V, seed=1000 + V)
  ref = PO.ce_reference(L, t, 1.0, V)
  nll, lse = _planted(P, L, t)
  valid = ref['valid']
  err = (nll[:M] - ref['loss']).abs().nan_to_num(nan=float('inf'))[valid].max().item()
  lse64 = torch.logsumexp(L.double(), -1)
  lerr = (lse[:M] - lse64).abs().nan_to_num(nan=float('inf')).max().item()
  # the rows behind the planted ones are all-zero logits: lse = log V, target ignored
  pad = (lse[M:] - np.log(V)).abs().max().item() if M < 768 else 0.0
  print(f'head_score planted M={M} V={V}: nll err {err:.2e} lse err {lerr:.2e} pad rows {pad:.2e} (bound {ROW:.1e})')
  assert err <= ROW
  assert torch.all(nll[:M][~valid] == 0) and torch.all(nll[M:] == 0)
  assert lerr <= ROW and pad <= ROW


def test_planted_edge_tile_and_tile_owner(P):
  """Rows whose only large logits sit in the last 24 columns of V = 50280 (the clamped duplicates of the ragged edge tile would count
  them twice: + log 2 on lse) or in the last column of an interior tile of every tile width (128 / 192 / 256), target there too (an
  off-by-one tile owner reads another column's logit, or none)."""
  V = 50280
  cols = [127, 128, 191, 192, 255, 256, 383, 384, 50175, 50176, V - 24, V - 9, V - 8, V - 1]
  L = torch.zeros(len(cols) + 1, V)
  t = torch.zeros(len(cols) + 1, dtype=torch.int64)
  for i, c in enumerate(cols):
    L[i, c] = 20.0
    t[i] = c
  L[-1, V - 24:] = torch.linspace(15, 20, 24)  # the whole edge
  t[-1] = V - 24
  L = L.to(BF16)
  ref = PO.ce_reference(L, t, 1.0, V)
  nll, lse = _planted(P, L, t)
  n = L.shape[0]
  err = (nll[:n] - ref['loss']).abs().nan_to_num(nan=float('inf')).max().item()
  lerr = (lse[:n] - torch.logsumexp(L.double(), -1)).abs().nan_to_num(nan=float('inf')).max().item()
  print(f'head_score planted edges: nll err {err:.2e} lse err {lerr:.2e}')
  assert err <= ROW and lerr <= ROW


@pytest.mark.parametrize('M,V,K', [(1000, 50280, 768), (4096, 32000, 1024), (300, 1000, 128)])
def test_same_logits_as_the_training_head(P, M, V, K):
  from plainlm_amd import ops
  g = torch.Generator().manual_seed(M + V)
  Y = torch.randn(M, K, generator=g).to(BF16).cuda()
  W = (0.02 * torch.randn(V, K, generator=g)).to(BF16).cuda()
  t = torch.randint(0, V, (M,), generator=g)
  t[torch.rand(M, generator=g) < 0.05] = -100
  ref = PO.ce_reference(ops.gemm_nt(Y, W), t, 1.0, V)  # the parent's unchanged kernel: the yardstick
  nll, lse = ops.head_score(Y, W, t.cuda(), want_lse=True)
  nll2, lse2 = ops.head_score(Y, W, t.cuda(), want_lse=True)
  assert torch.equal(nll, nll2) and torch.equal(lse, lse2)
  nll = nll.cpu().double()
  valid = ref['valid']
  err = (nll - ref['loss']).abs().nan_to_num(nan=float('inf'))[valid].max().item()
  print(f'head_score vs gemm_nt logits M={M} V={V} K={K}: nll err {err:.2e} (bound {ROW:.1e})')
  assert err <= ROW
  assert torch.all(nll[~valid] == 0) and int((~valid).sum()) > 0
  assert torch.equal(ops.head_score(Y, W, t.cuda()), nll2)  # without lse: same numbers


def _head_operands(seed=5):
  M, V, K = HEAD
  g = torch.Generator(device='cuda').manual_seed(seed)
  Y = torch.randn(M, K, generator=g, device='cuda').to(BF16)
  W = (0.02 * torch.randn(V, K, generator=g, device='cuda')).to(BF16)
  t = torch.randint(0, V, (M,), generator=g, device='cuda')
  return Y, W, t


def _parent_head(ops, Y, W, t, out_pad):
  """What evaluation does today: the training head's forward (HeadLossFn.forward under no_grad)."""
  M, V = Y.shape[0], W.shape[0]
  buf = torch.empty((M, out_pad), dtype=BF16, device=Y.device)
  ops.gemm_nt(Y, W, out=buf[:, :V])
  rows = ops.ce_fwd_bwd_(buf, t, 1.0 / M, V=V)
  return rows, ops.mean(rows)


def test_bench_shape_rows_and_mean_vs_parent_path(P):
  from plainlm_amd import ops
  M, V, K = HEAD
  Y, W, t = _head_operands()
  rows, mean_a = _parent_head(ops, Y, W, t, 50304)
  nll = ops.head_score(Y, W, t)
  mean_b = ops.mean(nll)
  err = (nll.double() - rows.double()).abs().max().item()
  rel = abs(mean_a.item() - mean_b.item()) / abs(mean_a.item())
  print(f'head_score bench shape: max row diff {err:.2e} (bound {2 * ROW:.1e}), means {mean_a.item():.7f} / {mean_b.item():.7f} rel {rel:.2e} (bound {MEAN_RTOL:.0e})')
  assert err <= 2 * ROW
  assert rel <= MEAN_RTOL


def test_bench_shape_memory(P):
  from plainlm_amd import ops
  M, V, K = HEAD
  Y, W, t = _head_operands()
  ops.release_workspaces()  # the workspace is part of the cost
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  nll = ops.head_score(Y, W, t)
  torch.cuda.synchronize()
  rise = torch.cuda.max_memory_allocated() - base
  logits = M * 50304 * 2
  print(f'head_score bench shape: peak memory rises by {rise / 2**20:.1f} MiB = {100.0 * rise / logits:.2f} % of the {logits / 2**20:.0f} MiB logits buffer')
  assert rise <= 0.05 * logits, f'peak memory rose by {rise} bytes = {100.0 * rise / logits:.2f} % of the logits buffer ({logits} bytes)'
  assert nll.shape == (M,)


def test_bench_shape_time_vs_parent_path(P):
  """Interleaved in one process, random operands: A = gemm_nt into a fresh [M, out_pad] buffer + ce_fwd_bwd_ + mean (today's eval
  head), B = head_score + mean.  median(B) <= median(A); A's own min-max spread is printed as the margin."""
  from plainlm_amd import ops
  Y, W, t = _head_operands()
  def run(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)
  fa = lambda: _parent_head(ops, Y, W, t, 50304)
  fb = lambda: ops.mean(ops.head_score(Y, W, t))
  for _ in range(3):
    run(fa), run(fb)
  ta, tb = [], []
  for _ in range(12):
    ta.append(run(fa))
    tb.append(run(fb))
  ma, mb = statistics.median(ta), statistics.median(tb)
  print(f'head_score bench shape time: A (gemm_nt + ce + mean) median {ma:.3f} ms [min {min(ta):.3f} max {max(ta):.3f}], '
        f'B (head_score + mean) median {mb:.3f} ms [min {min(tb):.3f} max {max(tb):.3f}], B / A = {mb / ma:.3f}')
  assert mb <= ma


# ---- model level ----------------------------------------------------------------------------------------------------------------
def _small(P, mdl):
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  m.load_state_dict(_weights(mdl))
  return m.cuda()


def _score_checks(m, ids, tgt, V, oracle_loss, mask=None):
  F = torch.nn.functional
  with torch.no_grad():
    rows = m.score(ids, tgt, mask)
    mean = m.score(ids, tgt, mask, reduction='mean')
    total = m.score(ids, tgt, mask, reduction='sum')
    logits = m(ids, mask).float().view(-1, V)
    lp = m.token_logprobs(ids, tgt, mask)
  assert rows.dtype == torch.float32 and tuple(rows.shape) == tuple(ids.shape) and mean.dim() == 0 and total.dim() == 0
  assert torch.equal(lp, -rows)
  ref_rows = F.cross_entropy(logits, tgt.view(-1), reduction='none')
  err = (rows.view(-1) - ref_rows).abs().max().item()
  print(f'score rows vs F.cross_entropy of forward(): {err:.2e} (bound {2 * ROW:.1e})')
  assert err <= 2 * ROW
  if oracle_loss is not None:
    rel = abs(mean.item() - oracle_loss) / abs(oracle_loss)
    print(f'score mean {mean.item():.6f} vs fp32 oracle {oracle_loss:.6f}: rel {rel:.2e}')
    assert rel <= LOSS_RTOL
  # 10 % ignored: the divisor is the number of non-ignored targets (CrossEntropyLoss's rule)
  tg2 = tgt.clone()
  g = torch.Generator().manual_seed(3)
  tg2.view(-1)[(torch.rand(tgt.numel(), generator=g) < 0.1).to(tgt.device)] = -100
  with torch.no_grad():
    mean2 = m.score(ids, tg2, mask, reduction='mean')
    rows2 = m.score(ids, tg2, mask)
  ref2 = F.cross_entropy(logits, tg2.view(-1), reduction='mean')
  rel2 = abs(mean2.item() - ref2.item()) / abs(ref2.item())
  print(f'score mean with ignored targets {mean2.item():.7f} vs F.cross_entropy {ref2.item():.7f}: rel {rel2:.2e} (bound {MEAN_RTOL:.0e})')
  assert torch.all(rows2.view(-1)[tg2.view(-1) < 0] == 0)
  assert rel2 <= MEAN_RTOL
  with torch.no_grad():
    assert torch.isnan(m.score(ids, torch.full_like(tgt, -100), mask, reduction='mean'))  # 0 / 0, as torch gives


def test_score_on_the_golden_model(P, mdl):
  m = _small(P, mdl)
  tok = mdl['tokens']
  ids, tgt = tok[:, :64].cuda(), tok[:, 1:65].cuda()
  ocfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=2)
  ref = O.loss_fn(_weights(mdl), ocfg, tok[:, :64], tok[:, 1:65]).item()
  with torch.no_grad():
    _score_checks(m, ids, tgt, 256, ref)
  with pytest.raises(RuntimeError, match=r'loss\(\)'):
    m.score(ids, tgt)  # grad enabled, parameters require grad
  with torch.no_grad(), pytest.raises(ValueError, match='reduction'):
    m.score(ids, tgt, reduction='avg')


def test_score_through_a_document_mask_and_a_dense_mask(P, mdl):
  from plainlm_amd import functional as Fn
  m = _small(P, mdl)
  tok = mdl['tokens']
  ids, tgt = tok[:, :64].cuda(), tok[:, 1:65].cuda()
  docs = [[int(v) for v in row if v > 0] for row in mdl['docs_lengths']]
  ds = O.doc_start_from_lengths(docs, 64)
  with torch.no_grad():
    _score_checks(m, ids, tgt, 256, None, mask=ds.cuda())
    g = torch.Generator().manual_seed(11)
    dense = torch.tril(torch.rand(2, 64, 64, generator=g) < 0.7) | torch.eye(64, dtype=torch.bool)
    _score_checks(m, ids, tgt, 256, None, mask=Fn.DenseMask(dense.cuda(), 2))


def test_score_160m_shape_vs_oracle(P):
  ocfg = O.OracleConfig(vocab_size=50280, seq_len=1024, dim=768, n_layers=12, n_heads=12)
  w = O.init_params(ocfg, seed=7)
  rng = np.random.default_rng(1234)
  tok = torch.from_numpy(rng.integers(0, 50280, size=(2, 1025)))
  ids, tgt = tok[:, :1024], tok[:, 1:]
  m = P.Transformer(P.ModelConfig(vocab_size=50280, seq_len=1024, dim=768, expand=8 / 3, n_layers=12, n_heads=12, mlp='glu'))
  m.load_state_dict(w)
  m = m.cuda()
  torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
  ref = O.loss_fn(w, ocfg, ids, tgt).item()
  with torch.no_grad():
    _score_checks(m, ids.cuda(), tgt.cuda(), 50280, ref)


# ---- engine ---------------------------------------------------------------------------------------------------------------------
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


def test_engine_fused_eval_head(P, mdl):
  tok = mdl['tokens']
  batches = [{'input_ids': tok[:1]}, {'input_ids': tok[1:]}]
  val_logits = _engine(P, mdl).eval(batches)
  eng = _engine(P, mdl, eval_head='fused')
  val_fused = eng.eval(batches)
  ocfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=2)
  ref = np.mean([O.loss_fn(_weights(mdl), ocfg, tok[i:i + 1, :64], tok[i:i + 1, 1:65]).item() for i in range(2)])
  print(f'engine eval: logits head {val_logits:.7f} fused head {val_fused:.7f} oracle {ref:.7f}')
  assert abs(val_fused - val_logits) <= LOSS_RTOL * abs(val_logits)
  assert abs(val_fused - ref) <= LOSS_RTOL * abs(ref)
  # training state untouched: the steps after a fused eval() are bit-identical to a run without it
  plain = _engine(P, mdl, eval_head='fused')
  a = [eng.step({'input_ids': tok[i % 2:i % 2 + 1]}).item() for i in range(3)]
  b = [plain.step({'input_ids': tok[i % 2:i % 2 + 1]}).item() for i in range(3)]
  assert a == b, (a, b)
  with pytest.raises(ValueError, match='eval_head'):
    _engine(P, mdl, eval_head='fast')


def test_engine_fused_eval_head_schedule_free_swap(P, mdl):
  tok = mdl['tokens']
  eng = _engine(P, mdl, eval_head='fused', optim='sfo_adamw')
  eng.step({'input_ids': tok[:1]})
  val = eng.eval([{'input_ids': tok[1:]}])
  assert np.isfinite(val)
  assert all(not g['train_mode'] for g in eng.optimizer.param_groups)  # evaluated at the averaged iterate; step() swaps back
  eng.step({'input_ids': tok[:1]})
  assert all(g['train_mode'] for g in eng.optimizer.param_groups)
