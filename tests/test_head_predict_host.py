"""CPU tests (no GPU) of the prediction head: its two entry points refuse bad arguments before any HIP call (the header, the binding
table and the library are compared in tests/test_host_logic.py), the workspace is a few per cent of the logits buffer, the kernels that
carry the prediction mode meet the plain NT kernel's register / K-loop bar, the Python layers validate their options, and the reference
arithmetic of tests/predict_ref.py is itself within a seventh of the GPU tests' bound."""

import ast
import ctypes as C
import os
import re
import subprocess
import sys
from collections import namedtuple

import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import predict_ref as R  # noqa: E402
from oracle import parity_ops as PO  # noqa: E402


def _lib_loaded():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


def test_head_predict_entry_point_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  assert lib.plm_version() == 112  # the prediction head's additions did not move it
  p = lambda: C.c_void_p(0x100000)  # plausible, never dereferenced
  def refused(*args):
    rc = lib.plm_head_predict_bf16(*args)
    assert rc < 0, rc
    msg = (lib.plm_last_error_string() or b'').decode()
    assert 'plm_head_predict_bf16' in msg, msg
    return rc, msg
  big = 1 << 40
  # Y, ldy, W, ldw, targets, pred, logp, entropy, nll, lse, M, V, K, workspace, bytes, stream
  assert 'null pointer' in refused(None, 768, p(), 768, p(), p(), p(), None, None, None, 512, 1024, 768, p(), big, None)[1]
  assert 'null pointer' in refused(p(), 768, None, 768, p(), p(), p(), None, None, None, 512, 1024, 768, p(), big, None)[1]
  assert 'null pointer' in refused(p(), 768, p(), 768, p(), None, p(), None, None, None, 512, 1024, 768, p(), big, None)[1]
  assert 'null pointer' in refused(p(), 768, p(), 768, p(), p(), None, None, None, None, 512, 1024, 768, p(), big, None)[1]
  assert 'null pointer' in refused(p(), 768, p(), 768, p(), p(), p(), None, None, None, 512, 1024, 768, None, big, None)[1]
  msg = refused(p(), 768, p(), 768, None, p(), p(), None, p(), None, 512, 1024, 768, p(), big, None)[1]  # nll without targets
  assert 'null pointer' in msg and 'targets' in msg
  assert 'K % 64' in refused(p(), 776, p(), 776, p(), p(), p(), None, None, None, 512, 1024, 776, p(), big, None)[1]
  assert 'multiples of 8' in refused(p(), 772, p(), 768, p(), p(), p(), None, None, None, 512, 1024, 768, p(), big, None)[1]
  assert 'multiples of 8' in refused(p(), 768, p(), 760, p(), p(), p(), None, None, None, 512, 1024, 768, p(), big, None)[1]  # ldw < K
  assert 'aligned' in refused(C.c_void_p(0x100002), 768, p(), 768, p(), p(), p(), None, None, None, 512, 1024, 768, p(), big, None)[1]
  assert 'aligned' in refused(p(), 768, p(), 768, p(), C.c_void_p(0x100004), p(), None, None, None, 512, 1024, 768, p(), big, None)[1]
  assert 'aligned' in refused(p(), 768, p(), 768, p(), p(), p(), C.c_void_p(0x100002), None, None, 512, 1024, 768, p(), big, None)[1]
  need = lib.plm_head_predict_workspace_bytes(512, 1024, 768)
  rc, msg = refused(p(), 768, p(), 768, p(), p(), p(), p(), p(), p(), 512, 1024, 768, p(), need - 1, None)
  assert rc == -4 and 'workspace' in msg  # PLM_E_WORKSPACE


def test_head_predict_workspace_is_positive_monotone_and_small():
  lib = _lib_loaded()
  prev = 0
  for M in (1, 8, 300, 511, 512, 1000, 4096, 8192, 32768, 65536):
    n = lib.plm_head_predict_workspace_bytes(M, 50280, 768)
    assert n > 0 and n >= prev, (M, n, prev)
    assert n >= lib.plm_head_score_workspace_bytes(M, 50280, 768)
    prev = n
  assert lib.plm_head_predict_workspace_bytes(0, 50280, 768) == 0
  bench = lib.plm_head_predict_workspace_bytes(32768, 50280, 768)
  assert bench <= 0.08 * 32768 * 50304 * 2  # the bench shape: 196.6 MiB next to 3144 MiB of logits
  assert bench >= 32768 * 393 * 16          # one 16-byte record per row and 128-column tile


@pytest.mark.timeout(600)
def test_the_kernels_that_carry_the_prediction_mode_meet_the_isa_bar():
  """The prediction mode is a run-time switch (EpiArgs.part4 != nullptr) INSIDE the four SCORE instantiations of gemm_nt_big_kernel -
  there is no second kernel - so those four carry it, and tests/test_head_score_host.py's bar holds for the new code as well.  Stated
  here again with what the mode adds: no spill, no scratch, at most 256 VGPRs (two workgroups per CU), at most one unconditional
  vmcnt(0) inside the K loop; and the two new small kernels exist and spill nothing."""
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'isa_scan.py'), 'gemm_big.hip'], capture_output=True, text=True, timeout=540)
  assert r.returncode == 0, r.stderr[-2000:]
  lines = r.stdout.splitlines()
  score, small = {}, {}
  for i, l in enumerate(lines):
    name = l.strip()
    if 'gemm_nt_big_kernel' in l and re.search(r'false, false, false, false, true>$', name):
      score[name] = (ast.literal_eval(lines[i + 1].strip()), lines[i + 2])
    if name in ('head_predict_combine_kernel', 'head_predict_rows_kernel'):
      small[name] = ast.literal_eval(lines[i + 1].strip())
  assert len(score) == 4, sorted(score)
  assert not any('predict' in l and 'gemm_nt' in l for l in lines)  # no second GEMM kernel: the mode lives in the four above
  for k, (meta, span) in score.items():
    assert meta['vspill'] == 0 and meta['sspill'] == 0 and meta['scratch'] == 0 and meta['vgpr'] <= 256, (k, meta)
    m = re.search(r'unconditional vmcnt\(0\): (\d+)', span)
    assert m and int(m.group(1)) <= 1, (k, span)
    m = re.search(r'scratch_: (\d+)', span)
    assert m and int(m.group(1)) == 0, (k, span)
  assert len(small) == 2, sorted(small)
  for k, meta in small.items():
    assert meta['vspill'] == 0 and meta['sspill'] == 0 and meta['scratch'] == 0, (k, meta)


def _cfg(**over):
  EC = dict(model='transformer', vocab_size=512, seq_len=128, d_model=128, expand='8/3', n_layers=2, n_heads=2,
            mlp_class='glu', tie_embeddings=False)
  EC.update(over)
  return namedtuple('Config', EC.keys())(**EC)


def test_python_layers_validate_and_have_no_cpu_path():
  from plainlm_amd import ops
  y, w = torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(16, 64, dtype=torch.bfloat16)
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.head_predict(y, w)
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.head_predict(y, w, torch.zeros(8, dtype=torch.int64))
  assert ops.HeadPredict._fields == ('pred', 'logp', 'entropy', 'nll', 'lse')
  assert P.HeadPrediction._fields == ('tokens', 'logprob', 'entropy', 'nll')
  model, _ = P.construct_model(_cfg())
  ids = torch.zeros(1, 128, dtype=torch.int64)
  with pytest.raises(RuntimeError, match='MI355X'):
    model.predict(ids)
  with torch.no_grad(), pytest.raises(RuntimeError, match='MI355X'):
    model.predict(ids, targets=ids, last_only=True)
  assert callable(engine.HipEngine.eval_metrics)
  ecfg = namedtuple('C', ['seq_len', 'grad_accumulation_steps', 'grad_clip', 'dtype'])(128, 1, 1.0, 'bfloat16')
  with pytest.raises(RuntimeError, match='no CPU path'):  # eval_metrics lives on the engine, and the engine has no CPU path
    P.TorchEngine(model, ecfg, 'cpu', None, None)


def test_reference_arithmetic_first_index_argmax_and_the_two_non_finite_hazards():
  """tests/predict_ref.py: the explicit first-index argmax, the fp64 definitions on hand-made rows, and the fp32 tile-wise restatement
  of the kernel's combine rule - which must survive -inf logits and empty records (a naive restatement gives NaN there) and, on the
  planted row classes the GPU test uses, stay within a seventh of that test's bound (3e-5 nats): the factor the bound leaves the kernel."""
  L = torch.tensor([[0., 2., 2., 1.], [3., 3., 3., 3.], [-1., -5., -1., -7.], [float('-inf'), 0., float('-inf'), 0.]])
  assert R.first_argmax(L).tolist() == [1, 0, 0, 1]
  assert R.tied_rows(L).tolist() == [True, True, True, True]
  ref = R.predict_reference(L)
  assert ref['pred'].tolist() == [1, 0, 0, 1]
  assert abs(ref['entropy'][1].item() - torch.log(torch.tensor(4.0)).item()) < 1e-6 and abs(ref['logp'][1].item() + 1.3862943611198906) < 1e-12
  assert abs(ref['entropy'][3].item() - 0.6931471805599453) < 1e-12  # two columns of probability 1/2, two of 0
  for tile in (1, 2, 3, 4):  # tile 1: a tile that is all -inf is an empty record
    r = R.tilewise_fp32(L, tile)
    assert r['pred'].tolist() == [1, 0, 0, 1], tile
    for k in ('logp', 'entropy', 'lse'):
      assert torch.isfinite(r[k]).all(), (tile, k)
      assert (r[k].double() - ref[k]).abs().max().item() < 1e-6, (tile, k)
  worst = {'logp': 0.0, 'entropy': 0.0}
  for M, V in ((22, 8200), (22, 50280), (704, 8)):
    Lc, _ = PO.ce_inputs(M, V, seed=1000 + V)
    ref = R.predict_reference(Lc)
    r = R.tilewise_fp32(Lc, 128)
    assert torch.equal(r['pred'], ref['pred'])
    for k in worst:
      worst[k] = max(worst[k], (r[k].double() - ref[k]).abs().max().item())
  print(f'fp32 tile-wise restatement vs fp64: {worst}')
  assert worst['logp'] <= PO.BOUNDS['ce_loss'] / 7 and worst['entropy'] <= PO.BOUNDS['ce_loss'] / 7
