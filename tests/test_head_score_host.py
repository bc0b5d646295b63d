"""CPU tests (no GPU) of the forward-only scoring head: the two new C entry points refuse bad arguments before any HIP call, the ABI
number did not move, the scoring instantiations of the persistent NT kernel meet the plain kernel's register / K-loop bar, and the
Python layers validate their options."""

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


def _lib_loaded():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


def test_head_score_entry_points_refuse_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  assert lib.plm_version() == 112  # the ABI the signatures were written for
  p = lambda: C.c_void_p(0x100000)  # plausible, never dereferenced
  def refused(*args):
    rc = lib.plm_head_score_bf16(*args)
    assert rc < 0, rc
    msg = (lib.plm_last_error_string() or b'').decode()
    assert 'plm_head_score_bf16' in msg, msg
    return rc, msg
  big = 1 << 40
  assert 'null pointer' in refused(None, 768, p(), 768, p(), p(), None, 512, 1024, 768, p(), big, None)[1]
  assert 'null pointer' in refused(p(), 768, p(), 768, p(), p(), None, 512, 1024, 768, None, big, None)[1]
  assert 'K % 64' in refused(p(), 776, p(), 776, p(), p(), None, 512, 1024, 776, p(), big, None)[1]
  assert 'multiples of 8' in refused(p(), 772, p(), 768, p(), p(), None, 512, 1024, 768, p(), big, None)[1]
  assert 'aligned' in refused(C.c_void_p(0x100002), 768, p(), 768, p(), p(), None, 512, 1024, 768, p(), big, None)[1]
  need = lib.plm_head_score_workspace_bytes(512, 1024, 768)
  rc, msg = refused(p(), 768, p(), 768, p(), p(), None, 512, 1024, 768, p(), need - 1, None)
  assert rc == -4 and 'workspace' in msg  # PLM_E_WORKSPACE


def test_head_score_workspace_is_positive_monotone_and_small():
  lib = _lib_loaded()
  prev = 0
  for M in (1, 8, 300, 511, 512, 1000, 4096, 8192, 32768, 65536):
    n = lib.plm_head_score_workspace_bytes(M, 50280, 768)
    assert n > 0 and n >= prev, (M, n, prev)
    prev = n
  assert lib.plm_head_score_workspace_bytes(0, 50280, 768) == 0
  # the bench shape: a few per cent of the [M, out_pad] bf16 logits it replaces
  assert lib.plm_head_score_workspace_bytes(32768, 50280, 768) <= 0.04 * 32768 * 50304 * 2


@pytest.mark.timeout(600)
def test_scoring_kernels_meet_the_plain_nt_kernels_isa_bar():
  """tools/isa_scan.py on csrc/gemm_big.hip: the four SCORE instantiations of gemm_nt_big_kernel (last template argument true) have no
  spill and no scratch, at most 256 VGPRs, and at most one unconditional vmcnt(0) inside the K loop - the main loop is the plain one."""
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'isa_scan.py'), 'gemm_big.hip'], capture_output=True, text=True, timeout=540)
  assert r.returncode == 0, r.stderr[-2000:]
  lines = r.stdout.splitlines()
  seen = {}
  for i, l in enumerate(lines):
    if 'gemm_nt_big_kernel' in l and re.search(r'false, false, false, false, true>$', l.strip()):
      seen[l.strip()] = (ast.literal_eval(lines[i + 1].strip()), lines[i + 2])
  assert len(seen) == 4, sorted(seen)  # 256x256, 256x128, 256x192, 128x192
  for k, (meta, span) in seen.items():
    assert meta['vspill'] == 0 and meta['sspill'] == 0 and meta['scratch'] == 0 and meta['vgpr'] <= 256, (k, meta)
    m = re.search(r'unconditional vmcnt\(0\): (\d+)', span)
    assert m and int(m.group(1)) <= 1, (k, span)
    m = re.search(r'scratch_: (\d+)', span)
    assert m and int(m.group(1)) == 0, (k, span)


def _cfg(**over):
  EC = dict(model='transformer', vocab_size=512, seq_len=128, d_model=128, expand='8/3', n_layers=2, n_heads=2,
            mlp_class='glu', tie_embeddings=False)
  EC.update(over)
  return namedtuple('Config', EC.keys())(**EC)


def test_eval_head_validation_and_score_has_no_cpu_path():
  assert engine.check_eval_head('logits') == 'logits' and engine.check_eval_head('fused') == 'fused'
  with pytest.raises(ValueError, match='eval_head'):
    engine.check_eval_head('fast')
  model, _ = P.construct_model(_cfg())
  ecfg = namedtuple('C', ['seq_len', 'grad_accumulation_steps', 'grad_clip', 'dtype', 'eval_head'])(128, 1, 1.0, 'bfloat16', 'fast')
  with pytest.raises(ValueError, match='eval_head'):  # the option is checked before the device
    P.TorchEngine(model, ecfg, 'cpu', None, None)
  ids = torch.zeros(1, 128, dtype=torch.int64)
  with pytest.raises(RuntimeError, match='MI355X'):
    model.score(ids, ids)
  with torch.no_grad(), pytest.raises(RuntimeError, match='MI355X'):
    model.token_logprobs(ids, ids)
  with pytest.raises(ValueError, match='reduction'):
    model.score(ids, ids, reduction='avg')
  from plainlm_amd import ops
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.head_score(torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(16, 64, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.int64))
