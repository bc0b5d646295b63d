"""The wide fused layer without a GPU: its entry points' argument refusals (every check comes before any HIP
call), the workspace query, and the refusals of Transformer.step_ragged / serve under fused='wide'."""

import inspect
import os
import sys

import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib, generate as G, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_paged_host import _cfg, _rc, p  # noqa: E402

# name -> (good arguments, [(index, bad value, word of the message)])
CALLS = {
  # x, A, W, M, N, K, stream
  'plm_wide_gemm_residual_bf16': ([p(), p(), p(), 65, 768, 2048, None],
                                  [(3, 257, 'rows'), (3, 0, 'rows'), (5, 48, 'unsupported shape'), (4, 24, 'unsupported shape'), (1, None, 'null'),
                                   (2, p(4104), 'aligned')]),
  # x, norm_w, eps, w_fc1, act, M, d, hidden, kind, stream
  'plm_wide_norm_fc1_act_bf16': ([p(), p(), 1e-6, p(), p(), 65, 768, 2048, 0, None],
                                 [(5, 257, 'rows'), (6, 48, 'd = 48'), (7, 40, 'hidden = 40'), (8, 3, 'mlp_kind'), (4, None, 'null'),
                                  (0, p(4104), 'aligned')]),
  # x, norm_w, eps, w_qkv, lens0, cu_rows, row_seq, cos, sin, rope_T, q_out, pool, ld_kv, table, status, R, B, max_pages, n_pages, nh, hd, stream
  'plm_ragged_norm_qkv_append_paged_wide_bf16': ([p(), p(), 1e-6, p(), p(), p(), p(), p(), p(), 512, p(), p(), 256, p(), p(), 65, 3, 8, 30, 2, 64, None],
                                                 [(13, None, 'null'), (5, None, 'null'), (11, None, 'null'), (20, 48, 'head_dim'), (12, 250, 'stride'),
                                                  (15, 257, 'rows'), (16, 0, 'bad shape'), (17, 0, 'max_pages'), (18, 0, 'n_pages'),
                                                  (10, p(4104), 'aligned')]),
  # x, norms x2, eps, w x4, lens0, cu_rows, row_seq, cos, sin, rope_T, pool, ld_kv, table, status, R, B, NT, Lcap, max_pages, n_pages, nh, hd,
  # hidden, kind, ws, bytes, stream
  'plm_ragged_layer_paged_wide_bf16': ([p(), p(), p(), 1e-6, p(), p(), p(), p(), p(), p(), p(), p(), p(), 512, p(), 256, p(), p(), 65, 3, 4, 512, 8, 30,
                                        2, 64, 352, 0, p(), 1 << 24, None],
                                       [(16, None, 'null'), (9, None, 'null'), (10, None, 'null'), (28, None, 'null'), (25, 96, 'head_dim'),
                                        (15, 128, 'stride'), (21, 513, 'Lcap'), (18, 257, 'rows'), (20, 66, 'NT'), (20, 0, 'NT'), (19, 0, 'bad shape'),
                                        (26, 40, 'hidden = 40'), (27, 3, 'mlp_kind'), (28, p(4104), 'aligned')]),
}


@pytest.mark.parametrize('name', list(CALLS))
def test_entry_points_refuse_bad_arguments_without_a_gpu(name):
  assert name in _lib.header_functions() and name in _lib.SIGNATURES
  good, bad = CALLS[name]
  for i, v, word in bad:
    args = list(good)
    args[i] = v
    rc, msg = _rc(name, *args)
    assert rc == -1 and name in msg and word in msg, (i, rc, msg)
  if 'layer' in name:  # a short workspace is refused with its own code, still before any HIP call
    args = list(good)
    args[-2] = 16
    rc, msg = _rc(name, *args)
    assert rc == -4 and 'workspace' in msg, (rc, msg)


def test_the_workspace_query_and_the_abi():
  lib, r16 = _lib.load(), lambda n: (n + 15) // 16 * 16
  for R, nh, hd, hidden, Lcap in ((1, 3, 32, 288, 64), (65, 2, 64, 352, 512), (256, 12, 64, 2048, 1024)):
    att = lib.plm_attn_ragged_paged_workspace_bytes(R, nh, hd, Lcap)
    assert att > 0 and lib.plm_ragged_layer_paged_wide_workspace_bytes(R, nh, hd, hidden, Lcap) == 2 * r16(R * nh * hd * 2) + r16(R * hidden * 2) + att
  for bad in ((257, 2, 64, 352, 512), (0, 2, 64, 352, 512), (65, 2, 48, 352, 512), (65, 2, 64, 40, 512), (65, 2, 64, 352, 0)):
    assert lib.plm_ragged_layer_paged_wide_workspace_bytes(*bad) == 0, bad
  assert ops.FUSED_WIDE_MAX_ROWS == 256 and ops.ragged_layer_paged_wide.__module__ == 'plainlm_amd.ops_wide'
  assert _lib.EXPECTED_ABI == 112 == lib.plm_version()  # additive: the number did not move


def test_step_ragged_and_serve_refusals_under_wide():
  m = P.Transformer(_cfg())
  pool = G.PagePool(1, 8, 2, 64, 'cpu')
  cache = G.PagedKVCache(pool, 3, 512)
  cache.admit(0)
  cache.admit(1)
  with pytest.raises(ValueError, match='at most 256 packed rows, got 257'):
    m.step_ragged(torch.zeros(257, dtype=torch.int64), [256, 1, 0], cache, fused='wide')
  for bad in ('Wide', 'skinny', 1, None):
    with pytest.raises(ValueError, match="fused must be False, True or 'wide'"):
      m.step_ragged(torch.zeros(6, dtype=torch.int64), [5, 1, 0], cache, fused=bad)
  assert pool.n_free == 8 and cache.bound == [0, 0, 0]  # a refused step takes no page
  with pytest.raises(RuntimeError, match='MI355X only'):  # every refusal above came before this one
    m.step_ragged(torch.zeros(40, dtype=torch.int64), [39, 1, 0], cache, fused='wide')
  tok = torch.zeros(6, dtype=torch.int64)
  with pytest.raises(ValueError, match=r"at most 256 rows a step, got max_batch 8 \+ prefill_chunk 249"):
    m.serve([tok], 4, 8, fused='wide', prefill_chunk=249)
  with pytest.raises(ValueError, match="fused='wide' needs prefill_chunk"):
    m.serve([tok], 4, 8, fused='wide')
  with pytest.raises(ValueError, match="fused must be False, True or 'wide'"):
    m.serve([tok], 4, 8, fused='narrow', prefill_chunk=8)
  with pytest.raises(RuntimeError, match='MI355X only'):
    m.serve([tok], 4, 8, fused='wide', prefill_chunk=248)
  names = list(inspect.signature(P.Transformer.serve).parameters)
  assert names == ['self', 'prompts', 'max_new_tokens', 'max_batch', 'pool', 'eos_id', 'fused', 'temperature', 'top_k', 'top_p', 'sample', 'seed',
                   'prefill_chunk']
