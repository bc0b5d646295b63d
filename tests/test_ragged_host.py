"""Ragged steps without a GPU: ops.ragged_plan, the new entry points' argument refusals (every check comes before
any HIP call), and the refusals of Transformer.step_ragged / serve(prefill_chunk=...)."""

import inspect
import os
import sys

import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib, generate as G, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_paged_host import _cfg, _rc, p  # noqa: E402


@pytest.mark.parametrize('counts', [[1], [0, 3, 0], [32, 33, 64], [1, 0, 70, 1, 0, 5], [0, 0, 2]])
def test_ragged_plan_against_its_restatement(counts):
  cu, row_seq, last_row, NT = ops.ragged_plan(counts)
  assert cu.tolist() == [sum(counts[:b]) for b in range(len(counts) + 1)]
  assert row_seq.tolist() == [b for b, c in enumerate(counts) for _ in range(c)]
  assert last_row.tolist() == [sum(counts[:b + 1]) - 1 if c else -1 for b, c in enumerate(counts)] and NT == sum((c + 31) // 32 for c in counts)
  assert all(t.dtype == torch.int32 and not t.is_cuda for t in (cu, row_seq, last_row)) and ops.ragged_plan.__module__ == 'plainlm_amd.ops_ragged'


# name -> (good arguments, [(index, bad value, word of the message)])
CALLS = {
  # qkv, ld_qkv, lens0, cu_rows, row_seq, cos, sin, rope_T, q_out, pool, ld_kv, table, status, R, B, max_pages, n_pages, nh, hd, stream
  'plm_kv_paged_append_rope_packed': ([p(), 384, p(), p(), p(), p(), p(), 256, p(), p(), 256, p(), p(), 40, 3, 4, 9, 2, 64, None],
                                      [(0, None, 'null'), (3, None, 'null'), (4, None, 'null'), (18, 48, 'head_dim'), (10, 250, 'stride'),
                                       (1, 380, 'stride'), (13, 0, 'bad shape'), (14, 0, 'bad shape'), (15, 0, 'max_pages'), (16, 0, 'n_pages'),
                                       (9, p(4104), 'aligned'), (3, p(4098), 'aligned')]),
  # q, pool, ld_kv, table, lens0, cu_rows, row_seq, out, lse, R, B, NT, Lcap, max_pages, n_pages, nh, hd, workspace, bytes, stream
  'plm_attn_ragged_paged': ([p(), p(), 256, p(), p(), p(), p(), p(), None, 40, 3, 4, 256, 4, 9, 2, 64, p(), 1 << 22, None],
                            [(0, None, 'null'), (5, None, 'null'), (17, None, 'null'), (16, 96, 'head_dim'), (2, 128, 'stride'), (12, 257, 'Lcap'),
                             (12, 0, 'Lcap'), (11, 0, 'NT'), (11, 41, 'NT'), (9, 0, 'bad shape'), (10, 0, 'bad shape'), (7, p(4104), 'aligned')]),
  # x, norm_w, eps, w_qkv, lens0, cu_rows, row_seq, cos, sin, rope_T, q_out, pool, ld_kv, table, status, R, B, max_pages, n_pages, nh, hd, stream
  'plm_ragged_norm_qkv_append_paged_bf16': ([p(), p(), 1e-6, p(), p(), p(), p(), p(), p(), 256, p(), p(), 256, p(), p(), 7, 3, 4, 9, 2, 64, None],
                                            [(13, None, 'null'), (5, None, 'null'), (11, None, 'null'), (20, 48, 'head_dim'), (12, 250, 'stride'),
                                             (15, 33, 'rows'), (16, 0, 'bad shape'), (17, 0, 'max_pages'), (18, 0, 'n_pages')]),
  # x, norms x2, eps, w x4, lens0, cu_rows, row_seq, cos, sin, rope_T, pool, ld_kv, table, status, R, B, NT, Lcap, max_pages, n_pages, nh, hd,
  # hidden, kind, ws, bytes, stream
  'plm_ragged_layer_paged_bf16': ([p(), p(), p(), 1e-6, p(), p(), p(), p(), p(), p(), p(), p(), p(), 256, p(), 256, p(), p(), 7, 3, 2, 256, 4, 9, 2,
                                   64, 352, 0, p(), 1 << 22, None],
                                  [(16, None, 'null'), (9, None, 'null'), (10, None, 'null'), (25, 96, 'head_dim'), (15, 128, 'stride'),
                                   (21, 257, 'Lcap'), (18, 33, 'rows'), (20, 8, 'NT'), (20, 0, 'NT'), (19, 0, 'bad shape'), (27, 3, 'mlp_kind')]),
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
  if 'attn' in name or 'layer' in name:  # a short workspace is refused with its own code, still before any HIP call
    args = list(good)
    args[-2] = 16
    rc, msg = _rc(name, *args)
    assert rc == -4 and 'workspace' in msg, (rc, msg)


def test_the_chunk_cap_and_the_workspace_queries():
  lib, Cn = _lib.load(), ops.KV_PAGED_CHUNK
  assert lib.plm_attn_ragged_paged_workspace_bytes(40, 2, 64, 64 * Cn) == 40 * 2 * 64 * (2 + 64) * 4
  assert lib.plm_attn_ragged_paged_workspace_bytes(40, 2, 64, 64 * Cn + 1) == 0 and lib.plm_attn_ragged_paged_workspace_bytes(40, 2, 48, 256) == 0
  rc, msg = _rc('plm_attn_ragged_paged', p(), p(), 256, p(), p(), p(), p(), p(), None, 40, 3, 4, 64 * Cn + 1, 65 * Cn // 64, 9, 2, 64, p(), 1 << 30, None)
  assert rc == -1 and 'chunks' in msg, (rc, msg)
  assert lib.plm_ragged_layer_paged_workspace_bytes(33, 2, 64, 352, 256) == 0 and lib.plm_ragged_layer_paged_workspace_bytes(32, 2, 64, 352, 256) > 0
  assert _lib.EXPECTED_ABI == 112 == lib.plm_version()  # additive: the number did not move


def test_step_ragged_and_serve_refusals_by_name():
  m = P.Transformer(_cfg())
  pool = G.PagePool(1, 4, 2, 64, 'cpu')
  cache = G.PagedKVCache(pool, 3, 64)
  cache.admit(0)
  cache.admit(1)
  with pytest.raises(ValueError, match='holds a sequence'):
    cache.admit(0)
  assert cache.pos.tolist() == [-1, -1, 0] and cache.lens.tolist() == [0, 0, 0] and cache.live.tolist() == [1, 1, 0] and pool.n_free == 4
  tok = torch.zeros(6, dtype=torch.int64)
  with pytest.raises(TypeError, match='PagedKVCache'):
    m.step_ragged(tok, [5, 1, 0], G.KVCache(1, 3, 64, 2, 64, 'cpu'))
  with pytest.raises(ValueError, match='mxfp8'):
    P.Transformer(_cfg(linear_precision='mxfp8')).step_ragged(tok, [5, 1, 0], cache)
  with pytest.raises(TypeError, match=r'int64 \[R\]'):
    m.step_ragged(tok.view(2, 3), [5, 1, 0], cache)
  for counts, word in (([5, 2, 0], 'sum to 7'), ([6, 0], 'need 3 counts'), ([7, -1, 0], 'none negative'), ([5, 0, 1], 'slot 2 is idle')):
    with pytest.raises(ValueError, match=word):
      m.step_ragged(tok, counts, cache)
  with pytest.raises(ValueError, match='do not fit max_len 64'):
    m.step_ragged(torch.zeros(65, dtype=torch.int64), [65, 0, 0], cache)
  with pytest.raises(ValueError, match='at most 32 packed rows'):
    m.step_ragged(torch.zeros(33, dtype=torch.int64), [32, 1, 0], cache, fused=True)
  assert pool.n_free == 4 and cache.bound == [0, 0, 0]  # a refused step takes no page
  with pytest.raises(RuntimeError, match='MI355X only'):  # every refusal above came before this one
    m.step_ragged(tok, [5, 1, 0], cache)
  for C in (0, -1, 2.0, True):
    with pytest.raises(ValueError, match='prefill_chunk must be None or an int >= 1'):
      m.serve([tok], 4, 2, prefill_chunk=C)
  with pytest.raises(ValueError, match=r'max_batch 8 \+ prefill_chunk 25'):
    m.serve([tok], 4, 8, fused=True, prefill_chunk=25)
  with pytest.raises(ValueError, match='greedy only'):
    m.serve([tok], 4, 2, prefill_chunk=4, top_k=5)


def test_serve_keeps_its_parameters_and_takes_prefill_chunk_last():
  names = list(inspect.signature(P.Transformer.serve).parameters)
  assert names == ['self', 'prompts', 'max_new_tokens', 'max_batch', 'pool', 'eos_id', 'fused', 'temperature', 'top_k', 'top_p', 'sample', 'seed',
                   'prefill_chunk']
  assert inspect.signature(P.Transformer.serve).parameters['prefill_chunk'].default is None
