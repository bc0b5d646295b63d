"""CPU tests (no GPU) of cache extension: tests/extend_ref.py's staircase mask, split partition and combine equal
the unsplit masked softmax; the three entry points refuse their documented bad arguments before any HIP call; the workspace query is
positive and monotone; and the refusals of ops.kv_append_rope_rows / attn_extend / attn_extend_workspace, KVCache.advance_by,
Transformer.new_cache and Transformer.extend that need no GPU."""

import ctypes as C
import math
import os
import sys
import types
from collections import namedtuple

import numpy as np
import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib
from plainlm_amd import generate as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import extend_ref as E  # noqa: E402


def _lib_loaded():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


def _refuser(lib, name):
  def refused(*args):
    rc = getattr(lib, name)(*args)
    assert rc < 0, rc
    msg = (lib.plm_last_error_string() or b'').decode()
    assert name in msg, msg
    return rc, msg
  return refused


p = lambda: C.c_void_p(0x100000)  # noqa: E731  plausible, 16-byte aligned, never dereferenced
odd = lambda: C.c_void_p(0x100004)  # noqa: E731


# ---- the fp64 restatement -------------------------------------------------------------------------------------------------------------
def test_staircase_split_and_combine_restatement_equals_the_unsplit_masked_softmax():
  rng = np.random.default_rng(1)
  hd, n = 16, 6
  cases = [(0, 6), (0, 1), (5, 6), (5, 3), (13, 6), (7, 0), (0, 0), (1, 9)]  # (lens0, c): lens0 = 0, rows r >= c, c = 0, c beyond n (clamped)
  for lens0, c in cases:
    cc = min(c, n)
    L = lens0 + cc
    q = rng.standard_normal((n, hd)) * 3
    k, v = rng.standard_normal((L + 4, hd)), rng.standard_normal((L + 4, hd))
    k[L:], v[L:] = np.nan, np.nan  # the stale tail: neither route may touch it
    mask = E.staircase(lens0, cc, n, L)
    assert mask.shape == (n, L) and not mask[cc:].any()
    for r in range(cc):
      assert mask[r, :lens0 + r + 1].all() and not mask[r, lens0 + r + 1:].any()
    want_o, want_l = E.chunk_attention(q, k, v, lens0, cc)
    assert (want_o[cc:] == 0).all() and (want_l[cc:] == math.inf).all()
    assert np.isfinite(want_o).all() and np.isfinite(want_l[:cc]).all()
    for S in (1, 2, 7, 64):
      o, l = E.split_and_combine(q, k, v, lens0, cc, S)
      if S > L:  # empty splits are part of the case (every split is empty when L == 0)
        assert any(a == b for a, b in E.R.split_ranges(L, S))
      assert np.isfinite(o).all()
      assert (o[cc:] == 0).all() and (l[cc:] == math.inf).all(), (lens0, c, S)
      assert np.abs(o - want_o).max() <= 1e-12, (lens0, c, S)
      assert cc == 0 or np.abs(l[:cc] - want_l[:cc]).max() <= 1e-12, (lens0, c, S)
  # a late split holds keys that only the late rows see: for the early rows it is an empty partial, not a NaN
  q = rng.standard_normal((4, hd))
  k, v = rng.standard_normal((4, hd)), rng.standard_normal((4, hd))
  o, l = E.split_and_combine(q, k, v, 0, 4, 4)
  wo, wl = E.chunk_attention(q, k, v, 0, 4)
  assert np.abs(o - wo).max() <= 1e-12 and np.abs(l - wl).max() <= 1e-12
  assert np.abs(o[0] - v[0]).max() <= 1e-12  # row 0 sees its own key alone


# ---- the C ABI's refusals -------------------------------------------------------------------------------------------------------------
def test_attn_extend_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  refused = _refuser(lib, 'plm_attn_extend')
  big = 1 << 40
  # q, kv, ld_kv, lens0, n_new, out, lse, B, n, Tmax, nh, hd, splits, workspace, bytes, stream
  ok = [p(), p(), 384, p(), None, p(), None, 5, 7, 40, 3, 64, 2, p(), big, None]
  for i in (0, 1, 3, 5, 13):  # every pointer but n_new and lse
    a = list(ok)
    a[i] = None
    assert 'null pointer' in refused(*a)[1], i
  for hd in (0, 16, 48, 96, 256):
    a = list(ok)
    a[11] = hd
    assert 'head_dim' in refused(*a)[1], hd
  for n in (0, -3):
    a = list(ok)
    a[8] = n
    assert 'n >= 1' in refused(*a)[1], n
  a = list(ok)
  a[7], a[8] = 4, 1 << 29  # B * n = 2^31
  assert 'B*n < 2^31' in refused(*a)[1]
  for i in (7, 9, 10):  # B, Tmax, nh
    a = list(ok)
    a[i] = 0
    assert 'bad' in refused(*a)[1], i
  for i in (0, 1, 5, 13):
    a = list(ok)
    a[i] = odd()
    assert 'aligned' in refused(*a)[1], i
  for s in (-1, 65, 1000):
    a = list(ok)
    a[12] = s
    assert 'splits' in refused(*a)[1], s
  for ld in (383, 380, 388):  # shorter than a row, and not a multiple of 8
    a = list(ok)
    a[2] = ld
    assert 'row stride' in refused(*a)[1], ld
  for splits in (0, 1, 7, 64):
    need = lib.plm_attn_extend_workspace_bytes(5, 7, 3, 64, 40, splits)
    assert need > 0
    a = list(ok)
    a[12], a[14] = splits, need - 1
    rc, msg = refused(*a)
    assert rc == -4 and 'workspace' in msg, (splits, rc, msg)  # PLM_E_WORKSPACE


def test_kv_append_rope_rows_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  refused = _refuser(lib, 'plm_kv_append_rope_rows')
  # qkv, ld_qkv, lens0, n_new, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv, status, B, n, Tmax, nh, hd, stream
  ok = [p(), 576, p(), None, p(), p(), 40, p(), p(), 384, p(), 5, 7, 40, 3, 64, None]
  for i in (0, 2, 4, 5, 7, 8, 10):  # every pointer but n_new
    a = list(ok)
    a[i] = None
    assert 'null pointer' in refused(*a)[1], i
  for hd in (0, 16, 96):
    a = list(ok)
    a[15] = hd
    assert 'head_dim' in refused(*a)[1], hd
  for n in (0, -1):
    a = list(ok)
    a[12] = n
    assert 'n >= 1' in refused(*a)[1], n
  a = list(ok)
  a[11], a[12] = 2, 1 << 30
  assert 'B*n < 2^31' in refused(*a)[1]
  for i in (0, 4, 5, 7, 8):
    a = list(ok)
    a[i] = odd()
    assert 'aligned' in refused(*a)[1], i
  for i, ld in ((1, 568), (1, 580), (9, 376), (9, 388)):
    a = list(ok)
    a[i] = ld
    assert 'row strides' in refused(*a)[1], (i, ld)
  for i in (6, 11, 13, 14):  # rope_T, B, Tmax, nh
    a = list(ok)
    a[i] = 0
    assert 'bad' in refused(*a)[1], i


def test_extend_workspace_is_positive_and_monotone():
  lib = _lib_loaded()
  ws = lib.plm_attn_extend_workspace_bytes  # (B, n, nh, hd, Tmax, splits)
  for hd in (32, 64, 128):
    for splits in (1, 7, 64):  # a forced count: monotone in the chunk width and in the batch
      prev = 0
      for n in (1, 2, 8, 32, 33, 128, 129, 1000):
        b = ws(8, n, 12, hd, 1024, splits)
        assert b > 0 and b % 16 == 0 and b > prev, (hd, splits, n, b, prev)
        assert b >= 8 * 12 * splits * n * (hd + 2) * 4  # one fp32 (m, l, acc[hd]) per (sequence, head, split, chunk row)
        prev = b
      prev = 0
      for B in (1, 2, 5, 8, 64, 1000):
        b = ws(B, 8, 12, hd, 1024, splits)
        assert b > prev, (hd, splits, B)
        prev = b
    prev = 0
    for splits in range(1, 65):
      b = ws(8, 8, 12, hd, 1024, splits)
      assert b > prev, (hd, splits, b, prev)
      prev = b
    for n in (1, 8, 128, 129, 1000):  # automatic: positive, never more than the largest forced count, the same for every call
      b = ws(8, n, 12, hd, 1024, 0)
      assert 0 < b <= ws(8, n, 12, hd, 1024, 64) and b == ws(8, n, 12, hd, 1024, 0), (hd, n)
    for Tmax in (1, 37, 64, 65, 1024, 1 << 20):
      assert ws(8, 8, 12, hd, Tmax, 0) > 0
  bad = ((0, 8, 12, 64, 1024, 0), (8, 0, 12, 64, 1024, 0), (8, 8, 0, 64, 1024, 0), (8, 8, 12, 48, 1024, 0), (8, 8, 12, 64, 0, 0),
         (8, 8, 12, 64, 1024, -1), (8, 8, 12, 64, 1024, 65), (4, 1 << 29, 12, 64, 1024, 1))
  for args in bad:
    assert ws(*args) == 0, args


# ---- Python --------------------------------------------------------------------------------------------------------------------------
def test_ops_have_no_cpu_path():
  from plainlm_amd import ops
  bf = torch.bfloat16
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.kv_append_rope_rows(torch.zeros(6, 192, dtype=bf), torch.zeros(2, dtype=torch.int32), torch.zeros(8, 32), torch.zeros(8, 32),
                            torch.zeros(2, 8, 128, dtype=bf), 1)
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.attn_extend(torch.zeros(6, 64, dtype=bf), torch.zeros(2, 8, 128, dtype=bf), torch.zeros(2, dtype=torch.int32), 1)
  with pytest.raises(ValueError, match='unsupported shape'):
    ops.attn_extend_workspace(2, 0, 1, 64, 8, 0, 'cpu')  # the query needs no GPU: refused shapes size nothing
  with pytest.raises(ValueError, match='unsupported shape'):
    ops.attn_extend_workspace(2, 3, 1, 48, 8, 0, 'cpu')


def test_chunk_lens_and_advance_by():
  assert G.chunk_lens(None, 3, 5, 'cpu') == (5, None)
  adv, dev = G.chunk_lens((5, 0, 3), 3, 5, 'cpu')
  assert adv is dev and dev.dtype == torch.int32 and dev.tolist() == [5, 0, 3]
  adv, dev = G.chunk_lens(torch.tensor([1, 2, 5]), 3, 5, 'cpu')
  assert dev.dtype == torch.int32 and dev.tolist() == [1, 2, 5]
  for bad in ((5, 3), (5, 3, 1, 1), (6, 0, 0), (-1, 0, 0)):
    with pytest.raises(ValueError, match='token_lens'):
      G.chunk_lens(bad, 3, 5, 'cpu')
  # advance_by: one in-place add on [pos | lens], an int or an int32 [B] tensor
  cache = object.__new__(G.KVCache)
  cache._pl = torch.tensor([[-1, 4, 9], [0, 5, 10]], dtype=torch.int32)
  pl = cache._pl
  cache.advance_by(3)
  assert cache._pl is pl and cache.lens.tolist() == [3, 8, 13] and cache.pos.tolist() == [2, 7, 12]
  cache.advance_by(torch.tensor([5, 0, 1], dtype=torch.int32))
  assert cache._pl is pl and cache.lens.tolist() == [8, 8, 14] and cache.pos.tolist() == [7, 7, 13]
  cache.advance()  # the decode step's move is unchanged
  assert cache.lens.tolist() == [9, 9, 15]


def test_extend_and_new_cache_refusals_come_before_any_launch():
  EC = dict(model='transformer', vocab_size=512, seq_len=128, d_model=128, expand='8/3', n_layers=2, n_heads=2, mlp_class='glu',
            tie_embeddings=False)
  model, _ = P.construct_model(namedtuple('Config', EC.keys())(**EC))
  fake = types.SimpleNamespace(B=2)  # a cache is only asked for its batch before the device check
  ids = torch.zeros(2, 5, dtype=torch.int64)
  with torch.no_grad(), pytest.raises(RuntimeError, match='MI355X'):
    model.extend(ids, fake)
  for bad in (torch.zeros(3, 5, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), torch.zeros(2, 0, dtype=torch.int64),
              torch.zeros(2, 5, 1, dtype=torch.int64)):
    with pytest.raises(ValueError, match=r'not a \[B, n\] chunk'):
      model.extend(bad, fake)
  with pytest.raises(TypeError, match='int64'):
    model.extend(ids.int(), fake)
  with pytest.raises(ValueError, match='max_len'):
    model.new_cache(2, max_len=129)
  with pytest.raises(ValueError, match='max_len'):
    model.new_cache(2, max_len=0)
  with pytest.raises(ValueError, match='B >= 1'):
    model.new_cache(0)
  with pytest.raises(RuntimeError, match='MI355X'):
    model.new_cache(2)
  with pytest.raises(RuntimeError, match='MI355X'):
    model.new_cache(2, max_len=64)
  mx = P.Transformer(P.ModelConfig(vocab_size=512, seq_len=128, dim=128, expand=8 / 3, n_layers=1, n_heads=2, linear_precision='mxfp8'))
  with pytest.raises(NotImplementedError, match='linear_precision'):
    mx.extend(ids, fake)
  with pytest.raises(NotImplementedError, match='linear_precision'):
    mx.new_cache(2)
