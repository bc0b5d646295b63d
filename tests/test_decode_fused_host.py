"""CPU tests (no GPU) of the fused decode step: its entry points refuse bad arguments before any HIP call (the
header, the binding table and the library are compared in tests/test_host_logic.py), the layer's workspace query is positive, a function
of the shapes alone and monotone in B and Tmax, and the ``fused`` keyword's own refusals need no GPU."""

import ctypes as C
import os

import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib, ops
from plainlm_amd import generate as G


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


def swapped(ok, i, v):
  a = list(ok)
  a[i] = v
  return a


def test_the_new_entry_points_are_declared_bound_and_exported():
  lib = _lib_loaded()
  for name in ('plm_decode_norm_qkv_append_bf16', 'plm_decode_gemm_residual_bf16', 'plm_decode_norm_fc1_act_bf16',
               'plm_decode_layer_workspace_bytes', 'plm_decode_layer_bf16'):
    assert name in _lib.header_functions() and name in _lib.SIGNATURES and hasattr(lib, name), name
  assert _lib.EXPECTED_ABI == 112 == lib.plm_version()  # additive: the number did not move
  assert ops.FUSED_DECODE_MAX_ROWS == 32


def test_norm_qkv_append_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  refused = _refuser(lib, 'plm_decode_norm_qkv_append_bf16')
  # x, norm_w, eps, w_qkv, pos, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv, status, B, Tmax, nh, hd, stream
  ok = [p(), p(), 1e-6, p(), p(), p(), p(), 40, p(), p(), 384, p(), 5, 40, 3, 64, None]
  for i in (0, 1, 3, 4, 5, 6, 8, 9, 11):
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
  for B in (0, -1, 33, 1000):
    assert 'rows' in refused(*swapped(ok, 12, B))[1], B
  for hd in (0, 16, 48, 96, 256):
    assert 'head_dim' in refused(*swapped(ok, 15, hd))[1], hd
  for i in (7, 13, 14):  # rope_T, Tmax, nh
    assert 'bad shape' in refused(*swapped(ok, i, 0))[1], i
  for ld in (383, 376, 388):
    assert 'row stride' in refused(*swapped(ok, 10, ld))[1], ld
  for i in (0, 1, 3, 8, 9):
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i
  assert refused(*swapped(ok, 12, 33))[0] == -1  # PLM_E_INVALID


def test_gemm_residual_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  refused = _refuser(lib, 'plm_decode_gemm_residual_bf16')
  # x, A, W, M, N, K, stream
  ok = [p(), p(), p(), 8, 768, 2048, None]
  for i in (0, 1, 2):
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i
  for M in (0, 33):
    assert 'rows' in refused(*swapped(ok, 3, M))[1], M
  for N in (0, 8, 776, 1 << 20):
    assert 'unsupported shape' in refused(*swapped(ok, 4, N))[1], N
  for K in (0, 16, 784, 2064, 1 << 20):  # d % 32 != 0
    assert 'unsupported shape' in refused(*swapped(ok, 5, K))[1], K


def test_norm_fc1_act_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  refused = _refuser(lib, 'plm_decode_norm_fc1_act_bf16')
  # x, norm_w, eps, w_fc1, act, M, d, hidden, mlp_kind, stream
  ok = [p(), p(), 1e-6, p(), p(), 8, 768, 2048, 0, None]
  for i in (0, 1, 3, 4):
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i
  for M in (0, 33):
    assert 'rows' in refused(*swapped(ok, 5, M))[1], M
  for kind in (-1, 3, 7):
    assert 'mlp_kind' in refused(*swapped(ok, 8, kind))[1], kind
  for d in (0, 16, 784):
    assert 'd = ' in refused(*swapped(ok, 6, d))[1], d
  for h in (0, 8, 2056):
    assert 'hidden' in refused(*swapped(ok, 7, h))[1], h
  for kind in (0, 1, 2):  # every known kind passes the same checks up to the next refusal
    assert 'rows' in refused(*swapped(swapped(ok, 8, kind), 5, 33))[1], kind


def test_decode_layer_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  refused = _refuser(lib, 'plm_decode_layer_bf16')
  big = 1 << 40
  # 0 x, 1 attn_norm_w, 2 mlp_norm_w, 3 eps, 4 w_qkv, 5 w_out, 6 w_fc1, 7 w_fc2, 8 pos, 9 lens, 10 rope_cos, 11 rope_sin, 12 rope_T, 13 kv,
  # 14 ld_kv, 15 status, 16 B, 17 Tmax, 18 nh, 19 hd, 20 hidden, 21 mlp_kind, 22 splits, 23 workspace, 24 bytes, 25 stream
  ok = [p(), p(), p(), 1e-6, p(), p(), p(), p(), p(), p(), p(), p(), 40, p(), 384, p(), 5, 40, 3, 64, 512, 0, 0, p(), big, None]
  for i in (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 23):
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
  for B in (0, 33):
    assert 'rows' in refused(*swapped(ok, 16, B))[1], B
  for hd in (16, 48, 96):
    assert 'head_dim' in refused(*swapped(ok, 19, hd))[1], hd
  for h in (0, 8, 520):
    assert 'hidden' in refused(*swapped(ok, 20, h))[1], h
  for kind in (-1, 3):
    assert 'mlp_kind' in refused(*swapped(ok, 21, kind))[1], kind
  for s in (-1, 65):
    assert 'splits' in refused(*swapped(ok, 22, s))[1], s
  for ld in (383, 376, 388):
    assert 'row stride' in refused(*swapped(ok, 14, ld))[1], ld
  for i in (0, 1, 2, 4, 5, 6, 7, 13, 23):
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i
  for i in (12, 17, 18):
    assert refused(*swapped(ok, i, 0))[0] == -1, i
  for splits in (0, 1, 7, 64):
    need = lib.plm_decode_layer_workspace_bytes(5, 3, 64, 512, 40, splits)
    assert need > 0
    rc, msg = refused(*swapped(swapped(ok, 22, splits), 24, need - 1))
    assert rc == -4 and 'workspace' in msg, (splits, rc, msg)  # PLM_E_WORKSPACE


def test_d_not_a_multiple_of_32_is_refused():
  """head dims are multiples of 32, so d % 32 != 0 cannot be reached through (nh, hd) of the qkv stage; the stages that take d or K
  as a number refuse it."""
  lib = _lib_loaded()
  assert 'd = ' in _refuser(lib, 'plm_decode_norm_fc1_act_bf16')(p(), p(), 1e-6, p(), p(), 8, 48, 512, 0, None)[1]
  assert 'unsupported shape' in _refuser(lib, 'plm_decode_gemm_residual_bf16')(p(), p(), p(), 8, 48, 48, None)[1]


def test_layer_workspace_is_positive_and_monotone_in_B_and_Tmax():
  lib = _lib_loaded()
  ws = lib.plm_decode_layer_workspace_bytes
  for hd in (32, 64, 128):
    for splits in (0, 1, 7, 64):
      prev = 0
      for B in (1, 2, 5, 8, 16, 17, 32):
        n = ws(B, 12, hd, 2048, 1024, splits)
        # q, attention output, activation, then what plm_attn_decode asks for: nothing else, every part a multiple of 16 bytes
        want = 2 * ((B * 12 * hd * 2 + 15) // 16 * 16) + (B * 2048 * 2 + 15) // 16 * 16 + lib.plm_attn_decode_workspace_bytes(B, 12, hd, 1024, splits)
        assert n == want and n % 16 == 0 and n > prev, (hd, splits, B, n, want, prev)
        prev = n
      prev = 0
      for Tmax in (1, 4, 37, 64, 65, 200, 1024, 8192, 1 << 20):
        n = ws(8, 12, hd, 2048, Tmax, splits)
        assert n > 0 and n >= prev, (hd, splits, Tmax, n, prev)
        prev = n
  for bad in ((0, 12, 64, 2048, 1024, 0), (33, 12, 64, 2048, 1024, 0), (8, 12, 48, 2048, 1024, 0), (8, 12, 64, 2040, 1024, 0),
              (8, 12, 64, 2048, 0, 0), (8, 12, 64, 2048, 1024, 65), (8, 0, 64, 2048, 1024, 0)):
    assert ws(*bad) == 0, bad


def test_fused_keyword_refusals_need_no_gpu():
  with pytest.raises(ValueError, match='leave fused off'):
    G.check_fused('decode_step', 33, 768)
  with pytest.raises(ValueError, match='leave fused off'):
    G.check_fused('generate_fused', 8, 48)
  G.check_fused('generate_fused', 32, 768)
  # guard's refusals come first, in their pinned order: CPU tokens are refused before the batch size is looked at
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=1, n_heads=2, mlp='glu'))
  with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
    m.generate_fused(torch.zeros(33, 8, dtype=torch.int64), 4)
  import inspect
  assert list(inspect.signature(m.generate_fused).parameters) == list(inspect.signature(m.generate).parameters)  # generate's own list, unchanged
  assert 'fused' not in inspect.signature(m.generate).parameters and 'fused' in inspect.signature(m.decode_step).parameters
  with pytest.raises(TypeError, match='int64'):
    m.decode_step(torch.zeros(33, dtype=torch.int32), None, fused=True)
