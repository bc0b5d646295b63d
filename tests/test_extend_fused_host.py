"""CPU tests (no GPU) of the fused extend: its three entry points refuse bad arguments before any HIP call, with
never-dereferenced pointers as tests/test_decode_fused_host.py does it; the layer's workspace query is 0 on refused shapes, a function of
its arguments alone and monotone in B*n and Tmax; and the ``fused`` keyword of ``extend``, ``check_fused_rows``, ``generate_lookup_fused``
and ``_LookupSession(..., fused=True)`` need no GPU for their host logic."""

import ctypes as C
import inspect
import os
import sys

import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib, ops
from plainlm_amd import generate as G

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_lookup_host as LH  # noqa: E402  the fake model, cache and lookup of the session tests


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


def swapped(ok, *pairs):
  a = list(ok)
  for i, v in zip(pairs[::2], pairs[1::2]):
    a[i] = v
  return a


def test_the_new_entry_points_are_declared_bound_and_exported():
  lib = _lib_loaded()
  for name in ('plm_extend_norm_qkv_append_bf16', 'plm_extend_layer_workspace_bytes', 'plm_extend_layer_bf16'):
    assert name in _lib.header_functions() and name in _lib.SIGNATURES and hasattr(lib, name), name
  assert _lib.EXPECTED_ABI == 112 == lib.plm_version()  # additive: the number did not move
  assert ops.FUSED_EXTEND_MAX_ROWS == 32 and ops.FUSED_DECODE_MAX_ROWS == 32  # the latter still
  for name in ('extend_norm_qkv_append', 'extend_layer_workspace', 'extend_layer'):
    assert getattr(ops, name).__module__ == 'plainlm_amd.ops_decode', name  # re-exported by ops, defined next to decode_layer


def test_extend_norm_qkv_append_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  refused = _refuser(lib, 'plm_extend_norm_qkv_append_bf16')
  # 0 x, 1 norm_w, 2 eps, 3 w_qkv, 4 lens0, 5 n_new, 6 rope_cos, 7 rope_sin, 8 rope_T, 9 q_out, 10 kv, 11 ld_kv, 12 status, 13 B, 14 n,
  # 15 Tmax, 16 nh, 17 hd, 18 stream
  ok = [p(), p(), 1e-6, p(), p(), p(), p(), p(), 40, p(), p(), 384, p(), 5, 3, 40, 3, 64, None]
  for i in (0, 1, 3, 4, 6, 7, 9, 10, 12):  # every pointer but n_new, lens0 among them
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
  for B, n in ((0, 3), (-1, 3), (33, 1), (1, 33), (4, 9), (11, 3), (5, 0), (5, -2), (1 << 40, 1 << 40), (1000, 1)):  # B*n of 0 and 33, n = 0
    rc, msg = refused(*swapped(ok, 13, B, 14, n))
    assert rc == -1 and 'rows' in msg, (B, n, msg)
  for hd in (0, 16, 48, 96, 256):
    assert 'head_dim' in refused(*swapped(ok, 17, hd))[1], hd
  for i in (8, 15, 16):  # rope_T, Tmax, nh
    assert 'bad shape' in refused(*swapped(ok, i, 0))[1], i
  for ld in (383, 376, 388):
    assert 'row stride' in refused(*swapped(ok, 11, ld))[1], ld
  for i in (0, 1, 3, 9, 10):
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i
  # NULL n_new is no refusal of its own: with it the call gets as far as the next bad argument
  assert 'head_dim' in refused(*swapped(ok, 5, None, 17, 48))[1]
  # the last shapes that are served pass every check up to the next refusal
  for B, n in ((32, 1), (1, 32), (4, 8), (8, 4), (2, 16)):
    assert 'head_dim' in refused(*swapped(ok, 13, B, 14, n, 17, 48))[1], (B, n)


def test_extend_layer_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  refused = _refuser(lib, 'plm_extend_layer_bf16')
  big = 1 << 40
  # 0 x, 1 attn_norm_w, 2 mlp_norm_w, 3 eps, 4 w_qkv, 5 w_out, 6 w_fc1, 7 w_fc2, 8 lens0, 9 n_new, 10 rope_cos, 11 rope_sin, 12 rope_T,
  # 13 kv, 14 ld_kv, 15 status, 16 B, 17 n, 18 Tmax, 19 nh, 20 hd, 21 hidden, 22 mlp_kind, 23 splits, 24 workspace, 25 bytes, 26 stream
  ok = [p(), p(), p(), 1e-6, p(), p(), p(), p(), p(), p(), p(), p(), 40, p(), 384, p(), 5, 3, 40, 3, 64, 512, 0, 0, p(), big, None]
  for i in (0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 13, 15, 24):
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
  for B, n in ((0, 3), (33, 1), (1, 33), (4, 9), (5, 0), (5, -1)):
    rc, msg = refused(*swapped(ok, 16, B, 17, n))
    assert rc == -1 and 'rows' in msg, (B, n, msg)
  for hd in (16, 48, 96):
    assert 'head_dim' in refused(*swapped(ok, 20, hd))[1], hd
  for h in (0, 8, 520):
    assert 'hidden' in refused(*swapped(ok, 21, h))[1], h
  for kind in (-1, 3):
    assert 'mlp_kind' in refused(*swapped(ok, 22, kind))[1], kind
  for s in (-1, 65):
    assert 'splits' in refused(*swapped(ok, 23, s))[1], s
  for ld in (383, 376, 388):
    assert 'row stride' in refused(*swapped(ok, 14, ld))[1], ld
  for i in (0, 1, 2, 4, 5, 6, 7, 13, 24):
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i
  for i in (12, 18, 19):
    assert refused(*swapped(ok, i, 0))[0] == -1, i
  for n_new in (p(), None):
    for splits in (0, 1, 7, 64):
      need = lib.plm_extend_layer_workspace_bytes(5, 3, 3, 64, 512, 40, splits)
      assert need > 0
      rc, msg = refused(*swapped(ok, 9, n_new, 23, splits, 25, need - 1))  # one byte short
      assert rc == -4 and 'workspace' in msg, (splits, rc, msg)  # PLM_E_WORKSPACE


def test_d_not_a_multiple_of_32_is_refused_by_the_stages_chunk_rows_reuse():
  """head dims are multiples of 32, so d % 32 != 0 cannot be reached through (nh, hd); the two row-agnostic stages the extend layer
  reuses take d or K as a number and refuse it, at chunk-row counts too."""
  lib = _lib_loaded()
  assert 'd = ' in _refuser(lib, 'plm_decode_norm_fc1_act_bf16')(p(), p(), 1e-6, p(), p(), 32, 48, 512, 0, None)[1]
  assert 'unsupported shape' in _refuser(lib, 'plm_decode_gemm_residual_bf16')(p(), p(), p(), 32, 48, 48, None)[1]
  # the existing entry points keep their refusal of M = 33
  assert 'rows' in _refuser(lib, 'plm_decode_gemm_residual_bf16')(p(), p(), p(), 33, 768, 768, None)[1]
  assert 'rows' in _refuser(lib, 'plm_decode_norm_qkv_append_bf16')(p(), p(), 1e-6, p(), p(), p(), p(), 40, p(), p(), 384, p(), 33, 40, 3, 64,
                                                                     None)[1]


def test_layer_workspace_is_zero_on_refused_shapes_and_monotone_in_rows_and_Tmax():
  lib = _lib_loaded()
  ws = lib.plm_extend_layer_workspace_bytes
  r16 = lambda v: (v + 15) // 16 * 16  # noqa: E731
  for hd in (32, 64, 128):
    for splits in (0, 1, 7, 64):
      for n in (1, 2, 4, 8):
        prev = 0
        for B in (1, 2, 3, 4):  # B * n grows: so does the workspace
          got = ws(B, n, 12, hd, 2048, 1024, splits)
          M = B * n
          want = 2 * r16(M * 12 * hd * 2) + r16(M * 2048 * 2) + lib.plm_attn_extend_workspace_bytes(B, n, 12, hd, 1024, splits)
          assert got == want and got % 16 == 0 and got > prev, (hd, splits, B, n, got, want, prev)
          assert got == ws(B, n, 12, hd, 2048, 1024, splits)  # a function of its arguments alone
          prev = got
      prev = 0
      for n in (1, 2, 5, 8, 16, 17, 32):
        got = ws(1, n, 12, hd, 2048, 1024, splits)
        assert got > prev, (hd, splits, n, got, prev)
        prev = got
      prev = 0
      for Tmax in (1, 4, 37, 64, 65, 200, 1024, 8192, 1 << 20):
        got = ws(4, 8, 12, hd, 2048, Tmax, splits)
        assert got > 0 and got >= prev, (hd, splits, Tmax, got, prev)
        prev = got
  for bad in ((0, 4, 12, 64, 2048, 1024, 0), (33, 1, 12, 64, 2048, 1024, 0), (1, 33, 12, 64, 2048, 1024, 0), (4, 9, 12, 64, 2048, 1024, 0),
              (8, 0, 12, 64, 2048, 1024, 0), (8, -1, 12, 64, 2048, 1024, 0), (8, 4, 12, 48, 2048, 1024, 0), (8, 4, 12, 64, 2040, 1024, 0),
              (8, 4, 12, 64, 2048, 0, 0), (8, 4, 12, 64, 2048, 1024, 65), (8, 4, 12, 64, 2048, 1024, -1), (8, 4, 0, 64, 2048, 1024, 0)):
    assert ws(*bad) == 0, bad
  # the decode layer's query is what it was: one row per sequence, plm_attn_decode's partials
  assert lib.plm_decode_layer_workspace_bytes(8, 12, 64, 2048, 1024, 0) == \
      2 * r16(8 * 768 * 2) + r16(8 * 2048 * 2) + lib.plm_attn_decode_workspace_bytes(8, 12, 64, 1024, 0)


def _model():
  return P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=1, n_heads=2, mlp='glu'))


def test_check_fused_rows_and_the_fused_keywords_need_no_gpu():
  for B, n in ((33, 1), (4, 9), (1, 33)):
    with pytest.raises(ValueError, match='leave fused off$'):
      G.check_fused_rows('extend', B, n, 768)
  with pytest.raises(ValueError, match='leave fused off$'):
    G.check_fused_rows('extend', 4, 8, 48)
  for B, n in ((4, 8), (8, 4), (1, 32), (32, 1), (1, 1)):
    G.check_fused_rows('extend', B, n, 768)
  m = _model()
  assert 'fused' in inspect.signature(m.extend).parameters and inspect.signature(m.extend).parameters['fused'].default is False
  assert list(inspect.signature(m.extend).parameters)[:5] == ['tokens', 'cache', 'token_lens', 'logits', 'all_rows']
  assert list(inspect.signature(m.generate_lookup_fused).parameters) == list(inspect.signature(m.generate_lookup).parameters)
  assert str(inspect.signature(m.generate_lookup_fused)) == str(inspect.signature(m.generate_lookup))  # the defaults too
  assert inspect.unwrap(G.Generation.generate_lookup_fused).__module__ == G.__name__
  # guard's refusals come first, in their pinned order: CPU tokens are refused before the row count is looked at
  with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
    m.generate_lookup_fused(torch.zeros(4, 8, dtype=torch.int64), 4, n_draft=8)
  cache = LH.FakeCache([[1, 2]] * 4)
  cache.kv, cache.n_heads, cache.head_dim = [None], 2, 64
  with pytest.raises(RuntimeError, match='no CPU fallback'):
    m.extend(torch.zeros(4, 9, dtype=torch.int64), cache, fused=True)
  with pytest.raises(TypeError, match='int64'):
    m.extend(torch.zeros(4, 9, dtype=torch.int32), cache, fused=True)


class FusedFakeModel(LH.FakeModel):
  """LH.FakeModel whose extend takes - and records - the ``fused`` keyword; a call without it records None."""

  def __init__(self, lm):
    super().__init__(lm)
    self.seen = []

  def extend(self, chunk, cache, token_lens=None, logits=False, all_rows=False, **kw):
    self.seen.append(dict(kw))
    return super().extend(chunk, cache, token_lens=token_lens, logits=logits, all_rows=all_rows)


@pytest.mark.parametrize('fused', [False, True])
def test_lookup_session_passes_fused_to_extend_and_nothing_else_changes(fused):
  N, k, ngram = 30, 4, (1, 4)
  lm = LH.lm_drift
  want_t, want_l = LH._reference(lm, LH.PROMPTS, N)
  plain = LH.Run(lm, LH.PROMPTS, N, k, ngram)  # the session as the existing tests run it: no keyword at all
  cache = LH.FakeCache(LH.PROMPTS)
  first = LH._first(lm, LH.PROMPTS)
  model = FusedFakeModel(lm)
  s = G._LookupSession(model, cache, LH._padded(LH.PROMPTS), first[0], k, ngram, N, None, None, lookup=LH.fake_lookup, fused=fused)
  toks, lps, stats = G.speculative_loop(first, s.draft_round, s.target_round, s.accept, N, k, None, s.advance, drafted_in_round=s.drafted)
  s.check()
  assert model.seen and all(kw == ({'fused': True} if fused else {}) for kw in model.seen), model.seen
  assert torch.equal(toks, want_t) and torch.equal(lps, want_l)
  assert torch.equal(toks, plain.toks) and torch.equal(lps, plain.lps) and stats['rounds'] == plain.stats['rounds']
  assert torch.equal(stats['drafted'], plain.stats['drafted']) and torch.equal(stats['accepted'], plain.stats['accepted'])
  assert int(stats['drafted'].sum()) > 0
  assert list(inspect.signature(G._LookupSession.__init__).parameters)[-1] == 'fused'
  assert inspect.signature(G._LookupSession.__init__).parameters['fused'].default is False
