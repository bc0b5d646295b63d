"""CPU tests (no GPU) of KV-cached generation: its three entry points refuse bad arguments before any HIP call (the header, the
binding table and the library are compared in tests/test_host_logic.py); the workspace query is positive and monotone;
tests/decode_ref.py's split-and-combine restatement equals the unsplit softmax, empty splits included; and the host logic of generate
(plainlm_amd/generate.py) on a fake step function."""

import ctypes as C
import math
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib
from plainlm_amd import generate as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import decode_ref as R  # noqa: E402


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


def test_attn_decode_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  refused = _refuser(lib, 'plm_attn_decode')
  big = 1 << 40
  # q, kv, ld_kv, lens, out, lse, B, Tmax, nh, hd, splits, workspace, bytes, stream
  ok = [p(), p(), 384, p(), p(), None, 5, 40, 3, 64, 2, p(), big, None]
  for i in (0, 1, 3, 4, 11):  # every pointer but lse
    a = list(ok)
    a[i] = None
    assert 'null pointer' in refused(*a)[1], i
  for hd in (0, 16, 48, 96, 256):
    a = list(ok)
    a[9] = hd
    assert 'head_dim' in refused(*a)[1], hd
  for i in (0, 1, 4, 11):
    a = list(ok)
    a[i] = odd()
    assert 'aligned' in refused(*a)[1], i
  for s in (-1, 65, 1000):
    a = list(ok)
    a[10] = s
    assert 'splits' in refused(*a)[1], s
  for ld in (383, 380, 388):  # shorter than a row, and not a multiple of 8
    a = list(ok)
    a[2] = ld
    assert 'row stride' in refused(*a)[1], ld
  for splits in (0, 1, 7, 64):
    need = lib.plm_attn_decode_workspace_bytes(5, 3, 64, 40, splits)
    a = list(ok)
    a[10], a[12] = splits, need - 1
    rc, msg = refused(*a)
    assert rc == -4 and 'workspace' in msg, (splits, rc, msg)  # PLM_E_WORKSPACE


def test_kv_append_rope_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  refused = _refuser(lib, 'plm_kv_append_rope')
  # qkv, ld_qkv, pos, rope_cos, rope_sin, rope_T, q_out, kv, ld_kv, status, B, Tmax, nh, hd, stream
  ok = [p(), 576, p(), p(), p(), 40, p(), p(), 384, p(), 5, 40, 3, 64, None]
  for i in (0, 2, 3, 4, 6, 7, 9):
    a = list(ok)
    a[i] = None
    assert 'null pointer' in refused(*a)[1], i
  for hd in (0, 16, 96):
    a = list(ok)
    a[13] = hd
    assert 'head_dim' in refused(*a)[1], hd
  for i in (0, 3, 4, 6, 7):
    a = list(ok)
    a[i] = odd()
    assert 'aligned' in refused(*a)[1], i
  for i, ld in ((1, 568), (1, 580), (8, 376), (8, 388)):
    a = list(ok)
    a[i] = ld
    assert 'row strides' in refused(*a)[1], (i, ld)
  for i in (5, 10, 11, 12):  # rope_T, B, Tmax, nh
    a = list(ok)
    a[i] = 0
    assert 'bad shape' in refused(*a)[1], i


def test_decode_workspace_is_positive_and_monotone():
  lib = _lib_loaded()
  ws = lib.plm_attn_decode_workspace_bytes
  for hd in (32, 64, 128):
    for splits in (0, 1, 7, 64):
      prev = 0
      for B in (1, 2, 5, 8, 64, 1000):
        n = ws(B, 12, hd, 1024, splits)
        assert n > 0 and n % 16 == 0 and n >= prev, (hd, splits, B, n, prev)
        prev = n
      prev = 0
      for Tmax in (1, 4, 37, 64, 65, 200, 1024, 8192, 1 << 20):
        n = ws(8, 12, hd, Tmax, splits)
        assert n > 0 and n >= prev, (hd, splits, Tmax, n, prev)
        prev = n
    prev = 0
    for splits in range(1, 65):
      n = ws(8, 12, hd, 1024, splits)
      assert n > prev, (hd, splits, n, prev)
      assert n >= 8 * 12 * splits * (hd + 2) * 4  # one fp32 (m, l, acc[hd]) per (sequence, head, split)
      prev = n
    assert ws(8, 12, hd, 1024, 0) <= ws(8, 12, hd, 1024, 64)  # automatic never needs more than the largest forced count
  for bad in ((0, 12, 64, 1024, 0), (8, 0, 64, 1024, 0), (8, 12, 48, 1024, 0), (8, 12, 64, 0, 0), (8, 12, 64, 1024, -1), (8, 12, 64, 1024, 65)):
    assert ws(*bad) == 0, bad


def test_split_and_combine_restatement_equals_the_unsplit_softmax():
  """tests/decode_ref.py: the kernel's partition and combine rule in fp64 against the plain softmax, to 1e-12, for split counts with and
  without empty ranges - and the two non-finite hazards: an empty range must not turn the result into NaN, no key at all is (0, +inf)."""
  rng = np.random.default_rng(0)
  hd = 16
  for L in (1, 5, 13):
    q, k, v = rng.standard_normal(hd) * 3, rng.standard_normal((L, hd)), rng.standard_normal((L, hd))
    want_o, want_l = R.attn_row(q, k, v)
    for S in (1, 2, 7):
      ranges = R.split_ranges(L, S)
      assert len(ranges) == S and ranges[0][0] == 0 and max(b for _, b in ranges) == L
      assert all(a <= b for a, b in ranges) and all(ranges[i][1] == ranges[i + 1][0] or ranges[i + 1][0] == L for i in range(S - 1))
      if S > L:
        assert any(a == b for a, b in ranges)  # empty splits are part of the case
      o, l = R.split_and_combine(q, k, v, S)
      assert np.isfinite(o).all() and math.isfinite(l)
      assert np.abs(o - want_o).max() <= 1e-12 and abs(l - want_l) <= 1e-12, (L, S)
  o, l = R.split_and_combine(np.ones(hd), np.zeros((0, hd)), np.zeros((0, hd)), 7)
  assert (o == 0).all() and l == math.inf
  o, l = R.attn_row(np.ones(hd), np.zeros((0, hd)), np.zeros((0, hd)))
  assert (o == 0).all() and l == math.inf


# ---- generate's host logic on a fake step -------------------------------------------------------------------------------------------
def _fake_step(V=11):
  calls = []

  def step(tok):
    calls.append(tok.clone())
    return (tok * 3 + 1) % V, -(tok.float() + 1.0)
  return step, calls


def test_generate_loop_counts_steps_and_freezes_after_eos():
  step, calls = _fake_step()
  first = (torch.tensor([2, 5, 4]), torch.tensor([-0.5, -0.25, -1.0]))
  toks, lps = G.generate_loop(first, step, 9)
  assert toks.shape == (3, 9) and lps.shape == (3, 9) and len(calls) == 8
  want = [2]
  for _ in range(8):
    want.append((want[-1] * 3 + 1) % 11)
  assert toks[0].tolist() == want and lps[0, 0].item() == -0.5 and lps[0, 1].item() == -3.0
  # eos = 4: sequence 0 (2, 7, 0, 1, 4, ...) emits it at index 4, sequence 1 (5, 5, ...) never, sequence 2 starts with it
  step, calls = _fake_step()
  te, le = G.generate_loop(first, step, 9, eos_id=4)
  assert te[0].tolist() == want[:5] + [4] * 4
  assert torch.equal(le[0, :5], lps[0, :5]) and (le[0, 5:] == 0).all()
  assert torch.equal(te[1], toks[1]) and torch.equal(le[1], lps[1])
  assert te[2].tolist() == [4] * 9 and le[2, 0].item() == -1.0 and (le[2, 1:] == 0).all()
  assert len(calls) == 8  # finished sequences still ride along: the batch stays rectangular
  assert G.generate_loop(first, step, 1)[0].shape == (3, 1)


def test_generate_loop_checks_for_the_end_at_most_once_every_16_steps():
  step, calls = _fake_step()
  checks = []

  def all_done(done):
    checks.append(len(calls))
    return bool(done.all())
  first = (torch.tensor([2, 5]), torch.zeros(2))
  toks, _ = G.generate_loop(first, step, 50, eos_id=10**6, all_done=all_done)  # never finishes
  assert toks.shape == (2, 50) and len(calls) == 49
  assert len(checks) <= 49 // 16 and all(b - a >= 16 for a, b in zip(checks, checks[1:])), checks
  # without eos_id there is nothing to check
  step, calls = _fake_step()
  checks.clear()
  G.generate_loop(first, step, 50, all_done=all_done)
  assert checks == []
  # everything finished early: the loop stops at the next check and the tail is eos / 0
  step, calls = _fake_step()
  checks.clear()
  te, le = G.generate_loop((torch.tensor([4, 4]), torch.tensor([-1.0, -2.0])), step, 40, eos_id=4, all_done=all_done)
  assert te.shape == (2, 40) and (te == 4).all() and (le[:, 1:] == 0).all() and le[:, 0].tolist() == [-1.0, -2.0]
  assert len(checks) == 1 and len(calls) == 15
  assert G.FINISH_CHECK_EVERY == 16


def test_prompt_lens_and_the_row_a_padded_prompt_continues_from():
  assert G.prompt_lens_list(None, 3, 16) == [16, 16, 16]
  assert G.prompt_lens_list((16, 9), 2, 16) == [16, 9]
  assert G.prompt_lens_list(torch.tensor([1, 16]), 2, 16) == [1, 16]
  for bad in ((16,), (16, 9, 3), (0, 9), (17, 9)):
    with pytest.raises(ValueError, match='prompt_lens'):
      G.prompt_lens_list(bad, 2, 16)
  B, T, d = 3, 8, 4
  y = torch.arange(B * T * d, dtype=torch.float32).view(B * T, d)
  lens = torch.tensor([8, 3, 1], dtype=torch.int32)
  rows = G.last_rows(y, B, T, lens)
  assert torch.equal(rows, torch.stack([y[7], y[8 + 2], y[16 + 0]]))  # row lens[b] - 1 of every sequence, not the padded last row
  assert [G.pad4(n) for n in (1, 4, 5, 16, 17)] == [4, 4, 8, 16, 20]


def test_over_length_and_other_refusals_come_before_any_launch():
  assert G.check_lengths(16, 32, 64) == 48
  assert G.check_lengths(17, 2, 64) == 20  # the padded prompt has to fit the cache too
  assert G.check_lengths(32, 32, 64) == 64
  with pytest.raises(ValueError, match=r'prompt length 33 \+ max_new_tokens 32 exceeds cfg.seq_len 64'):
    G.check_lengths(33, 32, 64)
  with pytest.raises(ValueError, match='max_new_tokens'):
    G.check_lengths(16, 0, 64)
  EC = dict(model='transformer', vocab_size=512, seq_len=128, d_model=128, expand='8/3', n_layers=2, n_heads=2, mlp_class='glu',
            tie_embeddings=False)
  model, _ = P.construct_model(namedtuple('Config', EC.keys())(**EC))
  ids = torch.zeros(1, 16, dtype=torch.int64)
  with pytest.raises(RuntimeError, match='MI355X'):
    model.generate(ids, 8)
  with torch.no_grad(), pytest.raises(RuntimeError, match='MI355X'):
    model.prefill(ids)
  with torch.no_grad(), pytest.raises(RuntimeError, match='MI355X'):
    model.decode_step(ids[:, 0], None)
  mx = P.Transformer(P.ModelConfig(vocab_size=512, seq_len=128, dim=128, expand=8 / 3, n_layers=1, n_heads=2, linear_precision='mxfp8'))
  with pytest.raises(NotImplementedError, match='linear_precision'):
    mx.prefill(ids)
  with pytest.raises(NotImplementedError, match='linear_precision'):
    mx.decode_step(ids[:, 0], None)
  from plainlm_amd import ops
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.attn_decode(torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(2, 8, 128, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32), 1)
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.kv_append_rope(torch.zeros(2, 192, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.int32), torch.zeros(8, 32), torch.zeros(8, 32),
                       torch.zeros(2, 8, 128, dtype=torch.bfloat16), 1)
