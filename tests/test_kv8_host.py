"""The FP8 KV cache without a GPU: the CPU reference (tests/kv8_ref.py, which the GPU tests trust) against a
literal per-block loop and on constructed blocks, ``forward_qdq`` against the oracle's forward, the two model-level distances the GPU
tolerance is checked against, every argument refusal of the new entry points before any HIP call, and the Python surface (KVCache,
ModelConfig.kv_cache, the pinned generate* parameter lists)."""
import ctypes as C
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_ref as R  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

import plainlm_amd as P  # noqa: E402
from plainlm_amd import _lib, ops  # noqa: E402
from plainlm_amd import generate as G  # noqa: E402

BF = torch.bfloat16
F8 = torch.float8_e4m3fn


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def literal(x, block=16):
  """The format's words, one block at a time, in Python floats: the smallest e with amax <= 448 * 2^e by search."""
  x = x.double()
  R_, K = x.shape
  q = torch.zeros((R_, K), dtype=torch.uint8)
  s = torch.zeros((R_, K // block), dtype=torch.uint8)
  for r in range(R_):
    for j in range(K // block):
      blk = x[r, j * block:(j + 1) * block]
      if not bool(torch.isfinite(blk).all()):
        q[r, j * block:(j + 1) * block], s[r, j] = 0x7F, 0xFF
        continue
      amax = float(blk.abs().max())
      if amax == 0.0:
        continue
      e = -127
      while e < 127 and amax > math.ldexp(448.0, e):
        e += 1
      s[r, j] = e + 127
      y = torch.tensor([math.ldexp(float(v), -e) for v in blk], dtype=torch.float32)
      q[r, j * block:(j + 1) * block] = y.to(F8).view(torch.uint8)
  return q, s


def test_reference_equals_the_literal_loop():
  g = torch.Generator().manual_seed(5)
  x = (torch.randn(7, 96, generator=g) * torch.exp2(torch.randint(-30, 30, (7, 96), generator=g).float())).to(BF)
  x[1, 16:32] = 0
  x[2, 40] = float('nan')
  x[3, 70] = float('-inf')
  q, s = R.quantize(x)
  ql, sl = literal(x)
  assert torch.equal(q, ql) and torch.equal(s, sl)
  assert R.row_bytes(768) == 1632 and R.row_bytes(96) == 208 and R.row_bytes(64) == 144 and R.row_bytes(128) == 272


def test_all_codes_round_trip_under_a_spread_of_scales():
  codes = torch.arange(256, dtype=torch.uint8).view(16, 16)
  for sb in (1, 2, 60, 119, 127, 128, 135, 200, 246):  # 246: 448 * 2^119, the largest block a bf16 maximum can ask for
    scales = torch.full((16, 1), sb, dtype=torch.uint8)
    v = R.dequantize(codes, scales)
    finite = torch.isfinite(v)
    assert int((~finite).sum()) == 2  # 0x7F and 0xFF
    # a dequantised block re-quantises to itself whenever its maximum needs this very scale: the top binade of the codes present
    for r in range(16):
      row = v[r:r + 1]
      if not bool(torch.isfinite(row).all()):
        continue
      q, s = R.quantize(row)
      back = R.dequantize(q, s)
      assert torch.equal(back, row), (sb, r)  # the VALUES always survive a second trip
      if float(row.abs().max()) > 224 * 2.0 ** (sb - 127):
        assert int(s[0, 0]) == sb and torch.equal(q[0] & 0x7F, codes[r] & 0x7F), (sb, r)
    assert torch.equal(v[finite].to(BF).double(), v[finite]) or sb < 10  # exact in bf16 above its subnormal range
  assert bool(torch.isnan(R.dequantize(codes, torch.full((16, 1), 255, dtype=torch.uint8))).all())


def _blk(first, rest=0.0):
  x = torch.full((1, 16), rest, dtype=torch.float64)
  x[0, 0] = first
  return x


def edge_rows():
  """The constructed blocks of the format's edges, bf16 [rows, 16]: shared with the GPU test, which runs them through the device."""
  rows = []
  for e in (-20, -1, 0, 3, 50):
    rows += [_blk(448.0 * 2.0 ** e), _blk(448.0 * 2.0 ** e * (1 + 2 ** -7))]       # amax exactly 448 * 2^e, and one bf16 ulp above
  rows += [_blk(256.0, 17.0), _blk(256.0, 19.0), _blk(256.0, 18.0), _blk(-256.0, -21.0)]  # RNE ties at step 2: 17 -> 16, 19 -> 20
  rows += [_blk(256.0, 2.0 ** -9 * k) for k in (1, 3, 5, 7)]                            # code subnormals 0x01 ..; k/2 ties below
  rows += [_blk(256.0, 2.0 ** -10), _blk(256.0, 3 * 2.0 ** -10), _blk(256.0, -2.0 ** -11)]
  rows += [_blk(0.0), _blk(-0.0, -0.0), _blk(float('nan'), 1.0), _blk(1.0, float('inf')), _blk(float('-inf'))]
  rows += [_blk(3e38, 1.0), _blk(1e-38, 1e-39), _blk(2.0 ** -133), _blk(1.0, -0.0)]   # the largest exponent bf16 reaches, the clamp of e at -127
  return torch.cat(rows).to(BF)


def test_constructed_edges():
  e = lambda x: int(R.quantize(x.to(BF))[1][0, 0]) - 127  # noqa: E731
  c = lambda x, i=0: int(R.quantize(x.to(BF))[0][0, i])  # noqa: E731
  for k in (-20, -1, 0, 3, 50):
    assert e(_blk(448.0 * 2.0 ** k)) == k and c(_blk(448.0 * 2.0 ** k)) == 0x7E
    assert e(_blk(448.0 * 2.0 ** k * (1 + 2 ** -7))) == k + 1
  # ties to even at a step of 2 (values 16..32 have step 2 in e4m3): 17 -> 16 (0x58), 19 -> 20 (0x5A), 18 exact (0x59)
  assert [c(_blk(256.0, v), 1) for v in (17.0, 19.0, 18.0)] == [0x58, 0x5A, 0x59] and c(_blk(-256.0, -21.0), 1) == 0xDA
  # subnormals: k * 2^-9 is code k; half steps tie to even: 2^-10 -> 0, 3 * 2^-10 -> 2; the sign of a value that rounds to zero stays
  assert [c(_blk(256.0, 2.0 ** -9 * k), 1) for k in (1, 3, 5, 7)] == [1, 3, 5, 7]
  assert c(_blk(256.0, 2.0 ** -10), 1) == 0 and c(_blk(256.0, 3 * 2.0 ** -10), 1) == 2 and c(_blk(256.0, -2.0 ** -11), 1) == 0x80
  q, s = R.quantize(_blk(-0.0, -0.0))
  assert int(s) == 0 and not bool(q.any())  # an all-zero block: zero codes, not sign bits
  for bad in (_blk(float('nan'), 1.0), _blk(1.0, float('inf')), _blk(float('-inf'))):
    q, s = R.quantize(bad)
    assert int(s) == 0xFF and bool((q == 0x7F).all()) and bool(torch.isnan(R.dequantize(q, s)).all())
  assert e(_blk(3e38)) == 120 and e(_blk(1e-38)) == -127 and e(_blk(2.0 ** -133)) == -127  # 448 * 2^119 < 3e38: bf16 never reaches the
  # clamp at 127; small values do reach the one at -127 (1e-38 / 2^-127 = 1.7, coded as a normal; 2^-133 as the subnormal 2^-6)
  x = edge_rows()
  assert torch.equal(R.quantize(x)[0], literal(x)[0]) and torch.equal(R.quantize(x)[1], literal(x)[1])


# ---- the model-level reference --------------------------------------------------------------------------------------------------------
def _golden():
  z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'model.npz'))
  w = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')}
  return w, torch.from_numpy(z['tokens'])[:, :64], O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=2)


def relmax(a, ref):
  return ((a.double() - ref.double()).abs().max() / ref.double().abs().max()).item()


def test_forward_qdq_switched_off_is_the_oracle_forward_and_the_two_distances():
  w, ids, cfg = _golden()
  plain = O.forward(w, cfg, ids)
  assert relmax(R.forward_qdq(w, cfg, ids, qdq_fn=None), plain) <= 1e-6
  q32 = R.forward_qdq(w, cfg, ids)
  q16 = R.forward_qdq(w, cfg, ids, round_kv=BF)
  d_plain, d_floor = relmax(q32, plain), relmax(q16, q32)
  print(f'golden model, logits relmax: qdq vs plain {d_plain:.3e}; qdq of bf16-rounded k/v vs qdq of fp32 k/v (the flip floor) {d_floor:.3e}')
  # what an e4m3 cache costs this model, and the floor rounding flips put under any comparison against forward_qdq: a bf16 rounding
  # that moves a value across an e4m3 rounding boundary changes that element by a whole e4m3 step (2^-4 relative), not by 2^-9.
  # e4m3 keeps 3 mantissa bits: an element error of at most 2^-4 relative; both distances stay far under 1 and are not zero
  assert 0 < d_floor < d_plain < 0.25


# ---- the C ABI: every refusal before any HIP call -----------------------------------------------------------------------------------------
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
NEW = ('plm_kv8_quant_rows', 'plm_kv8_dequant_rows', 'plm_kv8_append_rope_rows', 'plm_attn_decode_kv8', 'plm_attn_extend_kv8',
       'plm_extend_norm_qkv_append_kv8_bf16', 'plm_decode_layer_kv8_bf16', 'plm_extend_layer_kv8_bf16')
LD8 = 208  # nh = 3, hd = 32: 2 * 96 + 12 = 204 -> 208
BAD_LD8 = (203, 192, 200, 212, 216)  # short; no multiple of 16


def swapped(ok, i, v):
  a = list(ok)
  a[i] = v
  return a


def test_the_new_entry_points_are_declared_bound_and_exported():
  lib = _lib_loaded()
  for name in NEW:
    assert name in _lib.header_functions() and name in _lib.SIGNATURES and hasattr(lib, name), name
  assert _lib.EXPECTED_ABI == 112 == lib.plm_version()  # additive: the number did not move
  for name in NEW:
    assert hasattr(ops, {'plm_kv8_quant_rows': 'kv8_quant_rows', 'plm_kv8_dequant_rows': 'kv8_dequant_rows',
                         'plm_kv8_append_rope_rows': 'kv8_append_rope_rows', 'plm_attn_decode_kv8': 'attn_decode_kv8',
                         'plm_attn_extend_kv8': 'attn_extend_kv8', 'plm_extend_norm_qkv_append_kv8_bf16': 'extend_norm_qkv_append_kv8',
                         'plm_decode_layer_kv8_bf16': 'decode_layer_kv8', 'plm_extend_layer_kv8_bf16': 'extend_layer_kv8'}[name])
  assert ops.kv8_row_bytes(768) == 1632 and ops.kv8_row_bytes(96) == LD8 and ops.KV8_BLOCK == 16


@pytest.mark.parametrize('name', ['plm_kv8_quant_rows', 'plm_kv8_dequant_rows'])
def test_quant_and_dequant_rows_refuse_bad_arguments_without_a_gpu(name):
  refused = _refuser(_lib_loaded(), name)
  # quant: src, ld_src, kv8, ld_kv8, B, T, Tmax, nh, hd, stream; dequant: kv8, ld_kv8, dst, ld_dst, ...
  quant = name.endswith('quant_rows') and 'dequant' not in name
  ok = [p(), 192, p(), LD8, 5, 16, 37, 3, 32, None] if quant else [p(), LD8, p(), 192, 5, 16, 37, 3, 32, None]
  i_ld, i_ld8 = (1, 3) if quant else (3, 1)
  for i in (0, 2):
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i
  for hd in (0, 16, 48, 256):
    assert 'head_dim' in refused(*swapped(ok, 8, hd))[1], hd
  for i, v in ((4, 0), (5, 0), (5, 38), (6, 0), (7, 0), (4, 1 << 20)):
    assert 'bad shape' in refused(*swapped(ok, i, v))[1], (i, v)
  for ld in (191, 184, 196):
    assert 'bf16 row stride' in refused(*swapped(ok, i_ld, ld))[1], ld
  for ld in BAD_LD8:
    rc, msg = refused(*swapped(ok, i_ld8, ld))
    assert rc == -1 and 'FP8 cache' in msg and 'row stride' in msg, ld


def test_kv8_append_rope_rows_refuses_bad_arguments_without_a_gpu():
  refused = _refuser(_lib_loaded(), 'plm_kv8_append_rope_rows')
  # qkv, ld_qkv, lens0, n_new, rope_cos, rope_sin, rope_T, q_out, kv8, ld_kv8, status, B, n, Tmax, nh, hd, stream
  ok = [p(), 288, p(), p(), p(), p(), 40, p(), p(), LD8, p(), 5, 4, 37, 3, 32, None]
  for i in (0, 2, 4, 5, 7, 8, 10):
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
  for hd in (0, 16, 48, 256):
    assert 'head_dim' in refused(*swapped(ok, 15, hd))[1], hd
  for i in (6, 11, 12, 13, 14):
    assert 'bad shape' in refused(*swapped(ok, i, 0))[1], i
  for ld in (287, 280, 292):
    assert 'row stride' in refused(*swapped(ok, 1, ld))[1], ld
  for ld in BAD_LD8:
    rc, msg = refused(*swapped(ok, 9, ld))
    assert rc == -1 and 'FP8 cache' in msg, ld
  for i in (0, 4, 5, 7, 8):
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i


@pytest.mark.parametrize('name', ['plm_attn_decode_kv8', 'plm_attn_extend_kv8'])
def test_attention_over_kv8_refuses_bad_arguments_without_a_gpu(name):
  lib = _lib_loaded()
  refused = _refuser(lib, name)
  big = 1 << 40
  if name == 'plm_attn_decode_kv8':  # q, kv8, ld_kv8, lens, out, lse, B, Tmax, nh, hd, splits, workspace, bytes, stream
    ok = [p(), p(), LD8, p(), p(), p(), 5, 37, 3, 32, 0, p(), big, None]
    ptrs, i_hd, i_sp, i_ws, shape, need = (0, 1, 3, 4, 11), 9, 10, 12, (6, 7, 8), lambda s: lib.plm_attn_decode_workspace_bytes(5, 3, 32, 37, s)
  else:  # q, kv8, ld_kv8, lens0, n_new, out, lse, B, n, Tmax, nh, hd, splits, workspace, bytes, stream
    ok = [p(), p(), LD8, p(), p(), p(), p(), 5, 4, 37, 3, 32, 0, p(), big, None]
    ptrs, i_hd, i_sp, i_ws, shape, need = (0, 1, 3, 5, 13), 11, 12, 14, (7, 8, 9, 10), lambda s: lib.plm_attn_extend_workspace_bytes(5, 4, 3, 32, 37, s)
  for i in ptrs:
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
  for i in (0, 1, ptrs[3], ptrs[4]):
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i
  for hd in (16, 48, 96):
    assert 'head_dim' in refused(*swapped(ok, i_hd, hd))[1], hd
  for i in shape:
    assert 'bad shape' in refused(*swapped(ok, i, 0))[1], i
  for s in (-1, 65):
    assert 'splits' in refused(*swapped(ok, i_sp, s))[1], s
  for ld in BAD_LD8:
    rc, msg = refused(*swapped(ok, 2, ld))
    assert rc == -1 and 'FP8 cache' in msg, ld
  for s in (0, 1, 7, 64):
    rc, msg = refused(*swapped(swapped(ok, i_sp, s), i_ws, need(s) - 1))
    assert rc == -4 and 'workspace' in msg, (s, rc, msg)  # PLM_E_WORKSPACE


def test_fused_stage_over_kv8_refuses_bad_arguments_without_a_gpu():
  refused = _refuser(_lib_loaded(), 'plm_extend_norm_qkv_append_kv8_bf16')
  # x, norm_w, eps, w_qkv, lens0, n_new, rope_cos, rope_sin, rope_T, q_out, kv8, ld_kv8, status, B, n, Tmax, nh, hd, stream
  ok = [p(), p(), 1e-6, p(), p(), p(), p(), p(), 40, p(), p(), LD8, p(), 5, 4, 37, 3, 32, None]
  for i in (0, 1, 3, 4, 6, 7, 9, 10, 12):
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
  for B, n in ((0, 4), (33, 1), (5, 7), (1, 33), (5, 0)):
    assert 'rows' in refused(*swapped(swapped(ok, 13, B), 14, n))[1], (B, n)
  for hd in (0, 16, 48, 256):
    assert 'head_dim' in refused(*swapped(ok, 17, hd))[1], hd
  for i in (8, 15, 16):
    assert 'bad shape' in refused(*swapped(ok, i, 0))[1], i
  for ld in BAD_LD8:
    rc, msg = refused(*swapped(ok, 11, ld))
    assert rc == -1 and 'FP8 cache' in msg and 'row stride' in msg, ld
  for i in (0, 1, 3, 9, 10):
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i


@pytest.mark.parametrize('name', ['plm_decode_layer_kv8_bf16', 'plm_extend_layer_kv8_bf16'])
def test_layers_over_kv8_refuse_bad_arguments_without_a_gpu(name):
  lib = _lib_loaded()
  refused = _refuser(lib, name)
  big = 1 << 40
  # 0 x, 1 attn_norm_w, 2 mlp_norm_w, 3 eps, 4 w_qkv, 5 w_out, 6 w_fc1, 7 w_fc2, 8 pos | lens0, 9 lens | n_new, 10 rope_cos, 11 rope_sin,
  # 12 rope_T, 13 kv8, 14 ld_kv8, 15 status, 16 B, [17 n,] Tmax, nh, hd, hidden, mlp_kind, splits, workspace, bytes, stream
  head = [p(), p(), p(), 1e-6, p(), p(), p(), p(), p(), p(), p(), p(), 40, p(), LD8, p(), 5]
  dec = name.startswith('plm_decode')
  ok = head + ([] if dec else [4]) + [37, 3, 32, 512, 0, 0, p(), big, None]
  o = 0 if dec else 1  # the extend layer's extra n shifts what follows B
  nulls = (0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 13, 15, 24 + o - 1) + ((9,) if dec else ())  # n_new may be NULL
  for i in nulls:
    assert 'null pointer' in refused(*swapped(ok, i, None))[1], i
  for B in (0, 33):
    assert 'rows' in refused(*swapped(ok, 16, B))[1], B
  for hd in (16, 48, 96):
    assert 'head_dim' in refused(*swapped(ok, 19 + o, hd))[1], hd
  for h in (0, 8, 520):
    assert 'hidden' in refused(*swapped(ok, 20 + o, h))[1], h
  for kind in (-1, 3):
    assert 'mlp_kind' in refused(*swapped(ok, 21 + o, kind))[1], kind
  for s in (-1, 65):
    assert 'splits' in refused(*swapped(ok, 22 + o, s))[1], s
  for ld in BAD_LD8:
    rc, msg = refused(*swapped(ok, 14, ld))
    assert rc == -1 and 'FP8 cache' in msg, ld
  for i in (0, 1, 2, 4, 5, 6, 7, 13, 23 + o):
    assert 'aligned' in refused(*swapped(ok, i, odd()))[1], i
  for i in (12, 17 + o, 18 + o):
    assert refused(*swapped(ok, i, 0))[0] == -1, i
  for splits in (0, 1, 7, 64):
    need = lib.plm_decode_layer_workspace_bytes(5, 3, 32, 512, 37, splits) if dec else lib.plm_extend_layer_workspace_bytes(5, 4, 3, 32, 512, 37, splits)
    assert need > 0
    rc, msg = refused(*swapped(swapped(ok, 22 + o, splits), 24 + o, need - 1))
    assert rc == -4 and 'workspace' in msg, (splits, rc, msg)


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------
def _cfg(**kw):
  return P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu', **kw)


def test_kv_cache_config_and_kvcache_shapes():
  assert _cfg().kv_cache == 'bf16' and G.KV_DTYPES == ('bf16', 'fp8')
  with pytest.raises(ValueError, match='kv_cache'):
    P.Transformer(_cfg(kv_cache='fp4'))
  with pytest.raises(ValueError, match='kv_cache'):
    G.KVCache(2, 3, 8, 2, 64, 'cpu', kv_dtype='int8')
  m = P.Transformer(_cfg(kv_cache='fp8'))
  assert m.cfg.kv_cache == 'fp8'
  c = G.KVCache(2, 3, 8, 2, 64, 'cpu')
  assert c.kv_dtype == 'bf16' and c.row_bytes == 512 and c.kv[0].dtype == BF and tuple(c.kv[0].shape) == (3, 8, 256) and c.to_bf16(1) is c.kv[1]
  c8 = G.KVCache(2, 3, 8, 2, 64, 'cpu', kv_dtype='fp8')
  assert c8.kv_dtype == 'fp8' and c8.row_bytes == 272 == R.row_bytes(128) and c8.kv[1].dtype == torch.uint8 and tuple(c8.kv[1].shape) == (3, 8, 272)
  assert abs(R.row_bytes(768) / 3072 - 0.53) < 0.005
  c8.set_lens(torch.tensor([3, 0, 8], dtype=torch.int32))
  c8.advance()
  assert c8.lens.tolist() == [4, 1, 9] and c8.pos.tolist() == [3, 0, 8]
  c8.check()
  # a cache of another shape is refused before any library call, whatever its format
  G.check_cache('extend', c8, m)
  with pytest.raises(ValueError, match='another model shape'):
    G.check_cache('extend', G.KVCache(1, 3, 8, 2, 64, 'cpu', kv_dtype='fp8'), m)
  with pytest.raises(ValueError, match='another model shape'):
    G.check_cache('decode_step', G.KVCache(2, 3, 8, 4, 32, 'cpu'), m)
  from types import SimpleNamespace
  from plainlm_amd.construct import construct_model
  y = dict(model='transformer', vocab_size=256, d_model=128, expand='8/3', n_layers=1, n_heads=2, mlp_class='glu', seq_len=64, tie_embeddings=False)
  assert construct_model(SimpleNamespace(**y))[1].kv_cache == 'bf16'
  assert construct_model(SimpleNamespace(kv_cache='fp8', **y))[1].kv_cache == 'fp8'
  with pytest.raises(ValueError, match='kv_cache'):
    construct_model(SimpleNamespace(kv_cache='e5m2', **y))


PINNED = {
  'generate': ['prompt', 'max_new_tokens', 'prompt_lens', 'eos_id', 'sample', 'return_logprobs', 'temperature', 'top_k', 'top_p', 'seed'],
  'generate_speculative': ['prompt', 'max_new_tokens', 'draft', 'n_draft', 'prompt_lens', 'eos_id', 'return_logprobs', 'temperature', 'top_k',
                           'top_p', 'seed', 'return_stats'],
  'generate_lookup': ['prompt', 'max_new_tokens', 'n_draft', 'ngram', 'prompt_lens', 'eos_id', 'return_logprobs', 'temperature', 'top_k', 'top_p',
                      'seed', 'return_stats'],
}
PINNED['generate_fused'] = PINNED['generate']
PINNED['generate_lookup_fused'] = PINNED['generate_lookup']


def test_pinned_signatures_are_unchanged_and_the_new_parameter_is_last():
  for name, want in PINNED.items():
    assert list(inspect.signature(getattr(G.Generation, name)).parameters)[1:] == want, name
  assert list(inspect.signature(G.Generation.prefill).parameters)[1:] == ['x', 'prompt_lens', 'max_len', 'logits', 'kv_dtype']
  assert list(inspect.signature(G.Generation.new_cache).parameters)[1:] == ['B', 'max_len', 'kv_dtype']
  assert inspect.signature(G.Generation.prefill).parameters['kv_dtype'].default is None
  assert list(inspect.signature(G.KVCache.__init__).parameters)[1:] == ['n_layers', 'B', 'Tmax', 'n_heads', 'head_dim', 'device', 'kv_dtype']
  # the wrappers are defined in ops_kv8.py, not in ops.py
  assert ops.attn_decode_kv8.__module__ == 'plainlm_amd.ops_kv8' and ops.kv8_quant_rows.__module__ == 'plainlm_amd.ops_kv8'
