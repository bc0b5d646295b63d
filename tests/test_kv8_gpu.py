"""The FP8 KV cache on a real MI355X.  Dequantisation is exact, so everything below the model level is bit
equality: the quantisers against tests/kv8_ref.py on the bf16 rows the bf16 path writes for the same inputs, the attention kernels
against their bf16 twins on the dequantised cache, the fused stage against the unfused one, the layers against their stages.  The model
level has the one tolerance (see test_teacher_forced_logits_vs_forward_qdq)."""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity as PB  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv8_ref as R  # noqa: E402

BF16, U8, I32 = torch.bfloat16, torch.uint8, torch.int32


@pytest.fixture(scope='module')
def P():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  import plainlm_amd
  return plainlm_amd


@pytest.fixture(scope='module')
def ops(P):
  from plainlm_amd import ops as _ops
  return _ops


def i32(v):
  return torch.tensor(list(v), dtype=I32).cuda()


def biteq(a, b):
  return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def same(a, b):
  """Equal values, NaN where and only where the other has NaN."""
  na, nb = torch.isnan(a), torch.isnan(b)
  return torch.equal(na, nb) and torch.equal(a[~na], b[~nb])


def rnd(seed, *shape):
  return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def sentinel8(seed, B, Tmax, dm, pad=16):
  """A cache full of random bytes with a padded row stride: (the [B, Tmax, row_bytes] view, its CPU clone)."""
  rb = R.row_bytes(dm)
  buf = torch.randint(0, 256, (B, Tmax, rb + pad), generator=torch.Generator().manual_seed(seed), dtype=U8).cuda()
  kv = buf[:, :, :rb]
  return kv, kv.cpu().clone()


def cache8_of(kvrows, Tmax, pad=16):
  """bf16 k | v rows [B, Tmax, 2*dm] -> the FP8 cache tests/kv8_ref.py makes of them, on the GPU, row stride padded."""
  B, _, two_dm = kvrows.shape
  rb = R.row_bytes(two_dm // 2)
  buf = torch.zeros(B, Tmax, rb + pad, dtype=U8)
  buf[:, :, :rb] = R.pack_rows(kvrows.reshape(B * Tmax, two_dm)).view(B, Tmax, rb)
  return buf.cuda()[:, :, :rb]


def assert_rows_are_quantize_of(kv8, want_bf16, rows, before, dm):
  """Cache rows ``rows`` (a bool [B, Tmax]) hold kv8_ref.quantize of want_bf16's rows; every other row is what ``before`` held."""
  got = kv8.cpu()
  B, Tmax = rows.shape
  codes, scales = R.unpack_rows(got.reshape(B * Tmax, -1), dm)
  q, s = R.quantize(want_bf16.cpu().reshape(B * Tmax, 2 * dm))
  m = rows.reshape(-1)
  assert torch.equal(codes[m], q[m]) and torch.equal(scales[m], s[m])
  assert torch.equal(got[~rows], before[~rows])  # untouched rows, pad bytes included
  assert torch.equal(got[rows][:, 2 * dm + dm // 8:], before[rows][:, 2 * dm + dm // 8:])  # the pad bytes of a written row


# ---- quantiser, appender, dequantiser ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nh,hd', [(3, 32), (2, 64), (1, 128)])
def test_appender_writes_quantize_of_the_bf16_appenders_rows(ops, nh, hd):
  B, Tmax, dm = 5, 37, nh * hd
  cos, sin = (t.cuda() for t in O.rope_table(hd, Tmax))
  # (n, lens0, n_new): a chunk of 3 with both ends of the cache, a refused sequence (36 + 3 > 37), a ragged and an empty one; then the
  # decode step, n = 1, at positions 0 and Tmax - 1 with one position outside
  for n, lens0, n_new in ((3, (0, 34, 17, 36, 5), (3, 3, 1, 3, 0)), (1, (0, 36, 17, 37, 35), None), (4, (33, 0, 9, -1, 20), None)):
    qkv = (rnd(11 + n, B * n, 3 * dm + 8) * 2).to(BF16).cuda()[:, :3 * dm]  # a padded row stride
    kvb = rnd(12, B, Tmax, 2 * dm).to(BF16).cuda()
    kv8, before = sentinel8(13, B, Tmax, dm)
    nn = None if n_new is None else i32(n_new)
    qb, sb = ops.kv_append_rope_rows(qkv, i32(lens0), cos, sin, kvb, nh, n_new=nn)
    q8, s8 = ops.kv8_append_rope_rows(qkv, i32(lens0), cos, sin, kv8, nh, n_new=nn)
    assert biteq(qb, q8) and sb.tolist() == s8.tolist() == [1]
    rows = torch.zeros(B, Tmax, dtype=torch.bool)
    for b, l0 in enumerate(lens0):
      c = n if n_new is None else n_new[b]
      if 0 <= l0 and l0 + c <= Tmax:
        rows[b, l0:l0 + c] = True
    assert int(rows.sum()) > 0
    assert_rows_are_quantize_of(kv8, kvb, rows, before, dm)


def test_quant_rows_edge_cases_and_dequant_rows(ops):
  import test_kv8_host as H
  nh, hd, Tmax = 1, 32, 37
  dm = nh * hd
  e = H.edge_rows()  # [T, 16]: each edge block fills the four blocks of a row, rotated so that every block position sees it
  T = e.shape[0]
  assert T <= Tmax
  rows = torch.stack([torch.roll(e, k, dims=1) for k in range(4)], dim=1).reshape(1, T, 64)
  rows = torch.cat([rows, (rnd(3, 1, T, 64) * torch.exp2(torch.randint(-20, 20, (1, T, 64), generator=torch.Generator().manual_seed(4)).float())).to(BF16)])
  wide = torch.zeros(2, T, 3 * dm, dtype=BF16)
  wide[:, :, dm:] = rows
  kv8, before = sentinel8(21, 2, Tmax, dm)
  ops.kv8_quant_rows(wide.cuda()[:, :, dm:], kv8, nh)  # a column slice, as prefill passes it
  full = torch.zeros(2, Tmax, 2 * dm, dtype=BF16)
  full[:, :T] = rows
  written = torch.zeros(2, Tmax, dtype=torch.bool)
  written[:, :T] = True
  assert_rows_are_quantize_of(kv8, full, written, before, dm)
  # the dequantiser: every row of the cache, stale random bytes included, against the reference
  deq = ops.kv8_dequant_rows(kv8, nh, hd).cpu().double().reshape(2 * Tmax, 2 * dm)
  want = R.dequantize(*R.unpack_rows(kv8.cpu().reshape(2 * Tmax, -1), dm))
  # the random stale bytes reach what the model never does: values below bf16's normal range (the image may round there) and above its
  # largest finite value (the image is inf); everything between is exact, and NaN is NaN
  nan = torch.isnan(want)
  assert torch.equal(torch.isnan(deq), nan)
  ok = ~nan & ((want == 0) | ((want.abs() >= 2.0 ** -126) & (want.abs() < 2.0 ** 127)))
  assert int(ok.sum()) > ok.numel() // 2 and torch.equal(deq[ok], want[ok])
  back = ops.kv8_dequant_rows(kv8, nh, hd, T=T).cpu().double()
  assert same(back, R.qdq(full[:, :T].reshape(-1, 2 * dm)).view(2, T, 2 * dm))


# ---- attention over the FP8 cache = attention over its bf16 image ----------------------------------------------------------------------------
def attn_case(cls, B, Tmax, nh, hd, seed):
  """(q rows bf16 [B*Tmax, dm], FP8 cache, its dequantised bf16 image) of one of oracle/parity.py's input classes."""
  qkv, _ = PB.attn_inputs(cls, B, Tmax, nh, hd, seed)
  dm = nh * hd
  x = qkv.view(B, Tmax, 3 * dm)
  return x[:, :, :dm].reshape(B * Tmax, dm).contiguous().cuda(), cache8_of(x[:, :, dm:].contiguous(), Tmax)


def poison(kv8, lens):
  """0xFF (NaN codes under a NaN scale) in every row at and beyond lens[b]: such a row must never be read."""
  for b, n in enumerate(lens):
    kv8[b, n:] = 0xFF


@pytest.mark.parametrize('cls', ['randn', 'peaked', 'spike'])
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_decode_kv8_is_attn_decode_on_the_dequantised_cache(ops, hd, cls):
  B, Tmax, nh = 5, 37, 96 // hd if hd < 128 else 1
  lens = (0, 1, 13, 36, Tmax)
  qrows, kv8 = attn_case(cls, B, Tmax, nh, hd, 7)
  poison(kv8, lens)
  deq = ops.kv8_dequant_rows(kv8, nh, hd)
  q = qrows.view(B, Tmax, -1)[:, -1].contiguous()
  for splits in (1, 7, 64, 0):
    o8, l8 = ops.attn_decode_kv8(q, kv8, i32(lens), nh, splits=splits, want_lse=True)
    ob, lb = ops.attn_decode(q, deq, i32(lens), nh, splits=splits, want_lse=True)
    assert biteq(o8, ob) and torch.equal(l8, lb), (splits,)
    assert not torch.isnan(o8.float()).any() and torch.isinf(l8[0]).all() and torch.isfinite(l8[1:]).all()
    o2, l2 = ops.attn_decode_kv8(q, kv8, i32(lens), nh, splits=splits, want_lse=True)
    assert biteq(o8, o2) and torch.equal(l8, l2)  # two runs
    if splits:  # a forced split count: a sequence's result does not depend on what the others hold
      for b in (2, 4):
        o1, l1 = ops.attn_decode_kv8(q[b:b + 1], kv8[b:b + 1], i32(lens[b:b + 1]), nh, splits=splits, want_lse=True)
        assert biteq(o1[0], o8[b]) and torch.equal(l1[0], l8[b]), (splits, b)


def test_attn_decode_kv8_long_context_every_loop_makes_a_second_trip(ops):
  B, Tmax, nh, hd = 2, 1100, 2, 64
  lens = (1100, 1037)
  qrows, kv8 = attn_case('randn', B, Tmax, nh, hd, 9)
  poison(kv8, lens)
  deq = ops.kv8_dequant_rows(kv8, nh, hd)
  q = qrows.view(B, Tmax, -1)[:, -1].contiguous()
  for splits in (1, 3, 0):  # 1100 keys in one split: 128 (hd 64) keys per trip of the four waves
    o8, l8 = ops.attn_decode_kv8(q, kv8, i32(lens), nh, splits=splits, want_lse=True)
    ob, lb = ops.attn_decode(q, deq, i32(lens), nh, splits=splits, want_lse=True)
    assert biteq(o8, ob) and torch.equal(l8, lb), splits


@pytest.mark.parametrize('n', [1, 5, 33, 130])
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_extend_kv8_is_attn_extend_on_the_dequantised_cache(ops, hd, n):
  B, Tmax, nh = 4, 200, 2 if hd < 128 else 1
  lens0 = (Tmax - n, 7, 0, 61)              # a chunk ending on Tmax
  n_new = (n, min(n, 3), 0, n)              # ragged, one empty
  qrows, kv8 = attn_case('peaked' if n == 33 else 'randn', B, Tmax, nh, hd, 5 + n)
  poison(kv8, [a + c for a, c in zip(lens0, n_new)])
  deq = ops.kv8_dequant_rows(kv8, nh, hd)
  q = torch.cat([qrows.view(B, Tmax, -1)[b, min(lens0[b], Tmax - n):][:n] for b in range(B)]).contiguous()
  assert q.shape[0] == B * n
  for splits in (1, 7, 0):
    o8, l8 = ops.attn_extend_kv8(q, kv8, i32(lens0), nh, n_new=i32(n_new), splits=splits, want_lse=True)
    ob, lb = ops.attn_extend(q, deq, i32(lens0), nh, n_new=i32(n_new), splits=splits, want_lse=True)
    assert biteq(o8, ob) and torch.equal(l8, lb), splits
    assert not torch.isnan(o8.float()).any()  # the NaN planted beyond the valid rows did not reach the output
    o2, l2 = ops.attn_extend_kv8(q, kv8, i32(lens0), nh, n_new=i32(n_new), splits=splits, want_lse=True)
    assert biteq(o8, o2) and torch.equal(l8, l2)


# ---- the fused stage and layers -----------------------------------------------------------------------------------------------------------
ROWS = {1: (1, 1), 5: (5, 1), 16: (4, 4), 17: (17, 1), 32: (8, 4)}  # M -> (B, n)


def layer_weights(d, hidden, seed):
  w = lambda s, *shape: (rnd(s, *shape) * 0.05).to(BF16).cuda()  # noqa: E731
  return dict(attn_norm=(1 + 0.1 * rnd(seed, d)).cuda(), mlp_norm=(1 + 0.1 * rnd(seed + 1, d)).cuda(), w_qkv=w(seed + 2, 3 * d, d),
              w_out=w(seed + 3, d, d), w_fc1=w(seed + 4, 2 * hidden, d), w_fc2=w(seed + 5, d, hidden))


@pytest.mark.parametrize('M,d', [(1, 128), (5, 128), (16, 128), (17, 128), (32, 128), (5, 768), (17, 768)])
def test_fused_stage_and_layers_over_kv8(ops, M, d):
  B, n = ROWS[M]
  nh, hd, Tmax, hidden, eps = d // 64, 64, 37, 256, 1e-6
  W = layer_weights(d, hidden, 30)
  cos, sin = (t.cuda() for t in O.rope_table(hd, Tmax))
  x = rnd(40 + M, M, d).cuda()
  lens0 = [(7 * b) % (Tmax - n + 1) for b in range(B)]
  lens0[0] = Tmax - n  # ends on Tmax
  if B > 2:
    lens0[2] = Tmax    # refused
  n_new = None if n == 1 else i32([n if b % 3 else n - 1 for b in range(B)])
  # the stage: the cache holds quantize of what the bf16 stage stores for the same inputs, q_out is equal
  kvb = rnd(41, B, Tmax, 2 * d).to(BF16).cuda()
  kvb0 = kvb.clone()
  kv8, before = sentinel8(42, B, Tmax, d)
  qb, sb = ops.extend_norm_qkv_append(x, W['attn_norm'], eps, W['w_qkv'], i32(lens0), cos, sin, kvb, nh, n_new=n_new)
  q8, s8 = ops.extend_norm_qkv_append_kv8(x, W['attn_norm'], eps, W['w_qkv'], i32(lens0), cos, sin, kv8, nh, n_new=n_new)
  assert biteq(qb, q8) and sb.tolist() == s8.tolist() == [int(B > 2)]
  rows = (kvb.view(torch.int16) != kvb0.view(torch.int16)).any(dim=2).cpu()
  assert int(rows.sum()) == sum(0 if (B > 2 and b == 2) else (n if n_new is None else int(n_new[b])) for b in range(B))
  assert_rows_are_quantize_of(kv8, kvb, rows, before, d)
  # the layers: bit-equal to the composition of their stages
  status = torch.zeros(1, dtype=I32).cuda()
  lens1 = i32([a + 1 for a in lens0])
  for which in ('decode', 'extend') if n == 1 else ('extend',):
    ka = cache8_of((rnd(43, B, Tmax, 2 * d) * 2).to(BF16), Tmax)  # a valid cache: a refused sequence's attention still reads its rows
    kb = ka.clone()
    xa, xb = x.clone(), x.clone()
    q, _ = ops.extend_norm_qkv_append_kv8(xa, W['attn_norm'], eps, W['w_qkv'], i32(lens0), cos, sin, ka, nh, n_new=n_new, status=status)
    if which == 'decode':
      a = ops.attn_decode_kv8(q, ka, lens1, nh)
    else:
      a = ops.attn_extend_kv8(q, ka, i32(lens0), nh, n_new=n_new)
    ops.decode_gemm_residual(xa, a, W['w_out'])
    ops.decode_gemm_residual(xa, ops.decode_norm_fc1_act(xa, W['mlp_norm'], eps, W['w_fc1'], 'glu'), W['w_fc2'])
    if which == 'decode':
      ops.decode_layer_kv8(xb, W['attn_norm'], W['mlp_norm'], eps, W['w_qkv'], W['w_out'], W['w_fc1'], W['w_fc2'], i32(lens0), lens1, cos, sin, kb,
                           nh, 'glu', status)
    else:
      ops.extend_layer_kv8(xb, W['attn_norm'], W['mlp_norm'], eps, W['w_qkv'], W['w_out'], W['w_fc1'], W['w_fc2'], i32(lens0), n_new, cos, sin, kb,
                           nh, 'glu', status)
    assert torch.equal(xa.view(torch.int32), xb.view(torch.int32)) and torch.equal(ka, kb), which
    assert torch.isfinite(xa).all()


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mdl(golden_dir):
  z = np.load(os.path.join(golden_dir, 'model.npz'))
  return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.fixture(scope='module')
def qdq_logits(mdl):
  """forward_qdq of the golden model on its 64 tokens: computed once, shared, never written."""
  w = {k[2:]: v for k, v in mdl.items() if k.startswith('w:')}
  cfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=2)
  return R.forward_qdq(w, cfg, mdl['tokens'][:, :64])


def small(P, mdl, n_layers=2, **kw):
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=n_layers, n_heads=2, mlp='glu', **kw))
  w = {k[2:]: v for k, v in mdl.items() if k.startswith('w:')}
  m.load_state_dict({k: v for k, v in w.items() if k in m.state_dict()})
  return m.cuda()


def relmax(a, ref):
  a, ref = a.double().cpu(), ref.double().cpu()
  return ((a - ref).abs().max() / ref.abs().max()).item()


def teacher_forced(m, tok, prompt_lens, fused, T0=16, T=64):
  B = tok.shape[0]
  x = tok[:, :T0].clone()
  for b, n in enumerate(prompt_lens):
    x[b, n:] = 7  # padding: must not matter
  cache, first = m.prefill(x.cuda(), None if all(n == T0 for n in prompt_lens) else prompt_lens, logits=True)
  assert cache.kv_dtype == 'fp8' and cache.kv[0].dtype == U8
  rows = [first]
  for i in range(T - max(prompt_lens)):
    nxt = torch.stack([tok[b, prompt_lens[b] + i] for b in range(B)]).cuda()
    rows.append(m.decode_step(nxt, cache, logits=True, fused=fused))
  cache.check()
  return torch.stack(rows, dim=1)


# The bound of the model-level test.  Measured on an MI355X: relmax of the teacher-forced logits against forward_qdq is 1.113e-2, unfused
# and fused alike (1.994e-2 against the golden logits of the unquantised model; the ragged prompts reach 1.219e-2).  The margin is the one
# the project grants the bf16 cache against the golden logits, 2e-2 over a measured 4.8e-3: the bound is 4.64e-2.  The CPU flip floor
# (tests/test_kv8_host.py: qdq of bf16-rounded k / v against qdq of fp32 k / v, 1.229e-2 on this model) lies below the bound, as it
# must - the kernels quantise bf16 values, the reference fp32 ones - and is of the size of what was measured: the distance is rounding
# flips across e4m3 boundaries, not an error of the kernels, whose every stage is tested by equality above.
MEASURED_RELMAX = 1.113e-2
MARGIN = 2e-2 / 4.8e-3
FLIP_FLOOR = 1.229e-2


@pytest.mark.parametrize('fused', [False, True])
def test_teacher_forced_logits_vs_forward_qdq(P, mdl, qdq_logits, fused):
  """Logits of the golden model with kv_cache='fp8', teacher-forced over positions 15..63, against tests/kv8_ref.py forward_qdq.
  Measured relmax 1.113e-2 (fused and unfused); bound 1.113e-2 * (2e-2 / 4.8e-3) = 4.64e-2; CPU flip floor 1.229e-2."""
  m = small(P, mdl, kv_cache='fp8')
  logits = teacher_forced(m, mdl['tokens'], (16, 16), fused)
  assert tuple(logits.shape) == (2, 49, 256)
  e = relmax(logits.float(), qdq_logits[:, 15:64])
  print(f'kv_cache=fp8 fused={fused}: teacher-forced logits vs forward_qdq, positions 15..63: relmax {e:.3e}; vs golden {relmax(logits.float(), mdl["logits"][:, 15:64]):.3e}')
  assert MEASURED_RELMAX is not None and FLIP_FLOOR < MEASURED_RELMAX * MARGIN
  assert e < MEASURED_RELMAX * MARGIN


def test_ragged_prompts(P, mdl, qdq_logits):
  m = small(P, mdl, kv_cache='fp8')
  lens = (16, 9)
  logits = teacher_forced(m, mdl['tokens'], lens, False)
  for b, n in enumerate(lens):
    e = relmax(logits[b].float(), qdq_logits[b, n - 1:n + 48])
    print(f'kv_cache=fp8 ragged prompts: sequence {b} positions {n - 1}..{n + 47}: relmax {e:.3e}')
    assert e < MEASURED_RELMAX * MARGIN, (b, e)


def test_chunked_prefill_leaves_the_cache_bits_of_prefill_and_rollback(P, mdl):
  m = small(P, mdl)  # a bf16 model: the format is the cache's own
  tok = mdl['tokens'].cuda()
  want, _ = m.prefill(tok[:, :32], kv_dtype='fp8')
  cache = m.new_cache(2, kv_dtype='fp8')
  assert cache.kv_dtype == 'fp8' and m.new_cache(2).kv_dtype == 'bf16'
  for a, b in ((0, 7), (7, 16), (16, 32)):
    m.extend(tok[:, a:b], cache)
  cache.check()
  assert cache.lens.tolist() == [32, 32]
  for layer in range(2):
    assert torch.equal(cache.kv[layer][:, :32], want.kv[layer][:, :32]), layer
    assert biteq(cache.to_bf16(layer)[:, :32], want.to_bf16(layer)[:, :32])
  # rollback: drop 5 rows, re-append them in one chunk (fused this time): the rows come back, and the next prediction with them
  ref = m.decode_step(tok[:, 32], want, logits=True)
  cache.set_lens(i32([27, 27]))
  m.extend(tok[:, 27:32], cache, fused=True)
  got = m.decode_step(tok[:, 32], cache, logits=True)
  cache.check()
  assert cache.lens.tolist() == [33, 33]
  e = relmax(got.float(), ref.float())
  print(f'kv_cache=fp8 rollback + fused re-append: next logits vs the straight path: relmax {e:.3e}')
  assert e < 2e-2  # fused against unfused rows: the bound the project holds its two step paths to
  # a cache of another model's shape is refused before any library call
  with pytest.raises(ValueError, match='another model shape'):
    small(P, mdl, n_layers=1).decode_step(tok[:, 0], cache)


def test_generate_family_runs_on_the_fp8_cache_and_agrees(P, mdl):
  m = small(P, mdl, kv_cache='fp8')
  draft = small(P, mdl, n_layers=1, kv_cache='bf16')  # a draft chooses its own
  prompt = mdl['tokens'][:, :16].cuda()
  N = 12
  with torch.no_grad():
    base = m.generate(prompt, N)
    assert tuple(base.shape) == (2, N)
    assert torch.equal(m.generate_lookup(prompt, N, n_draft=3), base)
    assert torch.equal(m.generate_speculative(prompt, N, draft, n_draft=3), base)
    fused = m.generate_fused(prompt, N)
    assert torch.equal(m.generate_lookup_fused(prompt, N, n_draft=3), fused)
    agree = (fused == base).float().mean().item()
    print(f'kv_cache=fp8 greedy: generate_fused agrees with generate on {agree:.0%} of {2 * N} tokens')
    assert torch.equal(fused, base)


def test_fp8_fused_step_issues_as_many_calls_as_bf16_and_the_bf16_lists_are_unchanged(P, mdl, monkeypatch):
  from plainlm_amd import _lib
  import test_decode_fused_gpu as DF
  import test_decode_gpu as D
  cfg = dict(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=12, n_heads=2, mlp='glu')
  tok = mdl['tokens'].cuda()
  lists = {}
  for kv in ('bf16', 'fp8'):
    m = P.Transformer(P.ModelConfig(kv_cache=kv, **cfg)).cuda()
    cache, _ = m.prefill(tok[:, :16])
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, 'check', lambda rc, what: calls.append(what) or real(rc, what))
    m.decode_step(tok[:, 16], cache, fused=True)
    lists[kv] = list(calls)
    monkeypatch.undo()
    cache.check()
  assert len(lists['fp8']) == len(lists['bf16']) == 15
  assert lists['bf16'] == ['plm_embed_fwd'] + ['plm_decode_layer_bf16'] * 12 + ['plm_rmsnorm_fwd', 'plm_head_predict_bf16']
  assert lists['fp8'] == [c.replace('plm_decode_layer_bf16', 'plm_decode_layer_kv8_bf16') for c in lists['bf16']]
  # the golden model's bf16 lists, fused and unfused, as their own tests pin them
  m = small(P, mdl)
  cache, _ = m.prefill(tok[:, :16])
  calls = []
  real = _lib.check
  monkeypatch.setattr(_lib, 'check', lambda rc, what: calls.append(what) or real(rc, what))
  m.decode_step(tok[:, 16], cache, fused=True)
  assert calls == DF.FUSED_STEP_CALLS
  del calls[:]
  m.decode_step(tok[:, 17], cache)
  assert calls == D.DECODE_STEP_LAUNCHES
  del calls[:]
  m8 = small(P, mdl, kv_cache='fp8')
  monkeypatch.undo()
  cache8, _ = m8.prefill(tok[:, :16])
  monkeypatch.setattr(_lib, 'check', lambda rc, what: calls.append(what) or real(rc, what))
  m8.decode_step(tok[:, 16], cache8)
  swap = {'plm_kv_append_rope': 'plm_kv8_append_rope_rows', 'plm_attn_decode': 'plm_attn_decode_kv8'}
  assert calls == [swap.get(c, c) for c in D.DECODE_STEP_LAUNCHES]  # the same count, launch for launch
  monkeypatch.undo()
