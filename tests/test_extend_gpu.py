"""Cache extension on a real MI355X: plm_kv_append_rope_rows against the stand-alone RoPE pass (bit equality),
plm_attn_extend against the fp64 attention reference under oracle/parity.py's bounds and its bit-equality properties (determinism, stale
cache tail, padded chunk rows, independence of the rest of the batch), and Transformer.extend / new_cache on the golden model: chunked
prefill, ragged chunks, a decode step after a chunk, rollback."""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity as PB  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_decode_gpu as TD  # noqa: E402  (the decode tests' data, reference rows and model helpers)

BF16 = torch.bfloat16
bits, biteq, relmax = TD.bits, TD.biteq, TD.relmax
B_, NH, T_ = TD.B_, TD.NH, TD.T_
SPLITS = (1, 2, 7, 64, 0)


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
  return torch.tensor(v, dtype=torch.int32).cuda()


# ---- plm_kv_append_rope_rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_kv_append_rope_rows_is_rope_qk_at_the_chunk_positions(ops, hd):
  B, Tmax, nh = 4, 40, 3
  d = nh * hd
  g = torch.Generator().manual_seed(7 * hd)
  cos, sin = (t.cuda() for t in O.rope_table(hd, Tmax))
  sentinel_kv = torch.randn(B, Tmax, 2 * d, generator=g).to(BF16).cuda()
  # (n, lens0, n_new, refused sequence)
  cases = ((1, (0, 7, 30, 35), None, None), (5, (0, 7, 30, 35), (5, 0, 3, 5), None), (5, (0, 7, 30, 36), (5, 0, 3, 5), 3))
  kept = None
  for n, lens0, n_new, refused in cases:
    qkv = torch.randn(B * n, 3 * d, generator=g).to(BF16).cuda()
    counts = (n,) * B if n_new is None else n_new
    kv = sentinel_kv.clone()
    q_out = torch.randn(B * n, d, generator=g).to(BF16).cuda()  # a sentinel too: every row must be overwritten
    q, status = ops.kv_append_rope_rows(qkv, i32(lens0), cos, sin, kv, nh, n_new=None if n_new is None else i32(n_new), q_out=q_out)
    assert q.data_ptr() == q_out.data_ptr()
    # the yardstick: the same values at the same positions of a [B, Tmax] layout through the stand-alone RoPE pass
    full = torch.zeros(B, Tmax, 3 * d, dtype=BF16, device='cuda')
    for b in range(B):
      for r in range(counts[b]):
        if b != refused:
          full[b, lens0[b] + r] = qkv[b * n + r]
    rot = ops.rope_qk_(full.view(B * Tmax, 3 * d), cos, sin, B, Tmax, nh).view(B, Tmax, 3 * d)
    want_kv = sentinel_kv.clone()
    for b in range(B):
      for r in range(n):
        row, t = b * n + r, lens0[b] + r
        if b == refused or r >= counts[b]:
          assert (bits(q[row]) == 0).all(), (n, b, r)  # zeros, not the sentinel
          continue
        assert biteq(q[row], rot[b, t, :d]), (n, b, r)
        assert biteq(kv[b, t, :d], rot[b, t, d:2 * d]), (n, b, r)
        assert biteq(kv[b, t, d:], qkv[row, 2 * d:]), (n, b, r)  # v: a bit copy
        assert not biteq(q[row], qkv[row, :d]) or t == 0  # position 0 is the identity rotation
        want_kv[b, t] = kv[b, t]
    assert biteq(kv, want_kv)  # no other cache row changed; none at all of a refused sequence
    assert int(status.item()) == (0 if refused is None else 1)
    if n == 5 and refused is None:
      kept = (qkv, kv, q.clone())
    elif n == 5:  # the overflowing run again on the operands of the run before it: the other sequences are what they were
      qkv0, kv0, q0 = kept
      kv2 = sentinel_kv.clone()
      q2, st2 = ops.kv_append_rope_rows(qkv0, i32(lens0), cos, sin, kv2, nh, n_new=i32(n_new))
      assert int(st2.item()) == 1
      assert biteq(kv2[:3], kv0[:3]) and biteq(q2[:15], q0[:15])
      assert biteq(kv2[3], sentinel_kv[3]) and (bits(q2[15:]) == 0).all()


# ---- plm_attn_extend ------------------------------------------------------------------------------------------------------------------
CHUNKS = {33: ((0, 1, 60, 129, 167), (33, 2, 33, 0, 33)),      # crosses the 32-row wave tile and a 64-key tile edge
          130: ((0, 3, 70, 64, 1), (130, 130, 129, 1, 64))}    # crosses a 128-row workgroup tile
_case = {}


def extend_case(ops, hd):
  """test_decode_gpu.decode_case's data (the same generator, the same rotation: its cache is compared bit for bit) with the fp64
  reference of EVERY row kept, computed once per head dim and never modified."""
  if hd not in _case:
    d = NH * hd
    g = torch.Generator().manual_seed(T_ * NH + hd)
    qkv = torch.randn(B_ * T_, 3 * d, generator=g).to(BF16)
    cos, sin = (t.cuda() for t in O.rope_table(hd, T_))
    qrot = ops.rope_qk_(qkv.cuda(), cos, sin, B_, T_, NH)
    ref = PB.reference(qrot.cpu(), torch.zeros(B_ * T_, d), B_, T_, NH, hd)
    q3 = qrot.view(B_, T_, 3 * d)
    kv = q3[:, :, d:].contiguous()
    assert biteq(kv, TD.decode_case(ops, hd)['kv'])
    _case[hd] = dict(kv=kv, q=q3[:, :, :d].contiguous(), out=ref['out'], lse=ref['lse'])  # out [B, nh, T, hd], lse [B, nh, T]
  return _case[hd]


def chunk_q(c, n, lens0, n_new, pad):
  """q [B*n, d]: chunk row r of sequence b = the rotated q of position lens0[b] + r; rows at and beyond n_new[b] hold ``pad``."""
  d = c['q'].shape[2]
  q = torch.full((B_, n, d), pad, dtype=BF16, device='cuda')
  for b in range(B_):
    q[b, :n_new[b]] = c['q'][b, lens0[b]:lens0[b] + n_new[b]]
  return q.view(B_ * n, d)


def chunk_ref(c, n, lens0, n_new, hd):
  """(out [B, nh, n, hd], lse [B, nh, n], valid bool [B, n]) from rows lens0[b] + r of the full causal forward; padded rows: 0 / +inf."""
  out = torch.zeros(B_, NH, n, hd, dtype=torch.float64)
  lse = torch.full((B_, NH, n), float('inf'), dtype=torch.float64)
  valid = torch.zeros(B_, n, dtype=torch.bool)
  for b in range(B_):
    out[b, :, :n_new[b]] = c['out'][b, :, lens0[b]:lens0[b] + n_new[b]]
    lse[b, :, :n_new[b]] = c['lse'][b, :, lens0[b]:lens0[b] + n_new[b]]
    valid[b, :n_new[b]] = True
  return out, lse, valid


def check_vs_fp64(tag, out, lse, want_o, want_l, valid, n, hd):
  assert torch.isfinite(out.float()).all()
  got_o = out.double().cpu().view(B_, n, NH, hd).transpose(1, 2)
  got_l = lse.double().cpu()
  vh = valid[:, None, :].expand(B_, NH, n)
  assert torch.isfinite(got_l[vh]).all()
  m = {'row_out': PB.row_local(got_o, want_o)}
  m['proj_out'], m['proj_slice_out'] = PB.projection(got_o, want_o)
  m['lse'] = (got_l[vh] - want_l[vh]).abs().max().item()
  print(f'parity {tag}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  assert PB.BOUNDS['row']['out'] == 1.5e-2 and PB.BOUNDS['proj']['out'] == 3e-3 and PB.BOUNDS['proj_slice']['out'] == 3e-3 and PB.BOUNDS['lse'] == 1e-4
  bad = PB.violations(m)
  assert not bad, bad
  # rows at and beyond n_new[b]: out bits 0, lse +inf
  assert (bits(out).view(B_, n, -1)[~valid.cuda()] == 0).all()
  assert (lse.cpu()[~vh] == float('inf')).all()


@pytest.mark.parametrize('splits', SPLITS)
@pytest.mark.parametrize('n', [33, 130])
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_extend_vs_fp64_reference(ops, hd, n, splits):
  c = extend_case(ops, hd)
  lens0, n_new = CHUNKS[n]
  q = chunk_q(c, n, lens0, n_new, float('nan'))  # padded q rows are never loaded
  out, lse = ops.attn_extend(q, c['kv'], i32(lens0), NH, n_new=i32(n_new), splits=splits, want_lse=True)
  want_o, want_l, valid = chunk_ref(c, n, lens0, n_new, hd)
  check_vs_fp64(f'extend hd={hd} n={n} splits={splits}', out, lse, want_o, want_l, valid, n, hd)


@pytest.mark.parametrize('splits', SPLITS)
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_extend_one_row_is_decode_attention(ops, hd, splits):
  """n = 1 at lens0 = lens - 1 of the decode tests: the same fp64 rows, the same bounds."""
  c, dc = extend_case(ops, hd), TD.decode_case(ops, hd)
  lens0 = tuple(v - 1 for v in TD.LENS)
  q = chunk_q(c, 1, lens0, (1,) * B_, 0.0)
  assert biteq(q, dc['q'])
  out, lse = ops.attn_extend(q, c['kv'], i32(lens0), NH, splits=splits, want_lse=True)
  valid = torch.ones(B_, 1, dtype=torch.bool)
  check_vs_fp64(f'extend hd={hd} n=1 splits={splits}', out, lse, dc['out'], dc['lse'], valid, 1, hd)


@pytest.mark.parametrize('n', [33, 130])
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_extend_bit_equalities(ops, hd, n):
  c = extend_case(ops, hd)
  kv = c['kv']
  lens0, n_new = CHUNKS[n]
  q = chunk_q(c, n, lens0, n_new, 0.0)
  q_all = chunk_q(c, n, lens0, (n,) * B_, 0.0)  # every sequence has room for n rows: lens0[b] + n <= T
  l0, nn = i32(lens0), i32(n_new)
  for splits in SPLITS:
    run = lambda q_=q, kv_=kv, l0_=l0, nn_=nn, **k: ops.attn_extend(q_, kv_, l0_, NH, n_new=nn_, splits=splits, want_lse=True, **k)  # noqa: E731
    out, lse = run()
    # determinism
    out2, lse2 = run()
    assert biteq(out, out2) and torch.equal(lse, lse2), splits
    # lse NULL: the same out
    assert biteq(ops.attn_extend(q, kv, l0, NH, n_new=nn, splits=splits), out), splits
    # stale tail: NaN in the cache rows at and beyond lens0[b] + n_new[b] against a zero tail
    kv_nan, kv_zero = kv.clone(), kv.clone()
    for b in range(B_):
      kv_nan[b, lens0[b] + n_new[b]:] = float('nan')
      kv_zero[b, lens0[b] + n_new[b]:] = 0
    on_, sn_ = run(kv_=kv_nan)
    oz_, sz_ = run(kv_=kv_zero)
    assert biteq(on_, oz_) and torch.equal(sn_, sz_) and biteq(on_, out) and torch.equal(sn_, lse), splits
    # rows at and beyond n_new[b]: out bits 0, lse +inf
    for b in range(B_):
      assert (bits(out).view(B_, n, -1)[b, n_new[b]:] == 0).all() and (lse[b, :, n_new[b]:] == float('inf')).all(), (splits, b)
      assert torch.isfinite(lse[b, :, :n_new[b]]).all(), (splits, b)
    # n_new NULL is n for every sequence
    oa, sa = ops.attn_extend(q_all, kv, l0, NH, n_new=None, splits=splits, want_lse=True)
    ob, sb = ops.attn_extend(q_all, kv, l0, NH, n_new=i32((n,) * B_), splits=splits, want_lse=True)
    oc, sc = ops.attn_extend(q_all, kv, l0, NH, n_new=i32((n + 9,) * B_), splits=splits, want_lse=True)  # clamped to n
    assert biteq(oa, ob) and torch.equal(sa, sb) and biteq(oa, oc) and torch.equal(sa, sc), splits
    assert torch.isfinite(sa).all()
    # a negative lens0 is clamped to 0 (sequence 0 starts at 0 in both chunk sets)
    assert lens0[0] == 0
    neg = l0.clone()
    neg[0] = -5
    og, sg = run(l0_=neg)
    assert biteq(og, out) and torch.equal(sg, lse), splits
    # independence: a sequence alone, with the same forced split count, gives what it gives inside the batch
    if splits != 0:
      for b in range(B_):
        o1, s1 = ops.attn_extend(q[b * n:(b + 1) * n].contiguous(), kv[b:b + 1].contiguous(), l0[b:b + 1].contiguous(), NH,
                                 n_new=nn[b:b + 1].contiguous(), splits=splits, want_lse=True)
        assert biteq(o1, out[b * n:(b + 1) * n]) and torch.equal(s1[0], lse[b]), (splits, b)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mdl(golden_dir):
  z = np.load(os.path.join(golden_dir, 'model.npz'))
  return {k: torch.from_numpy(z[k]) for k in z.files}


BOUND = 2e-2  # the teacher-forced helper's bound of test_decode_gpu.py


def run_chunks(m, tok, T0, plan):
  """prefill(tok[:, :T0]) (T0 = 0: new_cache) then one extend per entry of plan = [(n, token_lens or None)]: every sequence is fed its
  own next tokens, right-padded with token 7.  Returns (cache, logits [B, T, V] with row p = the all_rows logits of position p where a
  chunk produced it, filled bool [B, T])."""
  B, T = tok.shape[0], 64
  V = m.cfg.vocab_size
  if T0:
    cache, _ = m.prefill(tok[:, :T0].cuda())
  else:
    cache = m.new_cache(B)
  pos = [T0] * B
  logits = torch.zeros(B, T, V)
  filled = torch.zeros(B, T, dtype=torch.bool)
  for n, tl in plan:
    w = [n] * B if tl is None else [int(v) for v in (tl.tolist() if isinstance(tl, torch.Tensor) else tl)]
    x = torch.full((B, n), 7, dtype=torch.int64)
    for b in range(B):
      x[b, :w[b]] = tok[b, pos[b]:pos[b] + w[b]]
    lg = m.extend(x.cuda(), cache, token_lens=tl, logits=True, all_rows=True)
    assert lg.dtype == BF16 and tuple(lg.shape) == (B, n, V)
    for b in range(B):
      logits[b, pos[b]:pos[b] + w[b]] = lg[b, :w[b]].float().cpu()
      filled[b, pos[b]:pos[b] + w[b]] = True
      pos[b] += w[b]
  cache.check()
  assert cache.lens.tolist() == pos and cache.pos.tolist() == [p - 1 for p in pos]
  return cache, logits, filled


def logits_error(logits, filled, golden):
  worst = 0.0
  for b in range(logits.shape[0]):
    worst = max(worst, relmax(logits[b][filled[b]], golden[b, :64][filled[b]]))
  return worst


def cache_mismatch(cache, want, lens):
  """Per layer: the number of bf16 elements of rows < lens[b] that differ in bits from ``want``'s."""
  out = []
  for kv, ref in zip(cache.kv, want.kv):
    out.append(sum(int((bits(kv[b, :n]) != bits(ref[b, :n])).sum()) for b, n in enumerate(lens)))
  return out


PLANS = {'prefill16+5,1,26,16': (16, [(5, None), (1, None), (26, None), (16, None)]),
         'new_cache+7,9,48': (0, [(7, None), (9, None), (48, None)])}


@pytest.mark.parametrize('plan', list(PLANS))
def test_extend_chunks_logits_vs_golden(P, mdl, plan):
  m = TD._small(P, mdl)
  T0, chunks = PLANS[plan]
  _, logits, filled = run_chunks(m, mdl['tokens'], T0, chunks)
  assert filled[:, T0:].all() and not filled[:, :T0].any()
  e = logits_error(logits, filled, mdl['logits'])
  print(f'extend {plan}: all_rows logits of positions {T0}..63 vs golden: relmax {e:.2e}')
  assert e < BOUND


@pytest.mark.parametrize('plan', list(PLANS))
def test_extend_chunks_leave_the_cache_bits_of_a_full_prefill(P, mdl, plan):
  m = TD._small(P, mdl)
  T0, chunks = PLANS[plan]
  cache, _, _ = run_chunks(m, mdl['tokens'], T0, chunks)
  want, _ = m.prefill(mdl['tokens'][:, :64].cuda())
  bad = cache_mismatch(cache, want, (64, 64))
  print(f'extend {plan}: cache elements that differ in bits from a 64-token prefill, per layer: {bad} of {2 * 64 * 256}')
  assert bad == [0, 0]


@pytest.mark.parametrize('on_device', [False, True])
def test_extend_ragged_token_lens(P, mdl, on_device):
  m = TD._small(P, mdl)
  tok = mdl['tokens']
  widths = [(8, 3), (8, 8), (8, 0), (8, 5), (8, 8), (8, 8)]  # sequence 0 reaches 64, sequence 1 stops at 48
  plan = [(8, i32(w) if on_device else w) for w in widths]
  cache, logits, filled = run_chunks(m, tok, 16, plan)
  assert filled[0, 16:].all() and filled[1, 16:48].all() and not filled[1, 48:].any()
  e = logits_error(logits, filled, mdl['logits'])
  print(f'extend ragged ({"device" if on_device else "host"} token_lens): relmax {e:.2e}')
  assert e < BOUND
  want, _ = m.prefill(tok[:, :64].cuda())
  bad = cache_mismatch(cache, want, (64, 48))
  print(f'extend ragged: cache elements that differ in bits from a 64-token prefill, per layer: {bad}')
  assert bad == [0, 0]
  # the default return: the row token_lens[b] - 1 of every sequence, as logits and as a prediction (wind back, append again)
  cache.set_lens(i32((56, 40)))
  x = torch.stack([tok[0, 56:64], tok[1, 40:48]])
  x[1, 5:] = 7
  tl = i32((8, 5)) if on_device else (8, 5)
  last = m.extend(x.cuda(), cache, token_lens=tl, logits=True)
  assert tuple(last.shape) == (2, 256) and cache.lens.tolist() == [64, 45]
  for b, p in enumerate((63, 44)):
    assert relmax(last[b].float(), mdl['logits'][b, p]) < BOUND, b
  cache.set_lens(i32((56, 40)))
  r = m.extend(x.cuda(), cache, token_lens=tl)
  assert tuple(r.tokens.shape) == (2,) and r.tokens.dtype == torch.int64 and (r.logprob <= 0).all() and r.nll is None
  eps = BOUND * mdl['logits'].abs().max().item()
  for b, p in enumerate((63, 44)):
    row = mdl['logits'][b, p].float()
    assert row.max().item() - row[int(r.tokens[b])].item() <= 4 * eps, b
  cache.check()


def test_extend_clamps_a_device_token_lens(P, mdl):
  """A device token_lens is never read back, so it cannot be refused: values outside [0, n] are clamped, for the kernels, for the
  lengths and for the gather of the last rows alike."""
  m = TD._small(P, mdl)
  tok = mdl['tokens']
  cache, _ = m.prefill(tok[:, :16].cuda())
  lg = m.extend(tok[:, 16:24].cuda(), cache, token_lens=i32((99, -4)), logits=True, all_rows=True)
  assert cache.lens.tolist() == [24, 16]
  assert relmax(lg[0].float(), mdl['logits'][0, 16:24]) < BOUND
  r = m.extend(tok[:, 24:32].cuda(), cache, token_lens=i32((99, -4)))
  assert cache.lens.tolist() == [32, 16] and tuple(r.tokens.shape) == (2,)
  last = m.extend(torch.stack([tok[0, 32:40], tok[1, 16:24]]).cuda(), cache, token_lens=i32((8, 99)), logits=True)
  cache.check()
  assert cache.lens.tolist() == [40, 24]
  for b, p in enumerate((39, 23)):
    assert relmax(last[b].float(), mdl['logits'][b, p]) < BOUND, b


def test_decode_step_continues_after_extend(P, mdl):
  m = TD._small(P, mdl)
  tok = mdl['tokens']
  cache, _ = m.prefill(tok[:, :16].cuda())
  m.extend(tok[:, 16:26].cuda(), cache)
  assert cache.lens.tolist() == [26, 26]
  r = m.decode_step(tok[:, 26].cuda(), cache)
  cache.check()
  assert cache.lens.tolist() == [27, 27]
  with torch.no_grad():
    full = m(tok[:, :28].cuda(), None).float()[:, 26]  # row 26 predicts token 27
  eps = 2e-2 * full.abs().max().item()
  gap = (full.max(dim=-1).values - full.gather(1, r.tokens[:, None])[:, 0]).max().item()
  print(f'decode_step after extend: worst (row max - chosen logit) {gap:.3e} against 4 eps = {4 * eps:.3e}')
  assert gap <= 4 * eps


def test_extend_rollback(P, mdl):
  """Speculative decoding's shape: extend by 8, roll back 3, extend the same 3 tokens again."""
  m = TD._small(P, mdl)
  tok = mdl['tokens']
  cache, _ = m.prefill(tok[:, :16].cuda())
  m.extend(tok[:, 16:24].cuda(), cache, logits=True, all_rows=True)
  before = [t.clone() for t in cache.kv]
  cache.set_lens(cache.lens - 3)
  assert cache.lens.tolist() == [21, 21]
  lg = m.extend(tok[:, 21:24].cuda(), cache, logits=True, all_rows=True)
  cache.check()
  assert cache.lens.tolist() == [24, 24]
  e = relmax(lg.float(), mdl['logits'][:, 21:24])
  bad = [int((bits(a[:, :24]) != bits(b[:, :24])).sum()) for a, b in zip(cache.kv, before)]
  print(f'extend rollback: logits of positions 21..23 vs golden relmax {e:.2e}; cache elements changed per layer {bad}')
  assert e < BOUND
  assert bad == [0, 0]


def test_extend_past_the_cache_surfaces_through_check(P, mdl):
  m = TD._small(P, mdl)
  tok = mdl['tokens']
  cache, _ = m.prefill(tok[:, :16].cuda(), max_len=20)
  m.extend(tok[:, 16:20].cuda(), cache)
  cache.check()  # exactly full
  m.extend(tok[:, 20:21].cuda(), cache)
  with pytest.raises(RuntimeError, match='outside'):
    cache.check()
  with pytest.raises(ValueError, match='max_len'):
    m.new_cache(2, max_len=65)
  assert m.new_cache(3, max_len=8).lens.tolist() == [0, 0, 0]


@pytest.mark.parametrize('mlp,nh', [('mlp', 2), ('glu', 4)])
def test_extend_other_mlp_class_and_head_dim_vs_oracle(P, mlp, nh):
  ocfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=nh, mlp=mlp)
  w = O.init_params(ocfg, seed=31 + nh)
  tok = torch.from_numpy(np.random.default_rng(nh).integers(0, 256, size=(2, 64)))
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=nh, mlp=mlp))
  m.load_state_dict(w)
  m = m.cuda()
  _, logits, filled = run_chunks(m, tok, 0, PLANS['new_cache+7,9,48'][1])
  assert filled.all()
  with torch.no_grad():
    ref = O.forward(w, ocfg, tok)
  e = relmax(logits, ref[:, :64])
  print(f'extend mlp={mlp} head_dim={128 // nh} vs fp32 oracle: relmax {e:.2e}')
  assert e < BOUND
