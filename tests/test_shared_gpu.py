"""Shared-prefix decoding on a real MI355X: plm_attn_decode_shared against an fp64 softmax over the concatenated
prefix and suffix keys under oracle/parity.py's attention bounds (control: plm_attn_decode on the concatenated, replicated cache) and its
bit-equality properties; plm_kv_append_rope_at against plm_kv_append_rope; the fused qkv stage against test_decode_fused_gpu's fp64
reference; decode_step on a SharedPrefixCache and generate_samples on the golden 2-layer model."""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity as PB  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_decode_gpu as TD  # noqa: E402
import test_decode_fused_gpu as TF  # noqa: E402

BF16, I32 = torch.bfloat16, torch.int32
bits, biteq, relmax = TD.bits, TD.biteq, TD.relmax
NP, NH, TP, TS, GMAX = 2, 2, 300, 9, 33
LENS_P = [(0, 257), (1, 300), (63, 256), (64, 65), (255, 1)]  # the edges of the 64-key tile and of the 256-key step; prompts differ
SPLITS_P = (0, 1, 2, 3)


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


def i32(v):
  return torch.tensor(list(v), dtype=I32).cuda()


def lens_s_of(G):
  ls = [(7 * i) % (TS + 1) for i in range(NP * G)]  # ragged; sample 0 has no suffix
  ls[-1] = TS                                        # and the last one a full suffix cache (Ts_max)
  return ls


_data = {}


def data(hd):
  """q [NP*GMAX, d], kv_p [NP, TP, 2d], kv_s [NP*GMAX, TS, 2d] bf16 on the GPU, drawn once per head dim and never modified."""
  if hd not in _data:
    g = torch.Generator().manual_seed(2100 + hd)
    d = NH * hd
    _data[hd] = tuple(torch.randn(*s, generator=g).to(BF16).cuda() for s in ((NP * GMAX, d), (NP, TP, 2 * d), (NP * GMAX, TS, 2 * d)))
  return _data[hd]


def reference(q, kv_p, lp, kv_s, ls, G, hd):
  """fp64 numpy: softmax over the concatenated prefix and suffix keys of each sample.  (out [M, NH, 1, hd], base-2 lse [M, NH, 1])."""
  M, d = NP * G, NH * hd
  q, kv_p, kv_s = (t.double().cpu().numpy() for t in (q, kv_p, kv_s))
  out, lse = np.zeros((M, NH, 1, hd)), np.full((M, NH, 1), np.inf)
  for i in range(M):
    p = i // G
    rows = np.concatenate([kv_p[p, :lp[p]], kv_s[i, :ls[i]]])
    for h in range(NH):
      if len(rows):
        s = rows[:, h * hd:(h + 1) * hd] @ q[i, h * hd:(h + 1) * hd] / np.sqrt(hd) * np.log2(np.e)
        w = np.exp2(s - s.max())
        out[i, h, 0] = w @ rows[:, d + h * hd:d + (h + 1) * hd] / w.sum()
        lse[i, h, 0] = s.max() + np.log2(w.sum())
  return torch.from_numpy(out), torch.from_numpy(lse)


def check_vs_fp64(tag, out, lse, want_o, want_l, hd):
  """test_extend_gpu.check_vs_fp64's bounds; a sample without a key: zero bits, lse +inf."""
  M = out.shape[0]
  got_o, got_l = out.double().cpu().view(M, NH, 1, hd), lse.double().cpu().view(M, NH, 1)
  keyed = torch.isfinite(want_l)
  assert torch.isfinite(out.float()).all() and torch.isfinite(got_l[keyed]).all()
  m = {'row_out': PB.row_local(got_o, want_o)}
  m['proj_out'], m['proj_slice_out'] = PB.projection(got_o, want_o)
  m['lse'] = (got_l[keyed] - want_l[keyed]).abs().max().item() if keyed.any() else 0.0
  print(f'parity {tag}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  assert PB.BOUNDS['row']['out'] == 1.5e-2 and PB.BOUNDS['proj']['out'] == 3e-3 and PB.BOUNDS['proj_slice']['out'] == 3e-3 and PB.BOUNDS['lse'] == 1e-4
  bad = PB.violations(m)
  assert not bad, (tag, bad)
  empty = ~keyed[:, 0, 0]
  assert (bits(out)[empty.cuda()] == 0).all() and (got_l[~keyed] == float('inf')).all(), tag


@pytest.mark.parametrize('G', [1, 5, 32, 33])
@pytest.mark.parametrize('lp', LENS_P)
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_decode_shared_vs_fp64_and_the_replicated_control(ops, hd, lp, G):
  q, kv_p, kv_s = data(hd)
  M = NP * G
  q, kv_s, ls = q[:M], kv_s[:M], lens_s_of(G)
  assert ls[0] == 0 and ls[-1] == TS
  want_o, want_l = reference(q, kv_p, lp, kv_s, ls, G, hd)
  for sp in SPLITS_P:
    out, lse = ops.attn_decode_shared(q, kv_p, i32(lp), kv_s, i32(ls), NH, splits_p=sp, want_lse=True)
    check_vs_fp64(f'shared hd={hd} lens_p={lp} G={G} splits_p={sp}', out, lse, want_o, want_l, hd)
    assert biteq(ops.attn_decode_shared(q, kv_p, i32(lp), kv_s, i32(ls), NH, splits_p=sp), out)  # lse NULL, and two runs
  # the control: what the parent can do - every sample with its own copy of the prompt, one cache
  cat = torch.zeros(M, TP + TS, 2 * NH * hd, dtype=BF16, device='cuda')
  for i in range(M):
    n = lp[i // G]
    cat[i, :n] = kv_p[i // G, :n]
    cat[i, n:n + ls[i]] = kv_s[i, :ls[i]]
  co, cl = ops.attn_decode(q, cat, i32(lp[i // G] + ls[i] for i in range(M)), NH, want_lse=True)
  check_vs_fp64(f'control hd={hd} lens_p={lp} G={G}', co, cl, want_o, want_l, hd)


@pytest.mark.parametrize('G', [5, 33])
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_decode_shared_bit_equalities(ops, hd, G):
  q0, kv_p, kv_s0 = data(hd)
  M, lp = NP * G, (257, TP)
  q, kv_s, ls = q0[:M], kv_s0[:M], lens_s_of(G)
  ls[1] = 0
  assert TS in ls and max(lp) == TP
  other = torch.Generator().manual_seed(5)
  kp_nan, ks_nan = kv_p.clone(), kv_s.clone()  # NaN in every row at and beyond lens_p / lens_s
  kp_nan[0, lp[0]:] = float('nan')
  for i in range(M):
    ks_nan[i, ls[i]:] = float('nan')
  assert torch.isnan(ks_nan[1].float()).all() and not torch.isnan(ks_nan[M - 1].float()).any()
  for sp in SPLITS_P:
    run = lambda q_, kp_, lp_, ks_, ls_: ops.attn_decode_shared(q_, kp_, i32(lp_), ks_, i32(ls_), NH, splits_p=sp, want_lse=True)  # noqa: E731
    out, lse = run(q, kv_p, lp, kv_s, ls)
    o2, l2 = run(q, kp_nan, lp, ks_nan, ls)  # unread rows
    assert biteq(o2, out) and torch.equal(l2, lse), sp
    # lens beyond the caches are clamped to them, negative ones to 0 (over the NaN tails: a clamp that failed would read them)
    o3, l3 = run(q, kp_nan, (257, TP + 4000), ks_nan, [5000 if n == TS else (-3 if n == 0 else n) for n in ls])
    assert biteq(o3, out) and torch.equal(l3, lse), sp
    if sp in (1, 2):
      continue
    # independence: sample i's bits do not depend on the other samples' q rows and suffixes
    i = G + 2
    q4, ks4 = torch.randn(q.shape, generator=other).to(BF16).cuda(), torch.randn(kv_s.shape, generator=other).to(BF16).cuda()
    ls4 = [TS - n for n in ls]
    q4[i], ks4[i], ls4[i] = q[i], kv_s[i], ls[i]
    o4, l4 = run(q4, kv_p, lp, ks4, ls4)
    assert biteq(o4[i], out[i]) and torch.equal(l4[i], lse[i]), sp
    # permuting the samples of a group permutes the output rows
    perm = torch.cat([torch.randperm(G, generator=other), G + torch.randperm(G, generator=other)]).cuda()
    o5, l5 = run(q[perm].contiguous(), kv_p, lp, kv_s[perm].contiguous(), [ls[j] for j in perm.tolist()])
    assert biteq(o5, out[perm]) and torch.equal(l5, lse[perm]), sp
    # an empty sample (no prefix, no suffix): zero bits, lse +inf; the other prompt's samples unchanged
    o6, l6 = run(q, kv_p, (0, TP), kv_s, ls)
    assert (bits(o6[1]) == 0).all() and (l6[1] == float('inf')).all(), sp
    assert biteq(o6[G:], out[G:]) and torch.equal(l6[G:], lse[G:]), sp


# ---- plm_kv_append_rope_at -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_kv_append_rope_at_is_kv_append_rope_at_the_shifted_position(ops, hd):
  B, nh, Ts, RT = 6, 3, 9, 40
  d = nh * hd
  g = torch.Generator().manual_seed(77 + hd)
  cos, sin = (t.cuda() for t in O.rope_table(hd, RT))
  qkv = torch.randn(B, 3 * d + 8, generator=g).to(BF16).cuda()[:, :3 * d]  # a padded row stride
  kv0 = torch.randn(B, Ts, 2 * d, generator=g).to(BF16).cuda()
  row, rot0 = (0, 8, 3, 9, 2, 5), (0, 20, 31, 5, 38, 7)  # sample 3: a row past the cache; sample 4: position 40 past the RoPE table
  ok = [r < Ts and r0 + r < RT for r, r0 in zip(row, rot0)]
  kv = kv0.clone()
  q, status = ops.kv_append_rope_at(qkv, i32(row), i32(rot0), cos, sin, kv, nh, q_out=torch.randn(B, d, generator=g).to(BF16).cuda())
  # the yardstick: plm_kv_append_rope at position rot0 + row into a cache long enough to have that row
  big = torch.zeros(B, RT, 2 * d, dtype=BF16, device='cuda')
  pos = [r0 + r if f else 0 for r, r0, f in zip(row, rot0, ok)]
  qy, _ = ops.kv_append_rope(qkv, i32(pos), cos, sin, big, nh)
  want = kv0.clone()
  for b in range(B):
    if ok[b]:
      assert biteq(q[b], qy[b]), b
      want[b, row[b]] = big[b, pos[b]]
    else:
      assert (bits(q[b]) == 0).all(), b  # zeros, not the sentinel
  assert biteq(kv, want)  # the appended rows hold the yardstick's bits; no other row changed, none of a refused sample
  assert int(status.item()) == 1
  # rot0 = 0 is plm_kv_append_rope, bit for bit
  rows = (0, 8, 3, 1, 2, 5)
  kv1, kv2 = kv0.clone(), kv0.clone()
  q1, s1 = ops.kv_append_rope_at(qkv, i32(rows), i32([0] * B), cos, sin, kv1, nh)
  q2, s2 = ops.kv_append_rope(qkv, i32(rows), cos, sin, kv2, nh)
  assert biteq(q1, q2) and biteq(kv1, kv2) and int(s1.item()) == int(s2.item()) == 0


# ---- the fused qkv stage ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,nh,hd', [(5, 2, 64), (17, 4, 32), (32, 1, 128)])
def test_decode_norm_qkv_append_at_vs_fp64_reference_and_the_unfused_chain(ops, M, nh, hd):
  """test_decode_fused_gpu's stage test with the row and the position told apart: its reference rotates at rot0 + row, its bounds judge."""
  d, Ts = nh * hd, 9
  seed = 3000 * M + hd
  x, nw = TF.rnd(seed, M, d), 1 + 0.1 * TF.rnd(seed + 1, d)
  w_qkv = TF.rnd(seed + 2, 3 * d, d, scale=d ** -0.5).to(BF16)
  cos, sin = O.rope_table(hd, TF.TMAX)
  row = [(3 * i) % Ts for i in range(M)]
  rot0 = [(5 * i) % (TF.TMAX - Ts) for i in range(M)]
  R = TF.s1_reference(x, nw, w_qkv, [a + b for a, b in zip(row, rot0)], cos, sin, nh, hd)
  kv0 = torch.randn(M, Ts, 2 * d, generator=torch.Generator().manual_seed(seed + 3)).to(BF16).cuda()
  xg, nwg, wg, cg, sg = x.cuda(), nw.cuda(), w_qkv.cuda(), cos.cuda(), sin.cuda()
  kv, kvc = kv0.clone(), kv0.clone()
  q, st = ops.decode_norm_qkv_append_at(xg, nwg, TF.EPS_NORM, wg, i32(row), i32(rot0), cg, sg, kv, nh)
  _, n1, _ = ops.rmsnorm_fwd(xg, nwg, TF.EPS_NORM)
  qc, stc = ops.kv_append_rope_at(ops.gemm_nt(n1, wg), i32(row), i32(rot0), cg, sg, kvc, nh)
  ar = torch.arange(M)
  for tag, qq, kk, ss in (('fused', q, kv, st), ('control', qc, kvc, stc)):
    got = kk.cpu()[ar, torch.tensor(row)]
    TF.judge(f'S1-at {tag} q', qq.cpu(), R['rot'][:, :d], R['rot_allow'][:, :d], TF.PO.BOUNDS)
    TF.judge(f'S1-at {tag} k', got[:, :d], R['rot'][:, d:], R['rot_allow'][:, d:], TF.PO.BOUNDS)
    TF.judge(f'S1-at {tag} v', got[:, d:], R['v'], R['v_allow'], TF.PG.BOUNDS)
    want = kv0.clone()
    want[ar.cuda(), i32(row).long()] = kk[ar.cuda(), i32(row).long()]
    assert biteq(kk, want) and int(ss.item()) == 0, tag  # no other row changed


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mdl(golden_dir):
  z = np.load(os.path.join(golden_dir, 'model.npz'))
  return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.fixture(scope='module')
def model(mdl):
  import plainlm_amd
  return TD._small(plainlm_amd, mdl)


@pytest.mark.parametrize('fused', [False, True])
def test_shared_decode_steps_teacher_forced_vs_the_fp32_oracle(model, mdl, fused):
  """P = 2 prompts of different lengths, G = 3 samples with distinct continuations (sample 0: the golden one); every step's logits against
  the fp32 oracle forward of each full sequence, under test_decode_gpu's teacher-forced bound."""
  tok, lens, G, S = mdl['tokens'], (16, 9), 3, 8
  cont = torch.stack([(tok[b, lens[b]:lens[b] + S] + 37 * g) % 256 for b in range(2) for g in range(G)])  # [P*G, S]
  x = tok[:, :16].clone()
  x[1, 9:] = 7  # padding: must not matter
  with torch.no_grad():
    cache, first = model.prefill(x.cuda(), lens, logits=True)
    shared = model.fork(cache, G, S)
    assert shared.rot0.tolist() == [16] * G + [9] * G
    rows = [first.repeat_interleave(G, dim=0)] + [model.decode_step(cont[:, j].cuda(), shared, logits=True, fused=fused) for j in range(S)]
  shared.check()
  assert shared.lens.tolist() == [S] * (2 * G) and cache.lens.tolist() == list(lens)
  got = torch.stack(rows, dim=1).float().cpu()  # [P*G, S + 1, V]: sample i's positions n - 1 + (0 .. S)
  ocfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=2)
  for i in range(2 * G):
    b, n = i // G, lens[i // G]
    ref = O.forward(TD._weights(mdl), ocfg, torch.cat([tok[b, :n], cont[i]])[None])[0, n - 1:]
    e = relmax(got[i], ref)
    print(f'shared teacher-forced fused={fused} sample {i}: relmax vs fp32 oracle {e:.2e}')
    assert e < 2e-2, (i, e)
    if i % G == 0:
      assert relmax(got[i], mdl['logits'][b, n - 1:n + S]) < 2e-2, i
  with torch.no_grad():  # one step past the fork: not stored, flagged
    model.decode_step(cont[:, 0].cuda(), shared, fused=fused)
  with pytest.raises(RuntimeError, match='larger max_new_tokens'):
    shared.check()


@pytest.mark.parametrize('fused', [False, True])
def test_generate_samples(model, mdl, fused):
  prompt, G, N = mdl['tokens'][:, :16].cuda(), 4, 12
  with torch.no_grad():
    t1, l1 = model.generate_samples(prompt, G, N, temperature=1.0, seed=11, return_logprobs=True, fused=fused)
    t2, l2 = model.generate_samples(prompt, G, N, temperature=1.0, seed=11, return_logprobs=True, fused=fused)
    assert t1.dtype == torch.int64 and tuple(t1.shape) == (2, G, N) and tuple(l1.shape) == (2, G, N)
    assert torch.equal(t1, t2) and torch.equal(l1, l2)  # a seed reproduces the call bit for bit
    assert all(len({tuple(r) for r in t1[p].tolist()}) > 1 for p in range(2))  # samples of one prompt differ at temperature 1
    # greedy: every sample's token within 4 eps of the row maximum of the full forward (the near-tie rule of the generate tests)
    toks = model.generate_samples(prompt, G, N, fused=fused)
    for g in range(G):
      full = model(torch.cat([prompt, toks[:, g]], dim=1), None).float()[:, 15:15 + N]
      eps = 2e-2 * full.abs().max().item()
      gap = (full.max(dim=-1).values - full.gather(2, toks[:, g, :, None])[:, :, 0]).max().item()
      assert gap <= 4 * eps, (g, gap, eps)
