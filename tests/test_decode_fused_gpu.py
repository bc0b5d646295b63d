"""The fused decode step on a real MI355X: the three skinny-M stages against fp64 references that round where the
contract rounds, each next to the unfused chain as a control under the same assertion; plm_decode_layer_bf16 against the composition of
its own stages (bit equality); and the cached model with ``fused=True`` under the bounds of tests/test_decode_gpu.py.

The allowances.  A stage is a chain of roundings, so a reference that rounds where the kernel rounds can differ from an honest kernel by
a whole bf16 ulp of an INTERMEDIATE wherever the exact value lies within fp32 round-off of a rounding boundary.  ``flip`` marks those
elements (the exact value is known to within an allowance; where that reaches the nearest boundary the rounded value may be either
neighbour) and the next link of the chain gets that distance as an absolute allowance, propagated through its own arithmetic:
  norm output     known to (BOUNDS['rstd'] + 2 EPS) |y|: the parity budget's own bound on rstd plus the two fp32 products;
  GEMM output     parity_gemm.allowance (BOUNDS['cond'] sqrt(K) EPS S) + flip(norm) |W|^T;
  RoPE            parity_ops.rope_reference's own allowance + flip(qkv) through |cos|, |sin|;
  activation      the largest change of the fp64 reference when gate / up move to a neighbour they may have flipped to;
  residual        flip(GEMM output) + the one fp32 rounding of the add (2 EPS |x|, doubled as parity_ops doubles its allowances).
Nothing is fitted to an output.  The metrics and bounds are parity_ops.elementwise with parity_ops.BOUNDS (ulp 4, neq 5e-3) on what passed
RoPE or an activation and with parity_gemm.BOUNDS (ulp 1, neq 2e-2) on a bare GEMM output."""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity_gemm as PG  # noqa: E402
from oracle import parity_ops as PO  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BF16, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
EPS_NORM = 1e-6
TMAX = 37
MS = (1, 5, 16, 17, 32)
HEADS = ((3, 32), (2, 64), (1, 128))
HIDDEN = 288  # 9 K steps of 32: the four waves of a workgroup get 3, 3, 3 and 0 of them
# (M, nh, hd, hidden): every row count on every head shape; d = 768 with hidden 2048 at M = 5 (a K loop of several chunks, K steps split
# 6 / 6 / 6 / 6 and 8 x 4) and at M = 17 (the two-MFMA body's 512-column chunks)
SHAPES = [(M, nh, hd, HIDDEN) for M in MS for nh, hd in HEADS] + [(5, 12, 64, 2048), (17, 12, 64, 2048)]
KINDS = ('glu', 'silu', 'relu_sq')


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


def bits(t):
  return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def biteq(a, b):
  return torch.equal(bits(a), bits(b))


def rnd(seed, *shape, scale=1.0):
  return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


# ---- the allowance algebra ---------------------------------------------------------------------------------------------------------------
def flip(ref, allow):
  """How far bf16(v) can lie from bf16_rne(ref) when v is known to lie within ``allow`` of ref: 0 where no rounding boundary is within
  ``allow`` of ref on either side (both round to the same value), else ``allow`` plus one ulp (the larger neighbour spacing: half an ulp
  of rounding on each side).  With an allowance far below an ulp that is one ulp on the few elements next to a boundary; where an
  upstream flip has made the allowance several ulps it grows with it."""
  a, ra = ref.abs(), PO.bf16_rne(ref).abs()
  up = PO.ulp_of(ra)
  lo = PO.ulp_of(ra * (1 - 2.0 ** -12))  # the spacing just below |r| (half of ``up`` at a power of two)
  d_up = ra + up / 2 - a
  d_lo = a - (ra - lo / 2)
  return torch.where(torch.minimum(d_up, d_lo) <= allow + PO.FLOOR, allow + up, torch.zeros_like(up))


def norm_ref(x, w):
  """(bf16 tensor of the correctly rounded norm output, flip allowance of its elements) from the fp32 x, w the kernel reads."""
  y, _ = PO.rmsnorm_fwd_reference(x, w, EPS_NORM)
  return PO.bf16_rne(y).to(BF16), flip(y, (PO.BOUNDS['rstd'] + 2 * PO.EPS) * y.abs())


def gemm_ref(a_bf, w_bf, e_a=None):
  """(fp64 un-rounded a w^T, its allowance) for bf16 a [M, K] whose elements may be off by e_a, w [N, K]."""
  R = PG.reference(a_bf.cpu(), w_bf.cpu())
  allow = PG.allowance(R)
  if e_a is not None:
    allow = allow + e_a @ w_bf.cpu().double().abs().t()
  return R['ref'], allow


def judge(tag, got, ref, allow, bounds):
  m = PO.elementwise(got, ref, allow)
  print(f'decode_fused {tag}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  bad = {k: (v, bounds[k]) for k, v in m.items() if not v <= bounds[k]}
  assert not bad, (tag, bad)


def positions(M):
  """One decode position per sequence: the cache's first and last row, one sequence past its end and one before its start (neither is
  stored), the rest inside."""
  base = [0, TMAX - 1, TMAX, 3, -1, 17, 36, 1]
  return (base + [(5 * i) % TMAX for i in range(M)])[:M]


def stored(pos):
  return [0 <= t < TMAX for t in pos]


# ---- S1: norm + qkv + RoPE + append ------------------------------------------------------------------------------------------------------
def s1_reference(x, nw, w_qkv, pos, cos, sin, nh, hd):
  d = nh * hd
  n_b, e_n = norm_ref(x, nw)
  ref, allow = gemm_ref(n_b, w_qkv, e_n)
  e_qkv = flip(ref, allow)
  qkv_b = PO.bf16_rne(ref).to(BF16)
  tp = torch.tensor(pos).clamp(0, TMAX - 1)
  M = x.shape[0]
  rot, rallow = PO.rope_reference(qkv_b, cos[tp], sin[tp], 1, M, nh)  # row r at table row r = position pos[r]
  ea, eb = e_qkv[:, :2 * d].reshape(M, 2 * nh, hd // 2, 2).unbind(-1)
  c, s = cos[tp].double().abs().reshape(M, 1, hd // 2), sin[tp].double().abs().reshape(M, 1, hd // 2)
  rallow = rallow + torch.stack([ea * c + eb * s, eb * c + ea * s], -1).reshape(M, 2 * d)
  return dict(rot=rot, rot_allow=rallow, v=ref[:, 2 * d:], v_allow=allow[:, 2 * d:])


def s1_check(tag, R, q, kv, status, kv0, pos, d):
  ok = stored(pos)
  rows = [b for b, f in enumerate(ok) if f]
  want_kv = kv0.clone()
  if rows:
    k_got = torch.stack([kv[b, pos[b], :d] for b in rows])
    v_got = torch.stack([kv[b, pos[b], d:2 * d] for b in rows])
    judge(tag + ' q', q[rows], R['rot'][rows, :d], R['rot_allow'][rows, :d], PO.BOUNDS)
    judge(tag + ' k', k_got, R['rot'][rows, d:], R['rot_allow'][rows, d:], PO.BOUNDS)
    judge(tag + ' v', v_got, R['v'][rows], R['v_allow'][rows], PG.BOUNDS)
    for b in rows:
      want_kv[b, pos[b]] = kv[b, pos[b]]
  assert biteq(kv, want_kv), tag  # no other cache row changed, a refused sequence's rows and the pad columns included
  for b, f in enumerate(ok):
    if not f:
      assert (bits(q[b]) == 0).all(), (tag, b)  # the zero q row of a refused sequence
  assert int(status.item()) == (0 if all(ok) else 1), tag


@pytest.mark.parametrize('M,nh,hd,hidden', SHAPES)
def test_norm_qkv_append_vs_fp64_reference_and_the_unfused_chain(ops, M, nh, hd, hidden):
  d = nh * hd
  seed = 1000 * M + 10 * nh + hd
  x, nw = rnd(seed, M, d), 1 + 0.1 * rnd(seed + 1, d)
  w_qkv = rnd(seed + 2, 3 * d, d, scale=d ** -0.5).to(BF16)
  cos, sin = O.rope_table(hd, TMAX)
  pos = positions(M)
  kv0 = torch.randn(M, TMAX, 2 * d + 8, generator=torch.Generator().manual_seed(seed + 3)).to(BF16).cuda()  # padded row stride
  R = s1_reference(x, nw, w_qkv, pos, cos, sin, nh, hd)
  xg, nwg, wg, cg, sg = x.cuda(), nw.cuda(), w_qkv.cuda(), cos.cuda(), sin.cuda()
  pg = torch.tensor(pos, dtype=I32).cuda()
  # the fused stage
  kv = kv0.clone()
  q, status = ops.decode_norm_qkv_append(xg, nwg, EPS_NORM, wg, pg, cg, sg, kv[:, :, :2 * d], nh)
  s1_check(f'S1 fused M={M} nh={nh} hd={hd}', R, q.cpu(), kv.cpu(), status, kv0.cpu(), pos, d)
  assert biteq(xg.cpu(), x)
  # the control: rmsnorm_fwd -> gemm_nt -> kv_append_rope, under the same assertion
  kvc = kv0.clone()
  qc = torch.zeros(M, d, dtype=BF16, device='cuda')
  _, n1, _ = ops.rmsnorm_fwd(xg, nwg, EPS_NORM)
  _, stc = ops.kv_append_rope(ops.gemm_nt(n1, wg), pg, cg, sg, kvc[:, :, :2 * d], nh, q_out=qc)
  s1_check(f'S1 control M={M} nh={nh} hd={hd}', R, qc.cpu(), kvc.cpu(), stc, kv0.cpu(), pos, d)
  # what passes through no sum is the control's bits
  assert int(status.item()) == int(stc.item())
  for b, f in enumerate(stored(pos)):
    if not f:
      assert biteq(q[b], qc[b]) and biteq(kv[b], kvc[b]), b
  # two runs are bit-equal
  kv2 = kv0.clone()
  q2, _ = ops.decode_norm_qkv_append(xg, nwg, EPS_NORM, wg, pg, cg, sg, kv2[:, :, :2 * d], nh)
  assert biteq(q2, q) and biteq(kv2, kv)


# ---- S2: GEMM + residual ---------------------------------------------------------------------------------------------------------------------
def s2_check(tag, got, x0, ref, allow):
  want = x0.double() + PO.bf16_rne(ref)
  add = 2 * PO.EPS * want.abs()  # the one fp32 rounding of the add, doubled
  err = (got.double().cpu() - want).abs()
  assert torch.isfinite(got).all(), tag
  slack = flip(ref, allow) + add + PO.FLOOR
  worst = (err / slack).max().item()
  flipped = (err > add + PO.FLOOR).sum().item() / max(err.numel(), PO.NEQ_MIN)
  print(f'decode_fused {tag}: worst err / allowance {worst:.2e}, share beyond the add\'s rounding {flipped:.2e}')
  assert worst <= 1.0, (tag, worst)
  assert flipped <= PG.BOUNDS['neq'], (tag, flipped)


@pytest.mark.parametrize('M,nh,hd,hidden', SHAPES)
def test_gemm_residual_vs_fp64_reference_and_the_unfused_chain(ops, M, nh, hd, hidden):
  d = nh * hd
  seed = 2000 * M + 10 * nh + hd
  for K in (d, hidden):  # the out projection and fc2
    x0 = rnd(seed + K, M, d)
    a = rnd(seed + K + 1, M, K).to(BF16)
    w = rnd(seed + K + 2, d, K, scale=K ** -0.5).to(BF16)
    ref, allow = gemm_ref(a, w)
    ag, wg = a.cuda(), w.cuda()
    xg = x0.clone().cuda()
    out = ops.decode_gemm_residual(xg, ag, wg)
    assert out.data_ptr() == xg.data_ptr()
    s2_check(f'S2 fused M={M} N={d} K={K}', xg.cpu(), x0, ref, allow)
    xc = x0.cuda() + ops.gemm_nt(ag, wg).float()  # the control: gemm_nt + add
    s2_check(f'S2 control M={M} N={d} K={K}', xc.cpu(), x0, ref, allow)
    x2 = x0.clone().cuda()
    ops.decode_gemm_residual(x2, ag, wg)
    assert biteq(x2, xg)


# ---- S3: norm + fc1 + activation -------------------------------------------------------------------------------------------------------------
def act_fp64(u, kind):
  return PO.swiglu_fwd_reference(u) if kind == 'glu' else PO.act_fwd_reference(u, kind)


def s3_reference(x, nw, w_fc1, kind):
  n_b, e_n = norm_ref(x, nw)
  ref, allow = gemm_ref(n_b, w_fc1, e_n)
  e_u = flip(ref, allow)
  u = PO.bf16_rne(ref)
  f0 = act_fp64(u, kind)
  h = f0.shape[1]
  worst = torch.zeros_like(f0)
  for sx in (0.0, 1.0, -1.0):  # gate (or the only operand) at itself and at either neighbour it may have flipped to; the same for up
    for sz in ((0.0, 1.0, -1.0) if kind == 'glu' else (0.0,)):
      step = torch.cat([sx * e_u[:, :h], sz * e_u[:, h:]], 1) if kind == 'glu' else sx * e_u
      worst = torch.maximum(worst, (act_fp64(u + step, kind) - f0).abs())
  return f0, worst


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('M,nh,hd,hidden', SHAPES)
def test_norm_fc1_act_vs_fp64_reference_and_the_unfused_chain(ops, M, nh, hd, hidden, kind):
  d = nh * hd
  seed = 3000 * M + 10 * nh + hd + KINDS.index(kind)
  x, nw = rnd(seed, M, d), 1 + 0.1 * rnd(seed + 1, d)
  w_fc1 = rnd(seed + 2, (2 if kind == 'glu' else 1) * hidden, d, scale=2 * d ** -0.5).to(BF16)
  ref, allow = s3_reference(x, nw, w_fc1, kind)
  xg, nwg, wg = x.cuda(), nw.cuda(), w_fc1.cuda()
  act = ops.decode_norm_fc1_act(xg, nwg, EPS_NORM, wg, kind)
  assert act.dtype == BF16 and tuple(act.shape) == (M, hidden)
  judge(f'S3 fused {kind} M={M} d={d} h={hidden}', act.cpu(), ref, allow, PO.BOUNDS)
  u = ops.gemm_nt(ops.rmsnorm_fwd(xg, nwg, EPS_NORM)[1], wg)
  ctl = ops.swiglu_fwd(u) if kind == 'glu' else ops.act_fwd(u, kind)
  judge(f'S3 control {kind} M={M} d={d} h={hidden}', ctl.cpu(), ref, allow, PO.BOUNDS)
  assert biteq(ops.decode_norm_fc1_act(xg, nwg, EPS_NORM, wg, kind), act) and biteq(xg.cpu(), x)


# ---- the layer driver adds nothing -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('M,nh,hd', [(5, 3, 32), (17, 2, 64), (32, 1, 128)])
def test_decode_layer_is_the_composition_of_its_stages(ops, M, nh, hd, kind):
  d, hidden = nh * hd, HIDDEN
  seed = 4000 * M + hd + KINDS.index(kind)
  x0 = rnd(seed, M, d).cuda()
  an, mn = (1 + 0.1 * rnd(seed + 1, d)).cuda(), (1 + 0.1 * rnd(seed + 2, d)).cuda()
  w_qkv = rnd(seed + 3, 3 * d, d, scale=d ** -0.5).to(BF16).cuda()
  w_out = rnd(seed + 4, d, d, scale=d ** -0.5).to(BF16).cuda()
  w_fc1 = rnd(seed + 5, (2 if kind == 'glu' else 1) * hidden, d, scale=d ** -0.5).to(BF16).cuda()
  w_fc2 = rnd(seed + 6, d, hidden, scale=hidden ** -0.5).to(BF16).cuda()
  cos, sin = (t.cuda() for t in O.rope_table(hd, TMAX))
  pos = positions(M)
  pg = torch.tensor(pos, dtype=I32).cuda()
  lens = (pg + 1).clamp(0, TMAX)
  kv0 = torch.randn(M, TMAX, 2 * d + 8, generator=torch.Generator().manual_seed(seed + 7)).to(BF16).cuda()
  for splits in (0, 3):
    x1, kv1, st1 = x0.clone(), kv0.clone(), torch.zeros(1, dtype=I32, device='cuda')
    q, _ = ops.decode_norm_qkv_append(x1, an, EPS_NORM, w_qkv, pg, cos, sin, kv1[:, :, :2 * d], nh, status=st1)
    ops.decode_gemm_residual(x1, ops.attn_decode(q, kv1[:, :, :2 * d], lens, nh, splits=splits), w_out)
    ops.decode_gemm_residual(x1, ops.decode_norm_fc1_act(x1, mn, EPS_NORM, w_fc1, kind), w_fc2)
    x2, kv2, st2 = x0.clone(), kv0.clone(), torch.zeros(1, dtype=I32, device='cuda')
    out = ops.decode_layer(x2, an, mn, EPS_NORM, w_qkv, w_out, w_fc1, w_fc2, pg, lens, cos, sin, kv2[:, :, :2 * d], nh, kind, st2, splits=splits)
    assert out.data_ptr() == x2.data_ptr()
    assert biteq(x2, x1) and biteq(kv2, kv1) and torch.equal(st2, st1), (splits, kind)
    assert torch.isfinite(x2).all() and not biteq(x2, x0) and int(st2.item()) == (0 if all(stored(pos)) else 1)
    ws = ops.decode_layer_workspace(M, nh, hd, hidden, TMAX, splits, 'cuda')  # a caller-owned workspace: the same bits
    x3, kv3 = x0.clone(), kv0.clone()
    ops.decode_layer(x3, an, mn, EPS_NORM, w_qkv, w_out, w_fc1, w_fc2, pg, lens, cos, sin, kv3[:, :, :2 * d], nh, kind, st2, splits=splits, workspace=ws)
    assert biteq(x3, x1) and biteq(kv3, kv1)


def test_ops_refuse_what_the_kernels_do_not_serve(ops):
  x = torch.zeros(33, 128, device='cuda')
  w = torch.zeros(128, 128, dtype=BF16, device='cuda')
  with pytest.raises(ValueError, match='33 rows'):
    ops.decode_gemm_residual(x, torch.zeros(33, 128, dtype=BF16, device='cuda'), w)
  with pytest.raises(ValueError, match='mlp kind'):
    ops.decode_norm_fc1_act(x[:4].contiguous(), torch.ones(128, device='cuda'), 1e-6, w, 'gelu')
  with pytest.raises(RuntimeError, match='unsupported shape'):  # K % 32 != 0: the library refuses, nothing falls back
    ops.decode_gemm_residual(x[:4].contiguous(), torch.zeros(4, 48, dtype=BF16, device='cuda'), torch.zeros(128, 48, dtype=BF16, device='cuda'))


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mdl(golden_dir):
  z = np.load(os.path.join(golden_dir, 'model.npz'))
  return {k: torch.from_numpy(z[k]) for k in z.files}


def _small(P, mdl):
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  m.load_state_dict({k[2:]: v for k, v in mdl.items() if k.startswith('w:')})
  return m.cuda()


def relmax(a, ref):
  a, ref = a.double().cpu(), ref.double().cpu()
  return ((a - ref).abs().max() / ref.abs().max()).item()


def _teacher_forced(m, tok, prompt_lens, T0=16, T=64):
  """tests/test_decode_gpu.py's walk with fused=True: prefill tok[:, :T0], then feed every sequence its own true next tokens."""
  B = tok.shape[0]
  x = tok[:, :T0].clone()
  for b, n in enumerate(prompt_lens):
    x[b, n:] = 7  # padding: must not matter
  cache, first = m.prefill(x.cuda(), None if all(n == T0 for n in prompt_lens) else prompt_lens, logits=True)
  steps = T - max(prompt_lens)
  rows = [first]
  for i in range(steps):
    nxt = torch.stack([tok[b, prompt_lens[b] + i] for b in range(B)]).cuda()
    rows.append(m.decode_step(nxt, cache, logits=True, fused=True))
  cache.check()
  assert cache.lens.tolist() == [n + steps for n in prompt_lens]
  return torch.stack(rows, dim=1)


def test_fused_cached_logits_vs_golden(P, mdl):
  m = _small(P, mdl)
  logits = _teacher_forced(m, mdl['tokens'], (16, 16))
  assert logits.dtype == BF16 and tuple(logits.shape) == (2, 49, 256)
  e = relmax(logits.float(), mdl['logits'][:, 15:64])
  print(f'fused teacher-forced cached logits vs golden, positions 15..63: relmax {e:.2e}')
  assert e < 2e-2


def test_fused_cached_logits_with_ragged_prompt_lens(P, mdl):
  m = _small(P, mdl)
  lens = (16, 9)
  logits = _teacher_forced(m, mdl['tokens'], lens)
  assert tuple(logits.shape) == (2, 49, 256)
  for b, n in enumerate(lens):
    e = relmax(logits[b].float(), mdl['logits'][b, n - 1:n + 48])
    print(f'fused ragged prompts: sequence {b} positions {n - 1}..{n + 47}: relmax {e:.2e}')
    assert e < 2e-2, (b, e)


@pytest.mark.parametrize('mlp,nh', [('mlp', 2), ('mlp_relu_sq', 2), ('glu', 4), ('glu', 1)])
def test_fused_cached_logits_other_mlp_classes_and_head_dims_vs_oracle(P, mlp, nh):
  ocfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=nh, mlp=mlp)
  w = O.init_params(ocfg, seed=31 + nh)
  tok = torch.from_numpy(np.random.default_rng(nh).integers(0, 256, size=(2, 64)))
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=nh, mlp=mlp))
  m.load_state_dict(w)
  m = m.cuda()
  logits = _teacher_forced(m, tok, (16, 16))
  with torch.no_grad():
    ref = O.forward(w, ocfg, tok)
  e = relmax(logits.float(), ref[:, 15:64])
  print(f'fused cached logits mlp={mlp} head_dim={128 // nh} vs fp32 oracle: relmax {e:.2e}')
  assert e < 2e-2


FUSED_STEP_CALLS = ['plm_embed_fwd', 'plm_decode_layer_bf16', 'plm_decode_layer_bf16', 'plm_rmsnorm_fwd', 'plm_head_predict_bf16']


def test_fused_step_issues_one_library_call_per_layer_and_the_default_is_unchanged(P, mdl, monkeypatch):
  from plainlm_amd import _lib
  import test_decode_gpu as D
  m = _small(P, mdl)
  tok = mdl['tokens'].cuda()
  cache, _ = m.prefill(tok[:, :16])
  calls = []
  real = _lib.check
  monkeypatch.setattr(_lib, 'check', lambda rc, what: calls.append(what) or real(rc, what))
  m.decode_step(tok[:, 16], cache, fused=True)
  assert calls == FUSED_STEP_CALLS, calls
  del calls[:]
  m.decode_step(tok[:, 17], cache)  # fused=False, the default: the pinned list
  assert calls == D.DECODE_STEP_LAUNCHES, calls
  monkeypatch.undo()
  cache.check()
  assert cache.lens.tolist() == [18, 18]


def test_generate_fused_greedy_against_the_full_forward(P, mdl):
  """generate()'s parameter list is pinned by tests/test_sample_host.py, so fused generation is the method generate_fused: generate's
  arguments, every decode step with fused=True."""
  m = _small(P, mdl)
  prompt = mdl['tokens'][:, :16].cuda()
  N = 32
  with torch.no_grad():
    toks, lps = m.generate_fused(prompt, N, return_logprobs=True)
    assert toks.dtype == torch.int64 and tuple(toks.shape) == (2, N) and lps.dtype == torch.float32 and tuple(lps.shape) == (2, N)
    seq = torch.cat([prompt, toks], dim=1)
    full = m(seq, None).float()  # row 15 + i predicts generated token i
    eps = 2e-2 * full.abs().max().item()
    rows = full[:, 15:15 + N]
    chosen = rows.gather(2, toks[:, :, None])[:, :, 0]
    gap = (rows.max(dim=-1).values - chosen).max().item()
    share = (rows.argmax(-1) == toks).float().mean().item()
    print(f'fused generate vs full forward: worst (row max - chosen logit) {gap:.3e} against 4 eps = {4 * eps:.3e}; exact matches with the '
          f'recompute argmax {share:.4f}')
    assert gap <= 4 * eps  # every generated position, none excluded
    tg = torch.full_like(seq, -100)
    tg[:, 15:15 + N] = toks
    want = -m.predict(seq, targets=tg).nll[:, 15:15 + N]
    assert (lps - want).abs().max().item() <= eps, ((lps - want).abs().max().item(), eps)
    assert (lps <= 0).all()
    t2, l2 = m.generate_fused(prompt, N, return_logprobs=True)  # two runs are bit-equal
    assert torch.equal(t2, toks) and torch.equal(l2, lps)
    assert torch.equal(m.generate_fused(prompt, N), toks)


def test_fused_refuses_more_than_32_sequences(P, mdl):
  m = _small(P, mdl)
  tok = torch.zeros(33, dtype=torch.int64, device='cuda')
  cache = m.new_cache(33)
  with pytest.raises(ValueError, match='leave fused off'):
    m.decode_step(tok, cache, fused=True)
  assert cache.lens.tolist() == [0] * 33  # refused before anything moved
  with torch.no_grad(), pytest.raises(ValueError, match='leave fused off'):
    m.generate_fused(torch.zeros(33, 16, dtype=torch.int64, device='cuda'), 4)
  with torch.no_grad():  # 32 is served
    assert tuple(m.generate_fused(torch.zeros(32, 16, dtype=torch.int64, device='cuda'), 2).shape) == (32, 2)
