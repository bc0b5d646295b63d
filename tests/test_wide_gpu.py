"""The wide fused layer on a real MI355X: its three stages against the fp64 references of
tests/test_decode_fused_gpu.py (which round where the contract rounds; the unfused chain runs as control under the same assertion), the
qkv stage's addresses and refusals, row independence by bit equality, the layer against its stages' bits, and the model through
step_ragged / serve with fused='wide' under the bounds of tests/test_ragged_gpu.py."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity_gemm as PG  # noqa: E402
from oracle import parity_ops as PO  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_decode_gpu as TD  # noqa: E402
from test_decode_fused_gpu import BF16, EPS_NORM, KINDS, flip, gemm_ref, judge, norm_ref, rnd, s2_check, s3_reference  # noqa: E402
from test_decode_gpu import P, biteq, bits, mdl, ops  # noqa: E402,F401
from test_paged_gpu import _model, _scrambled_pool, i32, paginate  # noqa: E402

# M: one row, both sides of the 16-, 32- and 64-row tile boundaries, four full tiles.  (nh, hd) = (3, 32) with hidden 288: K = 96 is one
# chunk of 3 steps (1 / 1 / 1 / 0 over the waves), K = 288 a full chunk (2 / 2 / 2 / 2) and a tail chunk of one step (1 / 0 / 0 / 0).
# d = 768 with hidden 2048 at M = 65: 3 and 8 pipelined chunks, and a second row tile of one row.
MS = (1, 16, 17, 32, 33, 64, 65, 256)
SHAPES = [(M, 3, 32, 288) for M in MS] + [(65, 12, 64, 2048)]
TMAX = 320  # five pages


def packing(M):
  """(lens0, counts) of M packed rows: a chunk across page edges, an idle slot, a prompt from nothing."""
  return (60, 130, 0), (M - M // 3, 0, M // 3)


def positions(lens0, counts):
  return [a + j for a, c in zip(lens0, counts) for j in range(c)]


def qkv_reference(x, nw, w_qkv, pos, cos, sin, nh, hd):
  """test_decode_fused_gpu.s1_reference with row m at table row pos[m] = lens0[b] + j."""
  d, M = nh * hd, x.shape[0]
  n_b, e_n = norm_ref(x, nw)
  ref, allow = gemm_ref(n_b, w_qkv, e_n)
  e_qkv = flip(ref, allow)
  tp = torch.tensor(pos)
  rot, rallow = PO.rope_reference(PO.bf16_rne(ref).to(BF16), cos[tp], sin[tp], 1, M, nh)
  ea, eb = e_qkv[:, :2 * d].reshape(M, 2 * nh, hd // 2, 2).unbind(-1)
  c, s = cos[tp].double().abs().reshape(M, 1, hd // 2), sin[tp].double().abs().reshape(M, 1, hd // 2)
  rallow = rallow + torch.stack([ea * c + eb * s, eb * c + ea * s], -1).reshape(M, 2 * d)
  return dict(rot=rot, rot_allow=rallow, v=ref[:, 2 * d:], v_allow=allow[:, 2 * d:])


def qkv_case(ops, M, nh, hd, lens0=None, counts=None, seed=0):
  d = nh * hd
  if counts is None:
    lens0, counts = packing(M)
  g = lambda i, *s, k=1.0: rnd(7000 * M + 10 * nh + hd + i + seed, *s, scale=k)  # noqa: E731
  cos, sin = O.rope_table(hd, TMAX)
  old = g(3, len(counts), TMAX, 2 * d).to(BF16).cuda()
  pool, table = paginate(old, [min(a + c, TMAX) for a, c in zip(lens0, counts)], M)
  cu, row_seq, _, NT = ops.ragged_plan(counts)
  return dict(x=g(0, M, d), nw=1 + 0.1 * g(1, d), w=g(2, 3 * d, d, k=d ** -0.5).to(BF16), cos=cos, sin=sin, pool=pool, table=table, lens0=lens0,
              counts=counts, cu=cu, rs=row_seq, NT=NT, d=d, nh=nh)


def run_qkv(ops, c, control=False, order=None):
  """The stage (or the unfused chain) on a fresh copy of the pool; order: the sequences packed in another order.  Returns (q, pool, status)."""
  cu, rs, x, l0, table = c['cu'], c['rs'], c['x'], c['lens0'], c['table']
  if order is not None:
    cu, rs, _, _ = ops.ragged_plan([c['counts'][b] for b in order])
    x = torch.cat([c['x'][c['cu'][b]:c['cu'][b + 1]] for b in order])
    l0, table = [c['lens0'][b] for b in order], c['table'][list(order)].contiguous()
  pool = c['pool'].clone()
  a = (i32(l0), cu.cuda(), rs.cuda(), c['cos'].cuda(), c['sin'].cuda(), pool, table, c['nh'])
  if control:
    q, st = ops.kv_paged_append_rope_packed(ops.gemm_nt(ops.rmsnorm_fwd(x.cuda(), c['nw'].cuda(), EPS_NORM)[1], c['w'].cuda()), *a)
  else:
    q, st = ops.ragged_norm_qkv_append_paged_wide(x.cuda(), c['nw'].cuda(), EPS_NORM, c['w'].cuda(), *a)
  return q, pool, st


def stored_rows(c, pool):
  """The k | v rows of the packed rows, read back through the table."""
  t = c['table'].cpu()
  return torch.stack([pool[int(t[b, p // 64]), p % 64] for b, (a, n) in enumerate(zip(c['lens0'], c['counts'])) for p in range(a, a + n)]).cpu()


@pytest.mark.parametrize('M,nh,hd', [s[:3] for s in SHAPES] + [(65, 2, 64), (65, 1, 128)])
def test_wide_qkv_stage_vs_fp64_reference_and_the_unfused_chain(ops, M, nh, hd):
  c = qkv_case(ops, M, nh, hd)
  d = c['d']
  R = qkv_reference(c['x'], c['nw'], c['w'], positions(c['lens0'], c['counts']), c['cos'], c['sin'], nh, hd)
  for tag, control in (('wide', False), ('control', True)):
    q, pool, st = run_qkv(ops, c, control)
    kv = stored_rows(c, pool)
    assert int(st.item()) == 0
    judge(f'S1 {tag} M={M} hd={hd} q', q.cpu(), R['rot'][:, :d], R['rot_allow'][:, :d], PO.BOUNDS)
    judge(f'S1 {tag} M={M} hd={hd} k', kv[:, :d], R['rot'][:, d:], R['rot_allow'][:, d:], PO.BOUNDS)
    judge(f'S1 {tag} M={M} hd={hd} v', kv[:, d:], R['v'], R['v_allow'], PG.BOUNDS)
  (qa, pa, _), (qb, pb, _) = run_qkv(ops, c), run_qkv(ops, c)
  assert biteq(qa, qb) and biteq(pa, pb)  # two runs are bit-equal


def test_wide_qkv_stage_addresses_refusal_and_packing_order(ops):
  lens0, counts = (60, 5, 130, 0), (40, 1, 0, 24)  # across a page edge, inside a page, idle, from nothing: 65 rows
  c = qkv_case(ops, 65, 3, 32, lens0, counts)
  q, pool, st = run_qkv(ops, c)
  t, before = c['table'].cpu(), c['pool']
  touched = torch.zeros(pool.shape[:2], dtype=torch.bool)
  for b, (a, n) in enumerate(zip(lens0, counts)):
    for p in range(a, a + n):
      touched[int(t[b, p // 64]), p % 64] = True
  changed = (bits(pool) != bits(before)).any(-1).cpu()
  assert int(st.item()) == 0 and torch.equal(changed, touched) and torch.isfinite(stored_rows(c, pool).float()).all()  # every other row, NaN fill included, is as it was
  # the reverse packing order: the same bits per row
  order = (3, 2, 1, 0)
  qr, poolr, _ = run_qkv(ops, c, order=order)
  back = torch.cat([qr[sum(counts[o] for o in order[:i]):sum(counts[o] for o in order[:i + 1])] for i in (3, 2, 1, 0)])
  assert biteq(back, q) and biteq(poolr, pool)
  # sequence 1 loses the page its row needs: refused on the device, q row zero, nothing of it stored, the others as before
  c2 = dict(c, table=c['table'].clone())
  c2['table'][1, 0] = -1
  qx, poolx, stx = run_qkv(ops, c2)
  assert int(stx.item()) == 1 and (bits(qx[40]) == 0).all() and biteq(qx[:40], q[:40]) and biteq(qx[41:], q[41:])
  page1 = int(t[1, 0])
  assert biteq(poolx[page1], before[page1]) and biteq(torch.cat([poolx[:page1], poolx[page1 + 1:]]), torch.cat([pool[:page1], pool[page1 + 1:]]))


@pytest.mark.parametrize('M,nh,hd,hidden', SHAPES)
def test_wide_gemm_residual_vs_fp64_reference_and_the_unfused_chain(ops, M, nh, hd, hidden):
  d = nh * hd
  seed = 2000 * M + 10 * nh + hd
  for K in (d, hidden):  # the out projection and fc2
    x0, a, w = rnd(seed + K, M, d), rnd(seed + K + 1, M, K).to(BF16), rnd(seed + K + 2, d, K, scale=K ** -0.5).to(BF16)
    ref, allow = gemm_ref(a, w)
    ag, wg, xg = a.cuda(), w.cuda(), x0.clone().cuda()
    assert ops.wide_gemm_residual(xg, ag, wg).data_ptr() == xg.data_ptr()
    s2_check(f'S2 wide M={M} N={d} K={K}', xg.cpu(), x0, ref, allow)
    s2_check(f'S2 control M={M} N={d} K={K}', (x0.cuda() + ops.gemm_nt(ag, wg).float()).cpu(), x0, ref, allow)
    assert biteq(ops.wide_gemm_residual(x0.clone().cuda(), ag, wg), xg)  # two runs are bit-equal
    if M == 65:  # rows 40 .. 64 launched alone (a 32-row tile) are the same rows of the 65-row launch (64-row tiles)
      assert biteq(ops.wide_gemm_residual(x0[40:].clone().cuda(), ag[40:].contiguous(), wg), xg[40:])


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('M,nh,hd,hidden', SHAPES)
def test_wide_norm_fc1_act_vs_fp64_reference_and_the_unfused_chain(ops, M, nh, hd, hidden, kind):
  d = nh * hd
  seed = 3000 * M + 10 * nh + hd + KINDS.index(kind)
  x, nw = rnd(seed, M, d), 1 + 0.1 * rnd(seed + 1, d)
  w_fc1 = rnd(seed + 2, (2 if kind == 'glu' else 1) * hidden, d, scale=2 * d ** -0.5).to(BF16)
  ref, allow = s3_reference(x, nw, w_fc1, kind)
  xg, nwg, wg = x.cuda(), nw.cuda(), w_fc1.cuda()
  act = ops.wide_norm_fc1_act(xg, nwg, EPS_NORM, wg, kind)
  assert act.dtype == BF16 and tuple(act.shape) == (M, hidden)
  judge(f'S3 wide {kind} M={M} d={d} h={hidden}', act.cpu(), ref, allow, PO.BOUNDS)
  u = ops.gemm_nt(ops.rmsnorm_fwd(xg, nwg, EPS_NORM)[1], wg)
  judge(f'S3 control {kind} M={M} d={d} h={hidden}', (ops.swiglu_fwd(u) if kind == 'glu' else ops.act_fwd(u, kind)).cpu(), ref, allow, PO.BOUNDS)
  assert biteq(ops.wide_norm_fc1_act(xg, nwg, EPS_NORM, wg, kind), act) and biteq(xg.cpu(), x)
  if M == 65:
    assert biteq(ops.wide_norm_fc1_act(xg[40:].contiguous(), nwg, EPS_NORM, wg, kind), act[40:])


@pytest.mark.parametrize('counts', [(4, 1, 0, 2), (40, 1, 0, 24)])  # R = 7 and R = 65
def test_wide_layer_is_its_stages_bits(ops, counts):
  c = qkv_case(ops, sum(counts), 2, 64, (60, 5, 130, 0), counts, seed=1)
  R, d, hidden = sum(counts), c['d'], 256
  g = lambda i, *s: (0.1 * rnd(R + i, *s)).to(BF16).cuda()  # noqa: E731
  mn, w_out, w_fc1, w_fc2 = (1 + 0.1 * rnd(R + 4, d)).cuda(), g(5, d, d), g(6, 2 * hidden, d), g(7, d, hidden)
  x, an, w_qkv, cos, sin = c['x'].cuda(), c['nw'].cuda(), c['w'].cuda(), c['cos'].cuda(), c['sin'].cuda()
  l0, cu, rs, table = i32(c['lens0']), c['cu'].cuda(), c['rs'].cuda(), c['table']
  xs, pool = x.clone(), c['pool'].clone()
  q, status = ops.ragged_norm_qkv_append_paged_wide(xs, an, EPS_NORM, w_qkv, l0, cu, rs, cos, sin, pool, table, 2)
  ops.wide_gemm_residual(xs, ops.attn_ragged_paged(q, pool, table, l0, cu, rs, 2, c['NT']), w_out)
  ops.wide_gemm_residual(xs, ops.wide_norm_fc1_act(xs, mn, EPS_NORM, w_fc1, 'glu'), w_fc2)
  xl, pl = x.clone(), c['pool'].clone()
  ops.ragged_layer_paged_wide(xl, an, mn, EPS_NORM, w_qkv, w_out, w_fc1, w_fc2, l0, cu, rs, cos, sin, pl, table, 2, 'glu', status, c['NT'])
  assert torch.isfinite(xl).all() and biteq(xl, xs) and biteq(pl, pool) and not biteq(xl, x) and int(status.item()) == 0


def test_step_ragged_wide_logits_vs_golden(P, mdl):
  """tests/test_ragged_gpu.py's teacher-forced run under fused='wide': slot 2 joins at step 3 with a 40-row chunk, a 46-row step."""
  m, tok, T = _model(P, mdl), mdl['tokens'], 64
  cache = m.new_cache_paged(3, _scrambled_pool(m, 5, 7), T)
  cache.admit(0)
  cache.admit(1)
  src, fed, rows = (0, 1, 0), [0, 0, 0], [[], [], []]
  for step in range(13):
    if step == 3:
      cache.admit(2)
    counts = [min(5, T - fed[0]), 1, 0 if step < 3 else (40 if step == 3 else 1)]
    x = torch.cat([tok[src[b], fed[b]:fed[b] + c] for b, c in enumerate(counts)]).cuda()
    for b, part in enumerate(m.step_ragged(x, counts, cache, logits=True, all_rows=True, fused='wide').split(counts)):
      rows[b].append(part)
      fed[b] += counts[b]
  cache.check()
  assert cache.lens.tolist() == fed == [64, 13, 49]
  for b in range(3):
    e = TD.relmax(torch.cat(rows[b]).float(), mdl['logits'][src[b], :fed[b]])
    print(f'step_ragged fused=wide: slot {b}: {fed[b]} rows, relmax {e:.2e}')
    assert e < 2e-2, (b, e)


def test_serve_wide_with_chunked_prefill_against_the_full_forward(P, mdl):
  """tests/test_ragged_gpu.py's serve run at prefill_chunk = 48: the 60-token prompt enters as 48 + 12 rows, steps hold up to 50 rows."""
  m, C = _model(P, mdl, seq_len=192), 48
  tok = mdl['tokens'].reshape(-1)
  plen, budget = (5, 60, 17, 33, 9), [70, 12, 40, 8, 20]
  prompts, o = [], 0
  for n in plen:
    prompts.append(tok[o:o + n].cuda())
    o += n
  with torch.no_grad():
    outs = m.serve(prompts, budget, max_batch=2, pool=_scrambled_pool(m, 3, 9), fused='wide', prefill_chunk=C)
    again = m.serve(prompts, budget, max_batch=2, pool=_scrambled_pool(m, 3, 8), fused='wide', prefill_chunk=C)
    for i, (p, t, t2) in enumerate(zip(prompts, outs, again)):
      assert torch.equal(t, t2) and t.numel() == budget[i], i
      seq = torch.cat([p, t])
      full = m(torch.nn.functional.pad(seq, (0, -seq.numel() % 4)).view(1, -1), None).float()[0]
      eps = 2e-2 * full.abs().max().item()
      rows = full[p.numel() - 1:p.numel() - 1 + t.numel()]  # row len(prompt) - 1 + j predicts generated token j
      gap = (rows.max(dim=-1).values - rows.gather(1, t[:, None])[:, 0]).max().item()
      print(f'serve prefill_chunk={C} fused=wide: sequence {i}: {t.numel()} tokens, worst (row max - chosen logit) {gap:.3e} against 4 eps = {4 * eps:.3e}')
      assert gap <= 4 * eps, i  # every generated position, none excluded
