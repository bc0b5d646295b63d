"""The fused extend on a real MI355X: the chunk-rows qkv stage against an fp64 reference that rounds where the
contract rounds, next to the unfused chain (rmsnorm_fwd + gemm_nt + kv_append_rope_rows) as a control under the same assertion; its
contract bits against that control; its bit equality with the decode stage on the same rows; plm_extend_layer_bf16 against the
composition of its own stages; and the cached model, ``extend(fused=True)`` and ``generate_lookup_fused``, under the bounds every cached
path of this project is held to.

The helpers, the allowance algebra and the bounds are those of tests/test_decode_fused_gpu.py (its docstring derives them): the stage's
reference is ``s1_reference``'s arithmetic with the row's position lens0[b] + r where that has pos[b], and ``stage_check`` asserts what
``s1_check`` asserts - parity_ops.BOUNDS on what passed RoPE (q, k), parity_gemm.BOUNDS on the bare GEMM output (v: 1 ulp beyond the
allowance, at most 2e-2 of the elements off the correctly rounded value).  Nothing here is fitted to an output."""

import functools
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
import test_decode_fused_gpu as DF  # noqa: E402
from test_decode_fused_gpu import BF16, EPS_NORM, I32, P, biteq, bits, mdl, ops, relmax, rnd  # noqa: E402,F401  (P, ops, mdl: fixtures)

TMAX = 24
HIDDEN = DF.HIDDEN
KINDS = DF.KINDS
# 16 and 17 rows on either side of the one- / two-MFMA body switch, 32 rows as the limit
CHUNKS = ((1, 1), (1, 5), (5, 3), (2, 8), (17, 1), (3, 7), (4, 8), (1, 32))
WIDE = 40  # a second cache length for the one chunk of 32 rows: no cache of 24 rows holds it, there its every full chunk is REFUSED
# (B, n, nh, hd, Tmax): every chunk shape on every head shape at Tmax = 24; d = 768 (a K loop of several chunks) at 15 rows and at 21;
# the 32-row chunk again where it fits
SHAPES = [(B, n, nh, hd, TMAX) for B, n in CHUNKS for nh, hd in DF.HEADS] + [(5, 3, 12, 64, TMAX), (3, 7, 12, 64, TMAX)] + \
    [(1, 32, nh, hd, WIDE) for nh, hd in DF.HEADS]
SHAPES_THAT_FIT = [s for s in SHAPES if s[1] <= s[4]]


# ---- the inputs and the reference of a shape, made once ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_inputs(B, n, nh, hd, T=TMAX):
  d, M = nh * hd, B * n
  seed = 5000 * M + 100 * n + 10 * nh + hd
  x, nw = rnd(seed, M, d), 1 + 0.1 * rnd(seed + 1, d)
  w_qkv = rnd(seed + 2, 3 * d, d, scale=d ** -0.5).to(BF16)
  cos, sin = O.rope_table(hd, T)
  kv0 = torch.randn(B, T, 2 * d + 8, generator=torch.Generator().manual_seed(seed + 3)).to(BF16)  # padded row stride
  return dict(x=x, nw=nw, w_qkv=w_qkv, cos=cos, sin=sin, kv0=kv0, g=dict(x=x.cuda(), nw=nw.cuda(), w=w_qkv.cuda(), cos=cos.cuda(), sin=sin.cuda()))


@functools.lru_cache(maxsize=None)
def stage_projection(B, n, nh, hd, T=TMAX):
  """s1_reference's first half, which no position enters: the fp64 un-rounded qkv of the correctly rounded norm output, its allowance,
  the flip allowance of its bf16 rounding and that rounding."""
  I = stage_inputs(B, n, nh, hd, T)
  n_b, e_n = DF.norm_ref(I['x'], I['nw'])
  ref, allow = DF.gemm_ref(n_b, I['w_qkv'], e_n)
  return dict(ref=ref, allow=allow, e_qkv=DF.flip(ref, allow), qkv_b=PO.bf16_rne(ref).to(BF16))


def stage_reference(B, n, nh, hd, pos, T=TMAX):
  """s1_reference's second half at one position per ROW (pos[b * n + r] = lens0[b] + r; clamped for the rows that are not stored and not
  judged)."""
  I, R = stage_inputs(B, n, nh, hd, T), stage_projection(B, n, nh, hd, T)
  d, M = nh * hd, B * n
  tp = torch.tensor(pos).clamp(0, T - 1)
  cos, sin = I['cos'], I['sin']
  rot, rallow = PO.rope_reference(R['qkv_b'], cos[tp], sin[tp], 1, M, nh)
  ea, eb = R['e_qkv'][:, :2 * d].reshape(M, 2 * nh, hd // 2, 2).unbind(-1)
  c, s = cos[tp].double().abs().reshape(M, 1, hd // 2), sin[tp].double().abs().reshape(M, 1, hd // 2)
  rallow = rallow + torch.stack([ea * c + eb * s, eb * c + ea * s], -1).reshape(M, 2 * d)
  return dict(rot=rot, rot_allow=rallow, v=R['ref'][:, 2 * d:], v_allow=R['allow'][:, 2 * d:])


def counts_of(B, n, n_new):
  return [n] * B if n_new is None else [min(max(int(c), 0), n) for c in n_new]


def refused_of(lens0, counts, lim):
  return [l0 < 0 or l0 + c > lim for l0, c in zip(lens0, counts)]


def stored_rows(B, n, lens0, counts, lim):
  """[(row b * n + r, b, cache row lens0[b] + r)] of every chunk row that is appended."""
  ref = refused_of(lens0, counts, lim)
  return [(b * n + r, b, lens0[b] + r) for b in range(B) if not ref[b] for r in range(counts[b])]


def stage_check(tag, R, q, kv, status, kv0, B, n, lens0, counts, d, lim=TMAX):
  """s1_check for chunk rows."""
  rows = stored_rows(B, n, lens0, counts, lim)
  want_kv = kv0.clone()
  if rows:
    ms = [m for m, _, _ in rows]
    k_got = torch.stack([kv[b, t, :d] for _, b, t in rows])
    v_got = torch.stack([kv[b, t, d:2 * d] for _, b, t in rows])
    DF.judge(tag + ' q', q[ms], R['rot'][ms, :d], R['rot_allow'][ms, :d], PO.BOUNDS)
    DF.judge(tag + ' k', k_got, R['rot'][ms, d:], R['rot_allow'][ms, d:], PO.BOUNDS)
    DF.judge(tag + ' v', v_got, R['v'][ms], R['v_allow'][ms], PG.BOUNDS)
    for _, b, t in rows:
      want_kv[b, t] = kv[b, t]
  assert biteq(kv, want_kv), tag  # no other cache row changed: padding rows, a refused sequence's rows and the pad columns included
  kept = {m for m, _, _ in rows}
  for m in range(B * n):
    if m not in kept:
      assert (bits(q[m]) == 0).all(), (tag, m)  # the zero q row of a padding row or of a refused sequence
  assert int(status.item()) == (1 if any(refused_of(lens0, counts, lim)) else 0), tag


def variants(B, n, T):
  """(tag, n_new or None, lens0): full chunks and ragged ones whose n_new holds 0, 1 and n (over the variants where B < 3), every one at
  lens0 = 0 and at lens0 = Tmax - c_b, the last row that fits, for some sequence.  Where c_b <= Tmax every chunk fits."""
  out = []
  for tag, n_new, shift in (('full-a', None, 0), ('full-b', None, 1), ('ragged-a', (n, 0, 1), 0), ('ragged-b', (1, n, 0), 1), ('ragged-c', (0, 1, n), 0)):
    cnt = [n] * B if n_new is None else [(n_new + (max(n - 1, 0), n // 2))[b % 5] for b in range(B)]
    room = [max(T - c, 0) for c in cnt]
    lens0 = [(0, room[b], min(3, room[b]), (5 * b) % (room[b] + 1))[(b + shift) % 4] for b in range(B)]
    out.append((tag, None if n_new is None else cnt, lens0))
  return out


def launch_stage(ops, I, B, n, nh, n_new, lens0, kv, cos=None, sin=None):
  g, d = I['g'], I['x'].shape[1]
  nn = None if n_new is None else torch.tensor(n_new, dtype=I32).cuda()
  return ops.extend_norm_qkv_append(g['x'], g['nw'], EPS_NORM, g['w'], torch.tensor(lens0, dtype=I32).cuda(), g['cos'] if cos is None else cos,
                                    g['sin'] if sin is None else sin, kv[:, :, :2 * d], nh, n_new=nn)


def launch_control(ops, I, B, n, nh, n_new, lens0, kv, cos=None, sin=None):
  """rmsnorm_fwd -> gemm_nt -> kv_append_rope_rows: what ``extend`` runs by default."""
  g, d = I['g'], I['x'].shape[1]
  nn = None if n_new is None else torch.tensor(n_new, dtype=I32).cuda()
  qc = torch.full((B * n, d), float('nan'), dtype=BF16, device='cuda')
  _, n1, _ = ops.rmsnorm_fwd(g['x'], g['nw'], EPS_NORM)
  _, st = ops.kv_append_rope_rows(ops.gemm_nt(n1, g['w']), torch.tensor(lens0, dtype=I32).cuda(), g['cos'] if cos is None else cos,
                                  g['sin'] if sin is None else sin, kv[:, :, :2 * d], nh, n_new=nn, q_out=qc)
  return qc, st


# ---- 1. the stage against fp64 and against the control -----------------------------------------------------------------------------------
@pytest.mark.parametrize('B,n,nh,hd,T', SHAPES)
def test_extend_norm_qkv_append_vs_fp64_reference_and_the_unfused_chain(ops, B, n, nh, hd, T):
  d = nh * hd
  I = stage_inputs(B, n, nh, hd, T)
  seen = set()
  for tag, n_new, lens0 in variants(B, n, T):
    counts = counts_of(B, n, n_new)
    assert refused_of(lens0, counts, T) == [c > T for c in counts]  # only a chunk longer than the cache is refused (stage_check: its contract)
    seen |= set(counts) if n_new is not None else set()
    R = stage_reference(B, n, nh, hd, [lens0[b] + r for b in range(B) for r in range(n)], T)
    kv0 = I['kv0'].cuda()
    kv = kv0.clone()
    q, status = launch_stage(ops, I, B, n, nh, n_new, lens0, kv)
    assert q.dtype == BF16 and tuple(q.shape) == (B * n, d)
    stage_check(f'S1r fused {tag} B={B} n={n} nh={nh} hd={hd} Tmax={T}', R, q.cpu(), kv.cpu(), status, I['kv0'], B, n, lens0, counts, d, T)
    assert biteq(I['g']['x'].cpu(), I['x'])  # x is read-only in the stage
    kvc = kv0.clone()
    qc, stc = launch_control(ops, I, B, n, nh, n_new, lens0, kvc)
    stage_check(f'S1r control {tag} B={B} n={n} nh={nh} hd={hd} Tmax={T}', R, qc.cpu(), kvc.cpu(), stc, I['kv0'], B, n, lens0, counts, d, T)
    assert torch.equal(status, stc)
    kv2 = kv0.clone()  # two runs are bit-equal
    q2, _ = launch_stage(ops, I, B, n, nh, n_new, lens0, kv2)
    assert biteq(q2, q) and biteq(kv2, kv), tag
  assert {0, 1, n} <= seen  # the ragged variants held all three


# ---- 2. the contract bits ---------------------------------------------------------------------------------------------------------------------
NAN_PATTERN = 0x7FC1  # a quiet bf16 NaN no kernel produces: an appended row no longer holds it, every other row must


@pytest.mark.parametrize('rope_rows', [TMAX, TMAX - 2])  # lim = min(Tmax, rope_T) is the cache's limit, then the table's
@pytest.mark.parametrize('B,n,nh,hd', [(5, 3, 3, 32), (5, 6, 2, 64), (17, 1, 1, 128)])
def test_refusals_padding_rows_and_untouched_cache_rows_are_the_control_s_bits(ops, B, n, nh, hd, rope_rows):
  d, lim = nh * hd, rope_rows
  I = stage_inputs(B, n, nh, hd)
  cos, sin = I['g']['cos'][:rope_rows].contiguous(), I['g']['sin'][:rope_rows].contiguous()
  # sequence 1 is one row too long, sequence 3 starts before the cache; both among healthy ones.  n_new on the device: above n (clamped
  # to n), negative (clamped to 0), and ragged
  n_new = [(n + 5, n, -3, 1, max(n - 1, 0))[b % 5] for b in range(B)]
  counts = counts_of(B, n, n_new)
  lens0 = [(0, lim + 1 - counts[1], 3, -1, lim - counts[4])[b % 5] if b < 5 else (2 * b) % (lim - n) for b in range(B)]
  want_refused = [b in (1, 3) for b in range(B)]
  assert refused_of(lens0, counts, lim) == want_refused and lens0[1] + counts[1] == lim + 1
  kv0 = torch.full((B, TMAX, 2 * d + 8), 0, dtype=torch.int16).fill_(NAN_PATTERN).view(BF16).cuda()
  kv, kvc = kv0.clone(), kv0.clone()
  q, st = launch_stage(ops, I, B, n, nh, n_new, lens0, kv, cos, sin)
  qc, stc = launch_control(ops, I, B, n, nh, n_new, lens0, kvc, cos, sin)
  assert int(st.item()) == 1 and torch.equal(st, stc)
  rows = stored_rows(B, n, lens0, counts, lim)
  kept = {m for m, _, _ in rows}
  for m in range(B * n):
    if m not in kept:  # padding rows and the refused sequences' rows: zeros, the control's bits
      assert (bits(q[m]) == 0).all() and biteq(q[m], qc[m]), m
  appended = torch.zeros(B, TMAX, dtype=torch.bool)
  for _, b, t in rows:
    appended[b, t] = True
  pattern = bits(kv0.cpu())
  for name, got in (('fused', bits(kv.cpu())), ('control', bits(kvc.cpu()))):
    changed = (got != pattern).any(dim=-1)
    assert torch.equal(changed, appended), (name, changed.nonzero().tolist())  # exactly the appended rows left the pattern: the clamp of n_new too
    assert (got[:, :, 2 * d:] == pattern[:, :, 2 * d:]).all(), name  # the pad columns of every row
  assert biteq(kv.cpu()[~appended], kvc.cpu()[~appended])
  assert not torch.isnan(q.float()).any() and not torch.isnan(kv.cpu()[appended][:, :2 * d].float()).any()
  # a healthy batch leaves the status word alone
  ok0 = [min(max(l0, 0), lim - c) for l0, c in zip(lens0, counts)]
  _, st_ok = launch_stage(ops, I, B, n, nh, n_new, ok0, kv0.clone(), cos, sin)
  assert int(st_ok.item()) == 0


# ---- 3. same core, same bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,n,nh,hd,T', SHAPES_THAT_FIT)
def test_full_chunks_are_the_decode_stage_s_bits_on_the_same_rows(ops, B, n, nh, hd, T):
  """The rows variant may differ from the decode stage only in where a row goes: plm_decode_norm_qkv_append_bf16 on the same M = B * n
  rows, each a sequence of its own at pos[m] = lens0[b] + r in a scratch cache, gives the same q rows and the same k | v rows."""
  d, M = nh * hd, B * n
  I = stage_inputs(B, n, nh, hd, T)
  g = I['g']
  lens0 = [(0, T - n, 3, (5 * b) % (T - n + 1))[b % 4] for b in range(B)]
  pos = [lens0[b] + r for b in range(B) for r in range(n)]
  kv = I['kv0'].cuda()
  q, st = launch_stage(ops, I, B, n, nh, None, lens0, kv)
  scratch = torch.zeros(M, T, 2 * d, dtype=BF16, device='cuda')
  qd, std = ops.decode_norm_qkv_append(g['x'], g['nw'], EPS_NORM, g['w'], torch.tensor(pos, dtype=I32).cuda(), g['cos'], g['sin'], scratch, nh)
  assert int(st.item()) == 0 == int(std.item())
  assert biteq(q, qd)
  got = torch.stack([kv[b, lens0[b] + r, :2 * d] for b in range(B) for r in range(n)])
  want = torch.stack([scratch[m, pos[m]] for m in range(M)])
  assert biteq(got, want) and bool((bits(want) != 0).any())


# ---- 4. the layer driver adds nothing ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('B,n,nh,hd', [(5, 3, 3, 32), (17, 1, 2, 64), (4, 8, 1, 128)])
def test_extend_layer_is_the_composition_of_its_stages(ops, B, n, nh, hd, kind):
  d, hidden, M = nh * hd, HIDDEN, B * n
  seed = 6000 * M + hd + KINDS.index(kind)
  x0 = rnd(seed, M, d).cuda()
  an, mn = (1 + 0.1 * rnd(seed + 1, d)).cuda(), (1 + 0.1 * rnd(seed + 2, d)).cuda()
  w_qkv = rnd(seed + 3, 3 * d, d, scale=d ** -0.5).to(BF16).cuda()
  w_out = rnd(seed + 4, d, d, scale=d ** -0.5).to(BF16).cuda()
  w_fc1 = rnd(seed + 5, (2 if kind == 'glu' else 1) * hidden, d, scale=d ** -0.5).to(BF16).cuda()
  w_fc2 = rnd(seed + 6, d, hidden, scale=hidden ** -0.5).to(BF16).cuda()
  cos, sin = (t.cuda() for t in O.rope_table(hd, TMAX))
  kv0 = torch.randn(B, TMAX, 2 * d + 8, generator=torch.Generator().manual_seed(seed + 7)).to(BF16).cuda()
  full = [(0, TMAX - n, 3, (5 * b) % (TMAX - n + 1))[b % 4] for b in range(B)]
  ragged = [(n, 0, 1, max(n - 1, 0))[b % 4] for b in range(B)]
  over = list(full)
  over[min(2, B - 1)] = TMAX + 1 - n  # one sequence does not fit: refused, the others unaffected
  for tag, lens0, n_new in (('full', full, None), ('ragged', [min(l, TMAX - n) for l in full], ragged), ('one-refused', over, None)):
    l0 = torch.tensor(lens0, dtype=I32).cuda()
    nn = None if n_new is None else torch.tensor(n_new, dtype=I32).cuda()
    for splits in (0, 3):
      x1, kv1, st1 = x0.clone(), kv0.clone(), torch.zeros(1, dtype=I32, device='cuda')
      q, _ = ops.extend_norm_qkv_append(x1, an, EPS_NORM, w_qkv, l0, cos, sin, kv1[:, :, :2 * d], nh, n_new=nn, status=st1)
      ops.decode_gemm_residual(x1, ops.attn_extend(q, kv1[:, :, :2 * d], l0, nh, n_new=nn, splits=splits), w_out)
      ops.decode_gemm_residual(x1, ops.decode_norm_fc1_act(x1, mn, EPS_NORM, w_fc1, kind), w_fc2)
      x2, kv2, st2 = x0.clone(), kv0.clone(), torch.zeros(1, dtype=I32, device='cuda')
      out = ops.extend_layer(x2, an, mn, EPS_NORM, w_qkv, w_out, w_fc1, w_fc2, l0, nn, cos, sin, kv2[:, :, :2 * d], nh, kind, st2, splits=splits)
      assert out.data_ptr() == x2.data_ptr()
      assert biteq(x2, x1) and biteq(kv2, kv1) and torch.equal(st2, st1), (tag, splits, kind)
      assert torch.isfinite(x2).all() and not biteq(x2, x0) and int(st2.item()) == (1 if tag == 'one-refused' else 0)
      ws = ops.extend_layer_workspace(B, n, nh, hd, hidden, TMAX, splits, 'cuda')  # a caller-owned workspace; a second run: the same bits
      x3, kv3, st3 = x0.clone(), kv0.clone(), torch.zeros(1, dtype=I32, device='cuda')
      ops.extend_layer(x3, an, mn, EPS_NORM, w_qkv, w_out, w_fc1, w_fc2, l0, nn, cos, sin, kv3[:, :, :2 * d], nh, kind, st3, splits=splits, workspace=ws)
      assert biteq(x3, x1) and biteq(kv3, kv1) and torch.equal(st3, st1)


def test_ops_refuse_what_the_kernels_do_not_serve(ops):
  d, nh = 128, 2
  w = torch.zeros(3 * d, d, dtype=BF16, device='cuda')
  nw = torch.ones(d, device='cuda')
  cos, sin = (t.cuda() for t in O.rope_table(64, TMAX))
  with pytest.raises(ValueError, match='33 rows'):
    ops.extend_norm_qkv_append(torch.zeros(33, d, device='cuda'), nw, 1e-6, w, torch.zeros(3, dtype=I32, device='cuda'), cos, sin,
                               torch.zeros(3, TMAX, 2 * d, dtype=BF16, device='cuda'), nh)
  with pytest.raises(ValueError, match='do not fit'):  # 10 rows are no whole chunks of 3 sequences
    ops.extend_norm_qkv_append(torch.zeros(10, d, device='cuda'), nw, 1e-6, w, torch.zeros(3, dtype=I32, device='cuda'), cos, sin,
                               torch.zeros(3, TMAX, 2 * d, dtype=BF16, device='cuda'), nh)
  with pytest.raises(ValueError, match='unsupported shape'):
    ops.extend_layer_workspace(4, 9, nh, 64, 512, TMAX, 0, 'cuda')


# ---- 5. the model, teacher-forced ---------------------------------------------------------------------------------------------------------
WIDTHS = (1, 3, 8, 4)


def _chunked(m, tok, plan, T0=16, device_lens=False):
  """Prefill tok[:, :T0], then append every sequence's own true continuation in chunks of WIDTHS with extend(fused=True, logits=True,
  all_rows=True).  plan[i][b] = the rows sequence b appends of chunk i (None: the full width).  Returns per sequence the list of
  (position, logits row) of every appended token, and the cache."""
  B = tok.shape[0]
  cache, _ = m.prefill(tok[:, :T0].cuda(), logits=True)
  at = [T0] * B
  got = [[] for _ in range(B)]
  for w, cs in zip(WIDTHS, plan):
    cs = [w] * B if cs is None else cs
    chunk = torch.full((B, w), 7, dtype=torch.int64)  # padding: must not matter
    for b in range(B):
      chunk[b, :cs[b]] = tok[b, at[b]:at[b] + cs[b]]
    lens = None if all(c == w for c in cs) and not device_lens else (torch.tensor(cs, dtype=I32).cuda() if device_lens else cs)
    out = m.extend(chunk.cuda(), cache, token_lens=lens, logits=True, all_rows=True, fused=True)
    assert out.dtype == BF16 and tuple(out.shape) == (B, w, m.cfg.vocab_size)
    for b in range(B):
      got[b] += [(at[b] + r, out[b, r]) for r in range(cs[b])]
      at[b] += cs[b]
  cache.check()
  assert cache.lens.tolist() == at
  return got, cache


def _worst(got, ref):
  """relmax of every sequence's appended rows against rows of the reference logits [B, T, V] at the same positions."""
  worst = 0.0
  for b, rows in enumerate(got):
    pos = [p for p, _ in rows]
    worst = max(worst, relmax(torch.stack([r for _, r in rows]).float(), ref[b, pos]))
  return worst


def test_fused_extend_logits_vs_golden(P, mdl):
  m = DF._small(P, mdl)
  got, cache = _chunked(m, mdl['tokens'], (None,) * 4)
  assert cache.lens.tolist() == [32, 32] and [p for p, _ in got[0]] == list(range(16, 32))
  e = _worst(got, mdl['logits'])
  print(f'fused extend, chunks of {WIDTHS}, logits vs golden at positions 16..31: relmax {e:.2e}')
  assert e < 2e-2


@pytest.mark.parametrize('device_lens', [False, True])
def test_fused_extend_logits_with_ragged_token_lens(P, mdl, device_lens):
  m = DF._small(P, mdl)
  plan = ((1, 0), (3, 1), (5, 8), (0, 4))  # 0, 1, the full width and something between, on either sequence
  got, cache = _chunked(m, mdl['tokens'], plan, device_lens=device_lens)
  assert cache.lens.tolist() == [25, 29]
  e = _worst(got, mdl['logits'])
  print(f'fused extend, ragged token_lens on the {"device" if device_lens else "host"}: relmax {e:.2e}')
  assert e < 2e-2


@pytest.mark.parametrize('mlp,nh', [('mlp', 2), ('mlp_relu_sq', 2), ('glu', 4), ('glu', 1)])
def test_fused_extend_logits_other_mlp_classes_and_head_dims_vs_oracle(P, mlp, nh):
  ocfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=nh, mlp=mlp)
  w = O.init_params(ocfg, seed=31 + nh)
  tok = torch.from_numpy(np.random.default_rng(nh).integers(0, 256, size=(2, 64)))
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=nh, mlp=mlp))
  m.load_state_dict(w)
  m = m.cuda()
  got, _ = _chunked(m, tok, (None, (3, 2), None, (4, 4)))
  with torch.no_grad():
    ref = O.forward(w, ocfg, tok)
  e = _worst(got, ref)
  print(f'fused extend logits mlp={mlp} head_dim={128 // nh} vs fp32 oracle: relmax {e:.2e}')
  assert e < 2e-2


# ---- 6. library calls ---------------------------------------------------------------------------------------------------------------------------
FUSED_EXTEND_CALLS = ['plm_embed_fwd', 'plm_extend_layer_bf16', 'plm_extend_layer_bf16', 'plm_rmsnorm_fwd', 'plm_head_predict_bf16']
# what the default extend issued before the fused path existed (two layers, a GLU MLP), recorded on the parent commit
DEFAULT_EXTEND_CALLS = [
  'plm_embed_fwd',
  'plm_rmsnorm_fwd', 'plm_gemm_bf16_nt', 'plm_kv_append_rope_rows', 'plm_attn_extend', 'plm_gemm_bf16_nt', 'plm_rmsnorm_fwd', 'plm_gemm_bf16_nt',
  'plm_swiglu_fwd', 'plm_gemm_bf16_nt',
  'plm_rmsnorm_fwd', 'plm_gemm_bf16_nt', 'plm_kv_append_rope_rows', 'plm_attn_extend', 'plm_gemm_bf16_nt', 'plm_rmsnorm_fwd', 'plm_gemm_bf16_nt',
  'plm_swiglu_fwd', 'plm_gemm_bf16_nt',
  'plm_rmsnorm_fwd', 'plm_head_predict_bf16']


def test_fused_extend_issues_one_library_call_per_layer_and_the_default_is_unchanged(P, mdl, monkeypatch):
  from plainlm_amd import _lib
  m = DF._small(P, mdl)
  tok = mdl['tokens'].cuda()
  cache, _ = m.prefill(tok[:, :16])
  calls = []
  real = _lib.check
  monkeypatch.setattr(_lib, 'check', lambda rc, what: calls.append(what) or real(rc, what))
  m.extend(tok[:, 16:19], cache, fused=True)
  assert calls == FUSED_EXTEND_CALLS, calls
  del calls[:]
  m.extend(tok[:, 19:24], cache, token_lens=[5, 2], fused=True)
  assert calls == FUSED_EXTEND_CALLS, calls
  del calls[:]
  m.extend(tok[:, 24:27], cache)  # fused=False, the default: the parent's list
  assert calls == DEFAULT_EXTEND_CALLS, calls
  monkeypatch.undo()
  cache.check()
  assert cache.lens.tolist() == [27, 24]


# ---- 7. generate_lookup_fused ---------------------------------------------------------------------------------------------------------------------
def _lookup_prompt(mdl):
  """A periodic prompt (period 4, from the golden tokens): with ngram = (1, 4) its own text is full of earlier occurrences to draft from."""
  return mdl['tokens'][:, :4].repeat(1, 4).cuda()


def test_generate_lookup_fused_greedy_against_the_full_forward(P, mdl):
  """test_generate_fused_greedy_against_the_full_forward's method on generate_lookup_fused: every generated position, none excluded."""
  m = DF._small(P, mdl)
  prompt = _lookup_prompt(mdl)
  N, k = 32, 7
  with torch.no_grad():
    toks, lps, stats = m.generate_lookup_fused(prompt, N, n_draft=k, ngram=(1, 4), return_logprobs=True, return_stats=True)
    assert toks.dtype == torch.int64 and tuple(toks.shape) == (2, N) and lps.dtype == torch.float32 and tuple(lps.shape) == (2, N)
    print(f'generate_lookup_fused: rounds {stats["rounds"]}, drafted {stats["drafted"].tolist()}, accepted {stats["accepted"].tolist()}')
    assert int(stats['drafted'].sum()) > 0  # a run that never proposed anything would exercise only n_prop = 0 chunks
    seq = torch.cat([prompt, toks], dim=1)
    full = m(seq, None).float()  # row 15 + i predicts generated token i
    eps = 2e-2 * full.abs().max().item()
    rows = full[:, 15:15 + N]
    chosen = rows.gather(2, toks[:, :, None])[:, :, 0]
    gap = (rows.max(dim=-1).values - chosen).max().item()
    share = (rows.argmax(-1) == toks).float().mean().item()
    print(f'generate_lookup_fused vs full forward: worst (row max - chosen logit) {gap:.3e} against 4 eps = {4 * eps:.3e}; exact matches with '
          f'the recompute argmax {share:.4f}')
    assert gap <= 4 * eps
    tg = torch.full_like(seq, -100)
    tg[:, 15:15 + N] = toks
    want = -m.predict(seq, targets=tg).nll[:, 15:15 + N]
    assert (lps - want).abs().max().item() <= eps, ((lps - want).abs().max().item(), eps)
    assert (lps <= 0).all()
    t2, l2, s2 = m.generate_lookup_fused(prompt, N, n_draft=k, ngram=(1, 4), return_logprobs=True, return_stats=True)  # two runs are bit-equal
    assert torch.equal(t2, toks) and torch.equal(l2, lps) and s2['rounds'] == stats['rounds']
    assert torch.equal(s2['drafted'], stats['drafted']) and torch.equal(s2['accepted'], stats['accepted'])
    assert torch.equal(m.generate_lookup_fused(prompt, N, n_draft=k), toks)


def test_generate_lookup_fused_sampled_is_bit_reproducible_under_a_seed(P, mdl):
  m = DF._small(P, mdl)
  prompt = _lookup_prompt(mdl)
  kw = dict(n_draft=7, ngram=(1, 4), temperature=0.8, top_k=20, top_p=0.9, seed=1234, return_logprobs=True, return_stats=True)
  with torch.no_grad():
    t1, l1, s1 = m.generate_lookup_fused(prompt, 24, **kw)
    t2, l2, s2 = m.generate_lookup_fused(prompt, 24, **kw)
  assert tuple(t1.shape) == (2, 24) and bool(((t1 >= 0) & (t1 < 256)).all()) and torch.isfinite(l1).all() and (l1 <= 0).all()
  assert torch.equal(t1, t2) and torch.equal(l1, l2) and s1['rounds'] == s2['rounds'] and torch.equal(s1['drafted'], s2['drafted'])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_fused_extend_refuses_more_than_32_chunk_rows(P, mdl):
  m = DF._small(P, mdl)
  for B, n in ((33, 1), (4, 9), (1, 33)):
    cache = m.new_cache(B)
    with pytest.raises(ValueError, match='leave fused off$'):
      m.extend(torch.zeros(B, n, dtype=torch.int64, device='cuda'), cache, fused=True)
    assert cache.lens.tolist() == [0] * B  # refused before anything moved
    cache.check()
  cache = m.new_cache(4)
  r = m.extend(torch.zeros(4, 8, dtype=torch.int64, device='cuda'), cache, fused=True)  # 32 rows are served
  assert tuple(r.tokens.shape) == (4,) and cache.lens.tolist() == [8] * 4
  cache.check()
  prompt = torch.zeros(4, 16, dtype=torch.int64, device='cuda')
  with torch.no_grad(), pytest.raises(ValueError, match='leave fused off$'):
    m.generate_lookup_fused(prompt, 4, n_draft=8)  # 4 x 9 rows
  with torch.no_grad():
    assert tuple(m.generate_lookup_fused(prompt, 4, n_draft=7).shape) == (4, 4)  # 4 x 8 rows
