"""The attention error budget (oracle/parity.py) against planted defects, on the CPU.

The stand-in kernel is the bf16-emulating attention of oracle/cpu_ref_bf16.py: it rounds where the HIP kernels round, so
it is what an honest kernel looks like under the budget.  Each defect below is a small edit of that stand-in, in Python,
of the kind a rewrite of the masking, scaling or row/tile bookkeeping of the attention kernels tends to introduce.  The
budget must ACCEPT the honest stand-in at the shapes the GPU tests use, and REJECT every defect - most of which pass
the older rel-to-max tolerances (1.6e-2 out, 2e-2 gradients).  Nothing here launches a kernel.

The second half calibrates the input classes of parity.attn_inputs (peaked, ramp, sink, spike): the stand-in, a tiled deferred-max
forward and a split-KV forward written step by step are within budget on every class, and one-line defects of those steps that
unit-normal data cannot see (the rescale of the running sums only ever ran on zeros there) are rejected on a class."""

import math

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O
from oracle import cpu_ref_bf16 as E
from oracle import parity as P

BF16 = torch.bfloat16


def _random_docs(B, T, seed, mean=None):
  """docs_lengths per row summing to T + 1: uniform lengths below T / 3 (tests/test_kernels_gpu.py), or geometric ones of ``mean``."""
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(B):
    lens, tot = [], 0
    while tot < T + 1:
      n = int(rng.geometric(1.0 / mean)) if mean else int(rng.integers(1, max(2, T // 3)))
      n = min(n, T + 1 - tot)
      lens.append(n)
      tot += n
    out.append(lens)
  return out


def _inputs(B, T, nh, hd, seed):
  g = torch.Generator().manual_seed(seed)
  d = nh * hd
  return torch.randn(B * T, 3 * d, generator=g).to(BF16), torch.randn(B * T, d, generator=g).to(BF16)


def _bwd(q, k, v, o, do, lse2, allow, rb, scale_mul=1.0, delta_edit=None, dv_drop_row=None, dk_drop=None):
  """cpu_ref_bf16._attn_bwd with the hooks the defects need (test_bwd_copy_is_the_stand_in pins the hook-free path to it)."""
  hd = q.shape[-1]
  scale = scale_mul / math.sqrt(hd)
  c2 = scale * E.LOG2E
  delta = (do * o).sum(-1, keepdim=True)
  if delta_edit is not None:
    delta = delta_edit(delta.clone())
  s = torch.matmul(q, k.transpose(-1, -2))
  p = torch.exp2(s * c2 - lse2).masked_fill(~allow, 0.0)
  dp = torch.matmul(do, v.transpose(-1, -2))
  ds = rb(p * (dp - delta))
  pv = rb(p)
  if dv_drop_row is not None:
    pv = pv.clone()
    pv[..., dv_drop_row, :] = 0.0
  dv = torch.matmul(pv.transpose(-1, -2), do)
  dq = torch.matmul(ds, k) * scale
  dsk = ds
  if dk_drop is not None:
    (q0, q1), (k0, k1) = dk_drop
    dsk = ds.clone()
    dsk[..., q0:q1, k0:k1] = 0.0
  dk = torch.matmul(dsk.transpose(-1, -2), q) * scale
  return dq, dk, dv, delta.squeeze(-1)


def _standin(qkv, dout, B, T, nh, hd, ds=None, defect=None, at=None):
  """parity.standin's steps with one defect planted: returns what a kernel would (qkv_rot, out, lse, dqkv, delta)."""
  rb = E._Round(True)
  cos, sin = O.rope_table(hd, T)
  d = nh * hd
  q, k, v = (t.float().reshape(B, T, nh, hd) for t in qkv.split(d, dim=1))
  qr, kr = E._rope(q, cos, sin, 1.0, rb), E._rope(k, cos, sin, 1.0, rb)
  qkv_rot = torch.cat([qr.reshape(B * T, d), kr.reshape(B * T, d), v.reshape(B * T, d)], dim=1).to(BF16)
  qh, kh, vh = (t.transpose(1, 2) for t in (qr, kr, v))
  if defect in ('doc_start_minus_1', 'doc_start_plus_1'):  # one row's doc_start read off by one (fwd and bwd share the mask)
    ds = ds.clone()
    ds[0, at] += -1 if defect == 'doc_start_minus_1' else 1
  allow = P.allow_mask(B, T, ds).expand(B, 1, T, T).clone()
  if defect == 'drop_diagonal':  # one query row misses its own key
    allow[:, :, at, at] = False
  allow_fwd = allow
  if defect == 'skip_key_tile':  # the forward skips one 64-key tile for one 32-row wave block
    (r0, c0) = at
    allow_fwd = allow.clone()
    allow_fwd[:, :, r0:r0 + 32, c0:c0 + 64] = False
  qf = qh * 1.01 if defect == 'scale' else qh  # softmax scale 1 % too large (forward; the backward below likewise)
  o, lse2 = E._attn_fwd(qf, kh, vh, allow_fwd, rb)
  if defect == 'lse_shift':
    lse2 = lse2 + math.log2(1.0 + 2.0 ** -8)
  do = dout.float().reshape(B, T, nh, hd).transpose(1, 2)
  kw = {}
  if defect == 'scale':
    kw['scale_mul'] = 1.01
  elif defect == 'delta_zero':
    kw['delta_edit'] = lambda dl: dl.index_fill_(2, torch.tensor([at]), 0.0)
  elif defect == 'delta_scale':
    kw['delta_edit'] = lambda dl: torch.cat([dl[:, :, :at], dl[:, :, at:at + 1] * 1.01, dl[:, :, at + 1:]], dim=2)
  elif defect == 'dv_last_row':
    kw['dv_drop_row'] = T - 1
  elif defect == 'dk_tile':
    kw['dk_drop'] = at
  dq, dk, dv, delta = _bwd(qh, kh, vh, o, do, lse2, allow, rb, **kw)
  dq, dk = (t.transpose(1, 2) for t in (dq, dk))  # [B, T, nh, hd], w.r.t. the rotated q, k
  if defect == 'rope_neighbour':  # the inverse rotation of one row uses the next position's angles
    c2, s2 = cos.clone(), sin.clone()
    c2[at], s2[at] = cos[at + 1], sin[at + 1]
    dq, dk = E._rope(dq, c2, s2, -1.0, rb), E._rope(dk, c2, s2, -1.0, rb)
  else:
    dq, dk = E._rope(dq, cos, sin, -1.0, rb), E._rope(dk, cos, sin, -1.0, rb)
  dqkv = torch.cat([dq.reshape(B * T, d), dk.reshape(B * T, d), rb(dv.transpose(1, 2)).reshape(B * T, d)], dim=1)
  return qkv_rot, o.transpose(1, 2).reshape(B * T, d).to(BF16), lse2.squeeze(-1), dqkv.to(BF16), delta


def _measure(B, T, nh, hd, ds=None, seed=0, defect=None, at=None, qkv=None):
  if qkv is None:
    qkv, dout = _inputs(B, T, nh, hd, seed)
  else:
    _, dout = _inputs(B, T, nh, hd, seed)
  qr, out, lse, dqkv, delta = _standin(qkv, dout, B, T, nh, hd, ds, defect, at)
  ref = P.reference(qr, dout, B, T, nh, hd, ds, out=out, rope=O.rope_table(hd, T))
  return P.metrics(P.kernel_result(B, T, nh, hd, out, lse, dqkv, delta), ref)


def test_bwd_copy_is_the_stand_in():
  """The hook-free _bwd and _standin are exactly cpu_ref_bf16's attention (parity.standin)."""
  B, T, nh, hd = 2, 200, 2, 64
  qkv, dout = _inputs(B, T, nh, hd, 1)
  ds = O.doc_start_from_lengths(_random_docs(B, T, 1), T)
  for a, b in zip(_standin(qkv, dout, B, T, nh, hd, ds), P.standin(qkv, dout, B, T, nh, hd, ds)):
    assert torch.equal(a, b)


def test_reference_matches_the_fp32_oracle():
  """parity.reference is cpu_ref's attention: its fp64 out / gradients agree with the fp32 oracle + autograd to fp32 round-off."""
  B, T, nh, hd = 2, 96, 2, 64
  qkv, dout = _inputs(B, T, nh, hd, 2)
  ds = O.doc_start_from_lengths(_random_docs(B, T, 2), T)
  cos, sin = O.rope_table(hd, T)
  d = nh * hd
  leaf = qkv.float().requires_grad_(True)
  q, k, v = (t.reshape(B, T, nh, hd) for t in leaf.split(d, dim=1))
  out32 = O.attention(O.rope_apply(q, cos, sin), O.rope_apply(k, cos, sin), v, ds)
  out32.backward(dout.float().reshape(B, T, d))
  qr = torch.cat([O.rope_apply(q, cos, sin).reshape(B * T, d), O.rope_apply(k, cos, sin).reshape(B * T, d), v.reshape(B * T, d)], 1)
  ref = P.reference(qr.detach(), dout, B, T, nh, hd, ds, rope=(cos, sin))  # (fp32-rotated q, k: no bf16 rounding between the two)
  got = P.kernel_result(B, T, nh, hd, out=out32.reshape(B * T, d), dqkv=leaf.grad)
  for n in ('out', 'dq', 'dk', 'dv'):
    err = (got[n] - ref[n]).abs().max().item() / ref[n].abs().max().item()
    assert err <= 1e-5, (n, err)
  # the LSE is base 2: exp2(lse) sums exp2(scaled scores), i.e. the softmax denominator
  s = torch.einsum('bhid,bhjd->bhij', *P.split_qkv(qr.detach(), B, T, nh, hd)[:2]) / math.sqrt(hd) * P.LOG2E
  s = s.masked_fill(~P.allow_mask(B, T, ds), float('-inf'))
  assert torch.allclose(torch.exp2(s - ref['lse'][..., None]).sum(-1), torch.ones(B, nh, T, dtype=torch.float64), atol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# the honest stand-in passes at the GPU tests' shapes
# ---------------------------------------------------------------------------------------------------------------------
def _honest_cases():
  cases = []
  for B, T, nh in [(2, 64, 2), (1, 128, 1), (2, 256, 3), (1, 200, 2), (2, 320, 2), (3, 512, 1), (1, 836, 2), (1, 1024, 2)]:  # test_attention_fwd_bwd
    for masked in (False, True):
      cases.append((f'fwd_bwd {B}x{T}x{nh} masked={masked}', B, T, nh, 64, _random_docs(B, T, T) if masked else None))
  for hd in (32, 128):  # test_attention_other_head_dims
    for B, T, nh, masked in [(2, 64, 2, False), (1, 200, 3, True), (2, 512, 2, True), (1, 1024, 2, False), (3, 328, 1, True)]:
      cases.append((f'hd {hd} {B}x{T}x{nh} masked={masked}', B, T, nh, hd, _random_docs(B, T, T + hd) if masked else None))
  T = 512
  structures = {'one_doc': [[T + 1]] * 2, 'singletons': [[1] * (T + 1)] * 2, 'tile_aligned_64': [[64] * 8 + [1], [192, 64, 128, 128, 1]],
                'tile_aligned_128': [[128, 256, 128, 1], [256, 256, 1]], 'off_by_one': [[63, 65, 127, 129, 128, 1], [1, 127, 1, 255, 129]],
                'geometric_256': _random_docs(2, T, 5, mean=256), 'long_then_short': [[400, 30, 30, 30, 23], [7, 500, 6]]}
  for kind, docs in structures.items():  # test_attention_doc_mask_structures
    cases.append((f'structure {kind}', 2, T, 2, 64, docs))
  rng = np.random.default_rng(20261002)  # test_attention_doc_masks_random_shapes' sweep
  for case in range(24):
    B, nh = int(rng.integers(1, 5)), int(rng.integers(1, 4))
    T = 4 * int(rng.integers(1, 176)) if case % 3 else 4 * int(rng.integers(1, 20))
    mean = float(rng.choice([1.5, 7, 40, 150, 400, 2000]))
    docs = []
    for _ in range(B):
      lens, tot = [], 0
      while tot < T + 1:
        n = int(min(rng.geometric(1.0 / mean), T + 1 - tot))
        lens.append(n)
        tot += n
      docs.append(lens)
    cases.append((f'random shape {case} {B}x{T}x{nh}', B, T, nh, 64, docs))
  return cases


def test_honest_stand_in_within_budget():
  """Every bound of the budget holds for the stand-in at every shape the GPU attention tests use up to T = 1024 (their larger
  batches and the bench grids repeat these per-row shapes; the GPU tests measure them on the kernels themselves)."""
  worst = {}
  bad = []
  for i, (tag, B, T, nh, hd, docs) in enumerate(_honest_cases()):
    ds = None if docs is None else O.doc_start_from_lengths(docs, T)
    m = _measure(B, T, nh, hd, ds, seed=i)
    for k, v in m.items():
      worst[k] = max(worst.get(k, 0.0), v)
    if P.violations(m):
      bad.append((tag, P.violations(m)))
  print('honest floor (worst over the shapes):', ' '.join(f'{k}={v:.1e}' for k, v in worst.items()))
  assert not bad, bad


def test_honest_stand_in_within_budget_rescale_branch():
  """test_attention_softmax_rescale_branch's inputs: a late spike in the running max."""
  B, T, nh, d = 1, 256, 1, 64
  g = torch.Generator().manual_seed(3)
  qkv = 0.3 * torch.randn(B * T, 3 * d, generator=g)
  qkv[200, d:2 * d] = 6.0
  qkv[230:, 0:d] += 2.0
  m = _measure(B, T, nh, d, qkv=qkv.to(BF16))
  assert not P.violations(m), m


# ---------------------------------------------------------------------------------------------------------------------
# every planted defect is rejected, by the metric that is meant to catch it
# ---------------------------------------------------------------------------------------------------------------------
_DOCS = [[100, 37, 200, 176], [300, 13, 200]]  # T = 512
DEFECTS = [
    # (id, shape (B, T, nh, hd), documents, defect, where, metrics of which at least one must exceed its bound)
    ('scale_hd64', (2, 512, 2, 64), None, 'scale', None, ('proj_out', 'proj_dq', 'proj_dk', 'proj_dv')),
    ('scale_hd128', (2, 512, 2, 128), None, 'scale', None, ('proj_out', 'proj_dq', 'proj_dk', 'proj_dv')),
    ('scale_hd64_lse', (2, 512, 2, 64), None, 'scale', None, ('lse',)),
    ('drop_diagonal', (2, 512, 2, 64), None, 'drop_diagonal', 300, ('lse',)),
    ('drop_diagonal_doc', (2, 512, 2, 64), _DOCS, 'drop_diagonal', 330, ('lse', 'row_out')),
    ('skip_interior_tile', (2, 512, 2, 64), None, 'skip_key_tile', (288, 128), ('row_out', 'lse')),
    ('skip_ragged_last_tile', (2, 200, 2, 64), None, 'skip_key_tile', (192, 192), ('row_out', 'lse')),
    ('doc_start_minus_1', (2, 512, 2, 64), _DOCS, 'doc_start_minus_1', 140, ('lse', 'row_out')),
    ('doc_start_plus_1', (2, 512, 2, 64), _DOCS, 'doc_start_plus_1', 140, ('lse', 'row_out')),
    ('dv_last_row', (2, 512, 2, 64), None, 'dv_last_row', None, ('row_dv',)),
    ('dv_last_row_doc', (2, 512, 2, 64), _DOCS, 'dv_last_row', None, ('row_dv',)),
    ('dk_tile', (2, 512, 2, 64), None, 'dk_tile', ((320, 384), (128, 192)), ('row_dk',)),
    ('delta_zero', (2, 512, 2, 64), None, 'delta_zero', 200, ('delta', 'row_dq')),
    ('delta_scale', (2, 512, 2, 64), None, 'delta_scale', 200, ('delta',)),
    ('lse_shift', (2, 512, 2, 64), None, 'lse_shift', None, ('lse',)),
    ('rope_neighbour', (2, 512, 2, 64), None, 'rope_neighbour', 77, ('row_dq', 'row_dk')),
]


@pytest.mark.parametrize('name,shape,docs,defect,at,caught_by', DEFECTS, ids=[d[0] for d in DEFECTS])
def test_planted_defect_is_rejected(name, shape, docs, defect, at, caught_by):
  B, T, nh, hd = shape
  ds = None if docs is None else O.doc_start_from_lengths(docs, T)
  if defect.startswith('doc_start'):  # the edited row stays a valid mask row (it still sees itself) but not the document's first row
    assert 0 < int(ds[0, at]) < at
  m = _measure(B, T, nh, hd, ds, seed=7, defect=defect, at=at)
  bad = P.violations(m)
  print(f'{name}: ' + ' '.join(f'{k}={v:.1e}' for k, v in m.items()))
  assert any(k in bad for k in caught_by), (name, {k: m[k] for k in caught_by})
  # ... and with room to spare: the bounds sit at least 2x below what each defect produces
  assert max(bad[k][0] / bad[k][1] for k in caught_by if k in bad) >= 2.0, (name, {k: bad.get(k) for k in caught_by})


# ---------------------------------------------------------------------------------------------------------------------
# input classes off unit-normal data (parity.attn_inputs): peaked softmax, a growing running max, sinks, a late spike
# ---------------------------------------------------------------------------------------------------------------------
def _class_docs(B, T):
  """The document layouts of tests/test_attn_classes_gpu.py: _DOCS at T = 512, test_kernels_gpu.py's random lengths elsewhere."""
  return _DOCS if (B, T) == (2, 512) else _random_docs(B, T, T)


def _pipeline(qkv, dout, B, T, nh, hd, ds, fwd, bwd_lse=None):
  """parity.standin's steps around a forward ``fwd(q, k, v, allow, rb) -> (o, lse2)``; ``bwd_lse`` edits the LSE the backward reads."""
  rb = E._Round(True)
  cos, sin = O.rope_table(hd, T)
  d = nh * hd
  q, k, v = (t.float().reshape(B, T, nh, hd) for t in qkv.split(d, dim=1))
  qr, kr = E._rope(q, cos, sin, 1.0, rb), E._rope(k, cos, sin, 1.0, rb)
  qkv_rot = torch.cat([qr.reshape(B * T, d), kr.reshape(B * T, d), v.reshape(B * T, d)], dim=1).to(BF16)
  qh, kh, vh = (t.transpose(1, 2) for t in (qr, kr, v))
  allow = P.allow_mask(B, T, ds).expand(B, 1, T, T)
  o, lse2 = fwd(qh, kh, vh, allow, rb)
  do = dout.float().reshape(B, T, nh, hd).transpose(1, 2)
  dq, dk, dv, delta = _bwd(qh, kh, vh, o, do, lse2 if bwd_lse is None else bwd_lse(lse2), allow, rb)
  dq, dk = (E._rope(t.transpose(1, 2), cos, sin, -1.0, rb) for t in (dq, dk))
  dqkv = torch.cat([dq.reshape(B * T, d), dk.reshape(B * T, d), rb(dv.transpose(1, 2)).reshape(B * T, d)], dim=1)
  return qkv_rot, o.transpose(1, 2).reshape(B * T, d).to(BF16), lse2.squeeze(-1), dqkv.to(BF16), delta


def _ballot(need, group):
  """need bool [B, nh, T, 1] -> True for every row of a ``group``-row block in which some row needs: the kernels' wave-wide ballot."""
  B, nh, T, _ = need.shape
  pad = (-T) % group
  x = torch.nn.functional.pad(need.squeeze(-1), (0, pad)).reshape(B, nh, -1, group)
  return x.any(-1, keepdim=True).expand_as(x).reshape(B, nh, T + pad)[..., :T].unsqueeze(-1)


def _tiled_fwd(q, k, v, allow, rb, defect=None, tile=64, group=32, defer=8.0):
  """The forward of csrc/attn_causal.hip / attn_doc.hip step by step in fp32 torch: 64-key tiles, a running maximum mc (log2 units)
  whose update is DEFERRED until a tile's maximum exceeds it by more than 2^defer, and then taken by every row of the 32-row block
  (the wave-uniform ballot); p against mc, fp32 lsum, bf16 P into the PV product; lse = mc + log2(lsum).  Defects, one line each:
    no_alpha_lsum        alpha not applied to lsum
    alpha_half_o         alpha applied to d-columns [0, 32) of o only
    mc_other_group       mc updated for a row whose 32-row block did not rescale (the ballot of its 64-row pair)
    p_before_rescale     p taken against the new maximum and added before the rescale ran
    lse_pre_update_mc    lse written from the mc the row's last tile started with"""
  B, nh, T, hd = q.shape
  c2 = (1.0 / math.sqrt(hd)) * E.LOG2E
  mc = torch.full((B, nh, T, 1), float('-inf'))
  lsum = torch.zeros(B, nh, T, 1)
  o = torch.zeros(B, nh, T, hd)
  mc_in = mc
  for k0 in range(0, T, tile):
    k1 = min(T, k0 + tile)
    s = torch.matmul(q, k[:, :, k0:k1].transpose(-1, -2)).masked_fill(~allow[..., k0:k1], float('-inf'))
    tm = s.max(-1, keepdim=True).values * c2
    active = torch.isfinite(tm)  # rows that see a key of this tile
    mc_in = torch.where(active, mc, mc_in)
    need = tm > mc + defer  # both -inf: False
    upd = _ballot(need, group)
    mn = torch.maximum(mc, tm)
    alpha = torch.where(upd & torch.isfinite(mc), torch.exp2(mc - mn), torch.ones_like(mc))  # mc = -inf: lsum = o = 0, nothing to rescale
    mc_new = torch.where(_ballot(need, 2 * group) if defect == 'mc_other_group' else upd, mn, mc)
    mref = torch.where(torch.isinf(mc_new), torch.zeros_like(mc_new), mc_new)
    p = torch.exp2(s * c2 - mref)
    if defect == 'p_before_rescale':
      lsum, o = lsum + p.sum(-1, keepdim=True), o + torch.matmul(rb(p), v[:, :, k0:k1])
    if defect != 'no_alpha_lsum':
      lsum = lsum * alpha
    o = torch.cat([o[..., :32] * alpha, o[..., 32:]], dim=-1) if defect == 'alpha_half_o' else o * alpha
    if defect != 'p_before_rescale':
      lsum, o = lsum + p.sum(-1, keepdim=True), o + torch.matmul(rb(p), v[:, :, k0:k1])
    mc = mc_new
  if defect == 'lse_pre_update_mc':
    mc = torch.where(torch.isfinite(mc_in), mc_in, mc)
  return rb(o / lsum), mc + torch.log2(lsum)


def _split_fwd(q, k, v, allow, rb, S=7, defect=None, tile=64):
  """The split-KV forward of csrc/attn_cache.hip step by step in fp32 torch: the keys cut into S ranges (whole 64-key tiles), one partial
  (m, l, acc) per row and range from an online softmax that rescales in every tile, and the combine in split order, every partial
  weighted by exp2(m_s - m_max); lse = m_max + log2(l).  Defects, one line each:
    combine_m_first      the combine takes the first non-empty split's maximum for m_max
    combine_drop_last    the combine drops the last non-empty split"""
  B, nh, T, hd = q.shape
  c2 = (1.0 / math.sqrt(hd)) * E.LOG2E
  per = -(-(-(-T // S)) // tile) * tile
  parts = []
  for k_lo in range(0, T, per):
    m = torch.full((B, nh, T, 1), float('-inf'))
    l = torch.zeros(B, nh, T, 1)
    acc = torch.zeros(B, nh, T, hd)
    for k0 in range(k_lo, min(T, k_lo + per), tile):
      k1 = min(T, k_lo + per, k0 + tile)
      s = torch.matmul(q, k[:, :, k0:k1].transpose(-1, -2)).masked_fill(~allow[..., k0:k1], float('-inf')) * c2
      mn = torch.maximum(m, s.max(-1, keepdim=True).values)
      base = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
      alpha, p = torch.exp2(m - base), torch.exp2(s - base)
      l, acc, m = l * alpha + p.sum(-1, keepdim=True), acc * alpha + torch.matmul(rb(p), v[:, :, k0:k1]), mn
    parts.append((m, l, acc))
  ms = torch.stack([m for m, _, _ in parts])  # [S, B, nh, T, 1]
  full = torch.isfinite(ms)
  mm = ms.max(0).values
  if defect == 'combine_m_first':
    mm = torch.gather(ms, 0, full.float().argmax(0, keepdim=True))[0]
  if defect == 'combine_drop_last':
    last = len(parts) - 1 - full.flip(0).float().argmax(0, keepdim=True)
    full = full & ((torch.arange(len(parts)).view(-1, 1, 1, 1, 1) != last) | (last == 0))  # (a row with one split keeps it)
  ll = torch.zeros(B, nh, T, 1)
  a = torch.zeros(B, nh, T, hd)
  for i, (m, l, acc) in enumerate(parts):
    sc = torch.where(full[i], torch.exp2(m - mm), torch.zeros_like(m))  # an empty split carries no weight
    ll, a = ll + l * sc, a + acc * sc
  return rb(a / ll), mm + torch.log2(ll)


_FWD = {'flat': lambda defect: (lambda q, k, v, allow, rb: E._attn_fwd(q, k, v, allow, rb)),
        'tiled': lambda defect: (lambda q, k, v, allow, rb: _tiled_fwd(q, k, v, allow, rb, defect)),
        'split': lambda defect: (lambda q, k, v, allow, rb: _split_fwd(q, k, v, allow, rb, defect=defect))}


def _class_run(kind, cls, B, T, nh, hd, docs, defect=None, seed=11):
  """(metrics, outputs, late-rescale counts) of stand-in ``kind`` with ``defect`` on the class's inputs."""
  ds = None if docs is None else O.doc_start_from_lengths(docs, T)
  qkv, dout = P.attn_inputs(cls, B, T, nh, hd, seed, ds)
  bwd_lse = (lambda l: l.to(BF16).float()) if defect == 'bwd_bf16_lse' else None
  res = _pipeline(qkv, dout, B, T, nh, hd, ds, _FWD[kind](None if defect == 'bwd_bf16_lse' else defect), bwd_lse)
  qr, out, lse, dqkv, delta = res
  ref = P.reference(qr, dout, B, T, nh, hd, ds, out=out, rope=O.rope_table(hd, T))
  late = P.late_rescales(P.scores_log2(qr, B, T, nh, hd), P.allow_mask(B, T, ds))
  return P.metrics(P.kernel_result(B, T, nh, hd, out, lse, dqkv, delta), ref), res, late


def _class_shapes():
  """(hd, B, T, nh, masked) of tests/test_attn_classes_gpu.py up to T = 1024 (its cached cases repeat these rows at lengths up to 1100)."""
  shapes = [(64, 2, 512, 2, m) for m in (False, True)] + [(64, 1, 836, 1, m) for m in (False, True)]
  for hd in (32, 128):
    shapes += [(hd, 2, 512, 2, False), (hd, 2, 512, 2, True), (hd, 1, 328, 1, True)]
  return shapes + [(hd, 2, 200, 2, False) for hd in (32, 64, 128)]  # the bit-packed family's T


def _floor_line(tag, worst):
  print(f'{tag}: ' + ' '.join(f'{k}={v:.1e}' for k, v in worst.items()))


@pytest.mark.parametrize('cls', P.CLASSES)
def test_honest_stand_in_within_budget_on_the_input_classes(cls):
  """The stand-in is within the class's bounds at every shape of the GPU class tests, and every case's data does what its class
  promises: no late rescale on randn, at least one per (batch, head) on peaked / ramp / spike."""
  worst, bad = {}, []
  for hd, B, T, nh, masked in _class_shapes():
    m, _, late = _class_run('flat', cls, B, T, nh, hd, _class_docs(B, T) if masked else None, seed=1000 * hd + T + masked)
    P.assert_class_precondition(cls, late, f'hd {hd} B={B} T={T} masked={masked}')
    for k, v in m.items():
      worst[k] = max(worst.get(k, 0.0), v)
    if P.violations(m, cls):
      bad.append((hd, B, T, nh, masked, P.violations(m, cls)))
  _floor_line(f'honest floor on {cls} (worst over the shapes)', worst)
  assert not bad, bad


_STEPWISE_SHAPES = [(64, 2, 512, 2, False), (64, 2, 512, 2, True), (32, 1, 1024, 1, False), (128, 1, 328, 1, True)]


@pytest.mark.parametrize('cls', P.CLASSES)
@pytest.mark.parametrize('kind', ['tiled', 'split'])
def test_honest_stepwise_stand_ins_within_budget(kind, cls):
  """The tiled deferred-max forward and the split-KV forward, without a defect, are honest kernels under the budget on every class."""
  worst, bad = {}, []
  for hd, B, T, nh, masked in _STEPWISE_SHAPES:
    m, _, _ = _class_run(kind, cls, B, T, nh, hd, _class_docs(B, T) if masked else None)
    for k, v in m.items():
      worst[k] = max(worst.get(k, 0.0), v)
    if P.violations(m, cls):
      bad.append((hd, B, T, nh, masked, P.violations(m, cls)))
  _floor_line(f'honest {kind} stand-in on {cls} (worst over the shapes)', worst)
  assert not bad, bad


CLASS_DEFECTS = [
    # (defect, stand-in, class that rejects it, shape (B, T, nh, hd), metrics of which one must exceed its bound 2x, passes on randn)
    ('no_alpha_lsum', 'tiled', 'ramp', (2, 512, 2, 64), ('lse', 'row_out'), True),
    ('alpha_half_o', 'tiled', 'spike', (2, 512, 2, 64), ('row_out',), True),
    ('mc_other_group', 'tiled', 'peaked', (2, 512, 2, 64), ('lse', 'row_out'), True),
    ('p_before_rescale', 'tiled', 'ramp', (2, 512, 2, 64), ('lse', 'row_out'), True),
    ('lse_pre_update_mc', 'tiled', 'ramp', (2, 512, 2, 64), ('lse',), True),
    ('combine_m_first', 'split', 'ramp', (1, 1024, 1, 32), ('lse',), True),  # exp2(m_s - m_first) overflows: the maxima grow by > 128
    # not gaps: unit-normal data shows these two already (a dropped split holds 1 / S of a flat softmax's weight; bf16(lse) is off by up
    # to 2^-5 at lse ~ 9, 2 % of every p, 1.3x row_dv's bound) - the classes reject them with the 2x margin that randn does not give
    ('combine_drop_last', 'split', 'peaked', (2, 512, 2, 64), ('lse', 'row_out'), False),
    ('bwd_bf16_lse', 'tiled', 'ramp', (1, 1024, 1, 32), ('row_dv',), False),
]


@pytest.mark.parametrize('defect,kind,cls,shape,caught_by,randn_passes', CLASS_DEFECTS, ids=[d[0] for d in CLASS_DEFECTS])
def test_class_defect_passes_on_randn_and_is_rejected_on_its_class(defect, kind, cls, shape, caught_by, randn_passes):
  """The gap as a test: on unit-normal data at the same shape the defect's outputs equal the honest stand-in's bit for bit (the
  deferred-max ones: the rescale only ever runs on lsum = o = 0) or pass the budget; on its class a bound is exceeded at least 2x."""
  B, T, nh, hd = shape
  m0, res0, late0 = _class_run(kind, 'randn', B, T, nh, hd, None, defect)
  _, honest0, _ = _class_run(kind, 'randn', B, T, nh, hd, None)
  P.assert_class_precondition('randn', late0)
  same = all(torch.equal(a, b) for a, b in zip(res0, honest0))
  passes = same or not P.violations(m0)
  print(f'{defect}: passes on randn: {passes} (bit for bit: {same})')
  assert passes == randn_passes, (defect, P.violations(m0))
  if kind == 'tiled' and defect != 'bwd_bf16_lse':
    assert same  # not merely inside the budget: invisible
  m, _, late = _class_run(kind, cls, B, T, nh, hd, None, defect)
  P.assert_class_precondition(cls, late)
  bad = P.violations(m, cls)
  assert any(k in bad for k in caught_by), (defect, {k: m[k] for k in caught_by})
  ratio = max(bad[k][0] / bad[k][1] for k in caught_by if k in bad)
  print(f'{defect}: rejected on {cls} {ratio:.1f}x over its bound ' + ' '.join(f'{k}={m[k]:.1e}' for k in caught_by))
  assert ratio >= 2.0, (defect, {k: bad.get(k) for k in caught_by})


CLASS_BOUND_DEFECTS = [
    # the defects the per-class row bounds (parity.BOUNDS_BY_CLASS) must still catch, planted on that class's data
    ('peaked', 'rope_neighbour', 77, ('row_dq', 'row_dk')),
    ('peaked', 'dk_tile', ((320, 384), (128, 192)), ('row_dk',)),
    ('peaked', 'delta_zero', 200, ('row_dq',)),
    # ramp: a row's weight sits in its last key tiles, so only a tile next to the diagonal carries any dK (dropping (128, 192) for rows
    # 320 .. 383 changes nothing); the rotation defect moves the unit-normal part of q / k only and is left to the other classes
    ('ramp', 'dk_tile', ((320, 384), (256, 320)), ('row_dk',)),
    ('ramp', 'delta_zero', 200, ('row_dq',)),
]


@pytest.mark.parametrize('hd', [32, 64, 128])
@pytest.mark.parametrize('cls,defect,at,caught_by', CLASS_BOUND_DEFECTS, ids=[f'{d[0]}-{d[1]}' for d in CLASS_BOUND_DEFECTS])
def test_class_bounds_still_reject_the_planted_defects(cls, defect, at, caught_by, hd):
  """A class's own, wider row bounds sit at least 2x below what the defects they are there for produce on that class."""
  assert cls in P.BOUNDS_BY_CLASS
  B, T, nh = 2, 512, 2
  qkv, _ = P.attn_inputs(cls, B, T, nh, hd, 11)
  m = _measure(B, T, nh, hd, None, seed=7, defect=defect, at=at, qkv=qkv)
  bad = P.violations(m, cls)
  print(f'{cls} {defect} hd {hd}: ' + ' '.join(f'{k}={m[k]:.1e} (bound {P.bound_of(k, cls):.1e})' for k in caught_by))
  assert any(k in bad for k in caught_by), (cls, defect, {k: m[k] for k in caught_by})
  assert max(bad[k][0] / bad[k][1] for k in caught_by if k in bad) >= 2.0, (cls, defect, {k: bad.get(k) for k in caught_by})
