"""The attention error budget (oracle/parity.py) against planted defects, on the CPU.

The stand-in kernel is the bf16-emulating attention of oracle/cpu_ref_bf16.py: it rounds where the HIP kernels round, so
it is what an honest kernel looks like under the budget.  Each defect below is a small edit of that stand-in, in Python,
of the kind a rewrite of the masking, scaling or row/tile bookkeeping of the attention kernels tends to introduce.  The
budget must ACCEPT the honest stand-in at the shapes the GPU tests use, and REJECT every defect - most of which pass
the older rel-to-max tolerances (1.6e-2 out, 2e-2 gradients).  Nothing here launches a kernel."""

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
