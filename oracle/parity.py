"""Error budget of the attention kernels.  TEST INFRASTRUCTURE ONLY (same rules as cpu_ref.py).

A single global number, max|got - ref| / max|ref|, lets a kernel be systematically wrong by a few 1e-3 (a softmax scale
off by 1 %, one row missing its diagonal key, dV missing the last query row) and still pass a per-cent tolerance.  This
file measures attention results the ways that separate such defects from honest bf16 rounding:

  * fp64 references (``reference``): out, the base-2 LSE, delta = rowsum(dO * O) and dQ / dK / dV, evaluated with
    cpu_ref.py's attention in float64 from the exact bf16 q, k (already rotated), v and dO the kernel saw; dQ / dK are
    taken back through the inverse RoPE in fp64, as the kernels' epilogues do;
  * row-local error (``row_local``): every row judged on its own scale, max|err| / max(rowmax|ref|, tau * scale) - a
    dropped key tile that is invisible against the tensor's global maximum is large against its own row;
  * projection coefficient (``projection``): |<g, r> / <r, r> - 1|.  Rounding noise of relative size s moves it by
    ~ s / sqrt(numel), a systematic error by its full size; per tensor and per (batch, head) slice;
  * LSE in absolute log2 units (every row sees at least its own key, so every LSE is finite) and delta relative to its
    row's rowsum |dO * O| (the size of the terms it cancels).

BOUNDS holds every bound the GPU tests and tests/test_parity_budget.py share.  Each was set from two measurements: the
honest floor (oracle/cpu_ref_bf16.py's attention, which rounds where the kernels round) and the worst value the MI355X
kernels show, with at least a 2x margin above the larger and at least 2x below the smallest planted defect of
tests/test_parity_budget.py.  Layout: tensors are [B, nh, T, hd] (rows along dim 2), LSE / delta [B, nh, T].

``attn_inputs`` draws the operands of the input classes beyond unit-normal data (peaked, ramp, sink, spike), ``late_rescales`` counts from
fp64 scores how often a class makes the deferred running-max update of the forward kernels fire, and BOUNDS_BY_CLASS holds the few
bounds a class needs of its own (profiles/attn_parity_classes.md has the measurements).
"""

from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import cpu_ref as O

Tensor = torch.Tensor
LOG2E = 1.4426950408889634

TAU = 0.05  # row-local scale floor, as a fraction of the tensor's (gradients: the dQ | dK | dV family's) max |ref|

BOUNDS = {
    'row': {'out': 1.5e-2, 'dq': 1.5e-1, 'dk': 1e-1, 'dv': 2e-2},   # row-local, max over rows
    'proj': {'out': 3e-3, 'dq': 6e-3, 'dk': 6e-3, 'dv': 3e-3},      # |c - 1| of the whole tensor
    'proj_slice': {'out': 3e-3, 'dq': 1e-2, 'dk': 1e-2, 'dv': 3e-3},  # |c - 1| of each (batch, head) slice
    'lse': 1e-4,                                                      # max |LSE2 - ref|, log2 units
    'delta': 1e-6,                                                    # max |delta - ref| / rowsum |dO * O|
}

# Bounds of their own for the input classes of ``attn_inputs`` on which BOUNDS keeps no 2x margin; everything absent here is BOUNDS.
# The same rule, from the measurements in profiles/attn_parity_classes.md: near one-hot rows make dS = P (dP - D) cancel, so the bf16
# rounding of dS is large against a row's own dQ / dK.  row dq: stand-in floor 0.13 (peaked) / 0.14 (ramp), MI355X 0.11 / 0.10, smallest
# planted defect it must catch on the class 1.9 (delta_zero); row dk: floor 0.087 / 0.085, MI355X 0.089 / 0.085, defect 0.52 (dk_tile).
BOUNDS_BY_CLASS: Dict[str, dict] = {
    'peaked': {'row': {'dq': 0.3, 'dk': 0.2}},
    'ramp': {'row': {'dq': 0.3, 'dk': 0.2}},
}


def heads(x: Tensor, B: int, T: int, nh: int, hd: int) -> Tensor:
  """[B*T, nh*hd] (the kernels' layout) -> [B, nh, T, hd] fp64 on the CPU."""
  return x.detach().double().cpu().reshape(B, T, nh, hd).transpose(1, 2)


def split_qkv(qkv: Tensor, B: int, T: int, nh: int, hd: int):
  """Projection layout [B*T, 3*nh*hd] -> q, k, v, each [B, nh, T, hd] fp64."""
  d = nh * hd
  return tuple(heads(qkv[:, i * d:(i + 1) * d], B, T, nh, hd) for i in range(3))


def rope64(x: Tensor, cos: Tensor, sin: Tensor, sgn: float) -> Tensor:
  """Interleaved-pair rotation of x [B, nh, T, hd] in fp64 with the fp32 tables the kernels use; sgn = -1 rotates back."""
  B, nh, T, hd = x.shape
  xf = x.reshape(B, nh, T, hd // 2, 2)
  a, b = xf[..., 0], xf[..., 1]
  c = cos[:T].double().reshape(1, 1, T, hd // 2)
  s = sin[:T].double().reshape(1, 1, T, hd // 2) * sgn
  return torch.stack([a * c - b * s, b * c + a * s], dim=-1).reshape(B, nh, T, hd)


def allow_mask(B: int, T: int, doc_start: Optional[Tensor]) -> Tensor:
  """bool [B or 1, 1, T, T], True = query i may see key j."""
  if doc_start is None:
    return torch.ones(T, T, dtype=torch.bool).tril().view(1, 1, T, T)
  return O.mask_from_doc_start(doc_start.cpu()).view(B, 1, T, T)


def reference(qkv_rot: Tensor, dout: Tensor, B: int, T: int, nh: int, hd: int, doc_start: Optional[Tensor] = None,
              out: Optional[Tensor] = None, rope=None) -> Dict[str, Tensor]:
  """fp64 attention from the bf16 operands a kernel saw: qkv_rot [B*T, 3*nh*hd] with q, k rotated, dout [B*T, nh*hd].
  Returns out, lse (base 2, the kernels' convention), delta = rowsum(dO * O) of ``out`` when given (the kernel's own bf16
  output: what its backward sums) else of the reference output, and dq / dk / dv; with rope = (cos, sin) dq / dk are
  the gradients w.r.t. the UN-rotated q, k (what plm_attn_bwd returns).  One batch row at a time."""
  q, k, v = split_qkv(qkv_rot, B, T, nh, hd)
  do = heads(dout, B, T, nh, hd)
  res = {n: [] for n in ('out', 'lse', 'dq', 'dk', 'dv')}
  for b in range(B):
    ds = None if doc_start is None else doc_start[b:b + 1].cpu()
    qb, kb, vb = (t[b:b + 1].transpose(1, 2).clone().requires_grad_(True) for t in (q, k, v))  # [1, T, nh, hd]
    ob = O.attention(qb, kb, vb, ds).reshape(1, T, nh, hd)
    ob.backward(do[b:b + 1].transpose(1, 2))
    s = torch.matmul(qb.detach().transpose(1, 2), kb.detach().transpose(1, 2).transpose(-1, -2)) / math.sqrt(hd)
    s = s.masked_fill(~allow_mask(1, T, ds), float('-inf'))
    res['lse'].append(torch.logsumexp(s, dim=-1) * LOG2E)
    res['out'].append(ob.detach().transpose(1, 2))
    for n, t in (('dq', qb), ('dk', kb), ('dv', vb)):
      res[n].append(t.grad.transpose(1, 2))
  ref = {n: torch.cat(t) for n, t in res.items()}
  ref['delta'], ref['delta_abs'] = delta_reference(ref['out'] if out is None else heads(out, B, T, nh, hd), do)
  if rope is not None:
    ref['dq'], ref['dk'] = (rope64(ref[n], rope[0], rope[1], -1.0) for n in ('dq', 'dk'))
  return ref


def delta_reference(o: Tensor, do: Tensor):
  """(rowsum(dO * O), rowsum |dO * O|) in fp64 from [B, nh, T, hd] operands; the second is the scale delta's error is judged on."""
  o, do = o.double(), do.double()
  return (do * o).sum(-1), (do * o).abs().sum(-1)


def to_rows(x: Tensor) -> Tensor:
  """[B, nh, T, hd] -> the kernels' [B*T, nh*hd] layout (inverse of heads)."""
  B, nh, T, hd = x.shape
  return x.transpose(1, 2).reshape(B * T, nh * hd)


def row_local(got: Tensor, ref: Tensor, scale: Optional[float] = None, tau: float = TAU) -> float:
  """max over rows of max|got - ref| / max(rowmax|ref|, tau * scale); scale defaults to the tensor's max |ref|."""
  got, ref = got.double(), ref.double()
  a = ref.abs().amax(-1)
  floor = tau * (a.max().item() if scale is None else scale)
  return ((got - ref).abs().amax(-1) / a.clamp_min(max(floor, 1e-300))).max().item()


def projection(got: Tensor, ref: Tensor, scale: Optional[float] = None, tau: float = TAU):
  """(|c - 1| of the whole tensor, worst |c - 1| over its (batch, head) slices), c = <g, r> / <r, r>.  Slices (or the
  tensor) whose max |ref| is below tau * scale carry no direction to measure and are skipped (0)."""
  got, ref = got.double(), ref.double()
  scale = ref.abs().max().item() if scale is None else scale

  def coef(g, r):
    if r.abs().max().item() < tau * scale or scale == 0.0:
      return 0.0
    r, g = r.flatten(), g.flatten()
    return abs((g @ r / (r @ r)).item() - 1.0)

  whole = coef(got, ref)
  worst = max(coef(got[b, h], ref[b, h]) for b in range(ref.shape[0]) for h in range(ref.shape[1]))
  return whole, worst


def metrics(got: Dict[str, Tensor], ref: Dict[str, Tensor]) -> Dict[str, float]:
  """Every metric for the entries present in ``got`` (out, lse, delta, dq, dk, dv in the layouts above)."""
  m = {}
  if 'out' in got:
    m['row_out'] = row_local(got['out'], ref['out'])
    m['proj_out'], m['proj_slice_out'] = projection(got['out'], ref['out'])
  gscale = max(ref[n].abs().max().item() for n in ('dq', 'dk', 'dv'))
  for n in ('dq', 'dk', 'dv'):
    if n in got:
      m['row_' + n] = row_local(got[n], ref[n], gscale)
      m['proj_' + n], m['proj_slice_' + n] = projection(got[n], ref[n], gscale)
  if 'lse' in got:
    m['lse'] = (got['lse'].double().cpu() - ref['lse']).abs().max().item()
  if 'delta' in got:
    m['delta'] = ((got['delta'].double().cpu() - ref['delta']).abs() / ref['delta_abs'].clamp_min(1e-30)).max().item()
  return m


def bound_of(key: str, cls: Optional[str] = None) -> float:
  """The bound of one metric of ``metrics`` ('row_dq', 'proj_slice_out', 'lse', ...): BOUNDS, or the input class's own entry."""
  by_cls = BOUNDS_BY_CLASS.get(cls, {})
  if key.startswith('row_'):
    return by_cls.get('row', {}).get(key[4:], BOUNDS['row'][key[4:]])
  if key.startswith('proj_slice_'):
    return by_cls.get('proj_slice', {}).get(key[11:], BOUNDS['proj_slice'][key[11:]])
  if key.startswith('proj_'):
    return by_cls.get('proj', {}).get(key[5:], BOUNDS['proj'][key[5:]])
  return by_cls.get(key, BOUNDS[key])


def violations(m: Dict[str, float], cls: Optional[str] = None) -> Dict[str, tuple]:
  """{metric: (value, bound)} for every metric above its bound (``cls``: an input class of attn_inputs with bounds of its own)."""
  bad = {}
  for key, val in m.items():
    bound = bound_of(key, cls)
    if not val <= bound:
      bad[key] = (val, bound)
  return bad


def check(got: Dict[str, Tensor], ref: Dict[str, Tensor], tag: str, cls: Optional[str] = None) -> Dict[str, float]:
  """Assert every metric of ``got`` within BOUNDS (``cls``: BOUNDS_BY_CLASS); prints them (one line, 'parity <tag>: ...') either way."""
  m = metrics(got, ref)
  print(f'parity {tag}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  bad = violations(m, cls)
  assert not bad, f'{tag}: ' + ', '.join(f'{k} {v:.3e} > {b:.1e}' for k, (v, b) in bad.items())
  return m


def kernel_result(B: int, T: int, nh: int, hd: int, out=None, lse=None, dqkv=None, delta=None) -> Dict[str, Tensor]:
  """The entry points' outputs ([B*T, nh*hd] out, [B*T, 3*nh*hd] dqkv, [B, nh, T] lse / delta) in the layouts ``metrics`` takes."""
  got = {}
  if out is not None:
    got['out'] = heads(out, B, T, nh, hd)
  if lse is not None:
    got['lse'] = lse.detach().double().cpu()
  if delta is not None:
    got['delta'] = delta.detach().double().cpu()
  if dqkv is not None:
    d = nh * hd
    for i, n in enumerate(('dq', 'dk', 'dv')):
      got[n] = heads(dqkv[:, i * d:(i + 1) * d], B, T, nh, hd)
  return got


# --------------------------------------------------------------------------------------
# input classes: attention operands off unit-normal data
# --------------------------------------------------------------------------------------
CLASSES = ('randn', 'peaked', 'ramp', 'sink', 'spike')
STRUCT_DIMS = 16  # structured parts live in the last 16 dims of a head: RoPE's lowest frequencies, <= ~0.13 rad over 1024 positions


def _doc_ranges(doc_start_row: Tensor, T: int):
  """[(start, end)] of the documents of one doc_start row [T]."""
  starts = torch.unique(doc_start_row[:T].long()).tolist()
  return list(zip(starts, starts[1:] + [T]))


def attn_inputs(cls: str, B: int, T: int, nh: int, hd: int, seed: int, doc_start: Optional[Tensor] = None):
  """Deterministic attention operands of one class: (qkv bf16 UN-rotated [B*T, 3*nh*hd], dout bf16 [B*T, nh*hd]), on the CPU.

    randn   what every other attention test draws: unit normal.
    peaked  randn with the q and k blocks times 3: scaled scores of std ~ 13 log2 units at any head dim, near one-hot P.
    ramp    randn; q's last 16 dims += 3, key j's last 16 dims += floor(j / 64): the running max grows in every key tile.
    sink    randn; q's last 16 dims += 2, the k row of every sequence's (with doc_start: every document's) first token has its
            last 16 dims set to 6: the maximum is fixed in the first visible tile and every later weight is tiny.
    spike   0.3 * randn; one key at 0.78 of the sequence (of every document) set to 6 in every dim, the queries after 0.9 of it
            += 2: tests/test_kernels_gpu.py::test_attention_softmax_rescale_branch's late jump of the running max, at any shape.
  """
  if cls not in CLASSES:
    raise ValueError(cls)
  g = torch.Generator().manual_seed(seed)
  d = nh * hd
  qkv = torch.randn(B * T, 3 * d, generator=g)
  dout = torch.randn(B * T, d, generator=g)
  x = qkv.view(B, T, 3, nh, hd)
  q, k = x[:, :, 0], x[:, :, 1]  # views: [B, T, nh, hd]
  lo = hd - STRUCT_DIMS
  if cls == 'peaked':
    q *= 3.0
    k *= 3.0
  elif cls == 'ramp':
    q[..., lo:] += 3.0
    k[..., lo:] += (torch.arange(T) // 64).float().view(1, T, 1, 1)
  elif cls == 'sink':
    q[..., lo:] += 2.0
    if doc_start is None:
      k[:, 0, :, lo:] = 6.0
    else:
      first = doc_start.cpu().long()[:, :T] == torch.arange(T).view(1, T)  # [B, T]
      k[..., lo:] = torch.where(first.view(B, T, 1, 1), torch.full_like(k[..., lo:], 6.0), k[..., lo:])
  elif cls == 'spike':
    qkv *= 0.3
    for b in range(B):
      for s, e in ([(0, T)] if doc_start is None else _doc_ranges(doc_start[b].cpu(), T)):
        n = e - s
        k[b, s + int(0.78125 * n)] = 6.0
        q[b, s + int(0.9 * n):e] += 2.0
  return qkv.to(torch.bfloat16), dout.to(torch.bfloat16)


def scores_log2(qkv_rot: Tensor, B: int, T: int, nh: int, hd: int) -> Tensor:
  """fp64 scaled scores q k^T / sqrt(hd) * log2(e) [B, nh, T, T] (unmasked) from the rotated bf16 operands: what the kernels' exp2 sees."""
  q, k, _ = split_qkv(qkv_rot, B, T, nh, hd)
  return torch.matmul(q, k.transpose(-1, -2)) * (LOG2E / math.sqrt(hd))


def late_rescales(s2: Tensor, allow: Tensor, tile: int = 64, defer: float = 8.0) -> Tensor:
  """How often the deferred running-max update of the causal / document forward kernels fires AFTER a row's first visible key tile:
  the number of (row, ``tile``-key tile) pairs at which the tile's largest visible score exceeds the row's running maximum by more
  than ``defer`` (both in log2 units; the kernels' ATTN_DEFER_LOG2 / DOC_DEFER_LOG2).  s2 [B, nh, Tq, Tk] from ``scores_log2``,
  allow bool broadcastable to it.  Returns the count per (batch, head), int64 [B, nh].  0 on unit-normal data: there the rescale
  (lsum *= alpha, o *= alpha) only ever runs on lsum = 0, o = 0."""
  B, nh, Tq, Tk = s2.shape
  s = s2.masked_fill(~allow.expand(B, nh, Tq, Tk), float('-inf'))
  mc = torch.full((B, nh, Tq), float('-inf'), dtype=s.dtype)
  count = torch.zeros(B, nh, dtype=torch.int64)
  for k0 in range(0, Tk, tile):
    tm = s[..., k0:k0 + tile].amax(-1)
    fire = tm > mc + defer  # -inf > -inf + defer: False
    count += (fire & torch.isfinite(mc)).sum(-1)
    mc = torch.where(fire, tm, mc)
  return count


def assert_class_precondition(cls: str, late: Tensor, tag: str = ''):
  """The classes stay honest when someone retunes them: randn never takes a late rescale, peaked / ramp / spike take one in every
  (batch, head); sink (the maximum sits in the first visible tile) is left to its own count."""
  if cls == 'randn':
    assert int(late.max()) == 0, (tag, cls, late.tolist())
  elif cls in ('peaked', 'ramp', 'spike'):
    assert int(late.min()) > 0, (tag, cls, late.tolist())


# --------------------------------------------------------------------------------------
# the honest floor: cpu_ref_bf16's attention, which rounds where the kernels round
# --------------------------------------------------------------------------------------
def standin(qkv: Tensor, dout: Tensor, B: int, T: int, nh: int, hd: int, doc_start: Optional[Tensor] = None):
  """The bf16-emulating attention of oracle/cpu_ref_bf16.py as a stand-in kernel, through the same entry-point contract:
  qkv (bf16, UN-rotated) -> (qkv_rot bf16, out bf16, lse fp32, dqkv bf16 w.r.t. the un-rotated projection, delta fp32),
  all in the kernels' layouts.  tests/test_parity_budget.py plants defects in copies of these steps."""
  from . import cpu_ref_bf16 as E
  rb = E._Round(True)
  cos, sin = O.rope_table(hd, T)
  d = nh * hd
  q, k, v = (t.float().reshape(B, T, nh, hd) for t in qkv.split(d, dim=1))
  qr, kr = E._rope(q, cos, sin, 1.0, rb), E._rope(k, cos, sin, 1.0, rb)
  qkv_rot = torch.cat([qr.reshape(B * T, d), kr.reshape(B * T, d), v.reshape(B * T, d)], dim=1).to(torch.bfloat16)
  qh, kh, vh = (t.transpose(1, 2) for t in (qr, kr, v))
  allow = allow_mask(B, T, doc_start)
  o, lse2 = E._attn_fwd(qh, kh, vh, allow, rb)
  do = dout.float().reshape(B, T, nh, hd).transpose(1, 2)
  dq, dk, dv = E._attn_bwd(qh, kh, vh, o, do, lse2, allow, rb)
  delta = (do * o).sum(-1)
  dq, dk = (E._rope(t.transpose(1, 2), cos, sin, -1.0, rb) for t in (dq, dk))
  dqkv = torch.cat([dq.reshape(B * T, d), dk.reshape(B * T, d), rb(dv.transpose(1, 2)).reshape(B * T, d)], dim=1)
  out = o.transpose(1, 2).reshape(B * T, d)
  return qkv_rot, out.to(torch.bfloat16), lse2.squeeze(-1), dqkv.to(torch.bfloat16), delta
