"""Attention parity off unit-normal data, on a real MI355X: every attention family against fp64 on the input classes of
oracle/parity.py's ``attn_inputs`` - peaked (near one-hot softmax), ramp (the running max grows in every key tile), sink (the maximum
sits on a sequence's / document's first token), spike (one late jump of the running max) - and exact power-of-two invariants.

On unit-normal data the deferred running-max update of the causal / document forward (csrc/attn_causal.hip, attn_doc.hip) never fires
after a row's first visible tile, the every-tile rescales of the other families run with alpha close to 1, and the backward's exp2
argument stays below 8; tests/test_parity_budget.py plants the defects that therefore pass every unit-normal test and shows that
these classes reject them.  Every case first asserts, from the fp64 scores, that its data does what its class promises
(parity.late_rescales).  References are computed once per (class, shape) and never modified.  Bounds: parity.BOUNDS, with the entries of
parity.BOUNDS_BY_CLASS where a class has its own (profiles/attn_parity_classes.md holds the measurements both are set from)."""

import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity as PB  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_attn_masked_gpu as TM  # noqa: E402

BF16 = torch.bfloat16
CLASSES = ('peaked', 'ramp', 'sink', 'spike')
DOCS_512 = [[100, 37, 200, 176], [300, 13, 200]]  # tests/test_parity_budget.py's _DOCS
KS = (-3, 4)  # the exact invariants' powers of two


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


def bits(t):
  return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def biteq(a, b):
  return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _random_docs(B, T, seed):
  """tests/test_kernels_gpu.py's document lengths."""
  rng = np.random.default_rng(seed)
  out = []
  for _ in range(B):
    lens, tot = [], 0
    while tot < T + 1:
      n = int(min(rng.integers(1, max(2, T // 3)), T + 1 - tot))
      lens.append(n)
      tot += n
    out.append(lens)
  return out


def _docs(B, T):
  return DOCS_512 if (B, T) == (2, 512) else _random_docs(B, T, T)


# --------------------------------------------------------------------------------------
# the training families: causal / document hd 64, generic hd 32 / 128
# --------------------------------------------------------------------------------------
TRAIN_SHAPES = [(64, 2, 512, 2, False), (64, 2, 512, 2, True), (64, 1, 836, 1, False), (64, 1, 836, 1, True),  # 836: ragged, four 256-row query tiles
                (32, 2, 512, 2, False), (32, 2, 512, 2, True), (32, 1, 328, 1, True),
                (128, 2, 512, 2, False), (128, 2, 512, 2, True), (128, 1, 328, 1, True)]
_train = {}


def train_case(ops, cls, hd, B, T, nh, masked):
  """Operands of one (class, shape), the rotated projection the kernels see, its fp64 reference and its late-rescale counts."""
  key = (cls, hd, B, T, nh, masked)
  if key not in _train:
    ds = O.doc_start_from_lengths(_docs(B, T), T) if masked else None
    qkv, dout = PB.attn_inputs(cls, B, T, nh, hd, 1000 * hd + T + masked, ds)
    cos, sin = O.rope_table(hd, T)
    qrot = ops.rope_qk_(qkv.cuda(), cos.cuda(), sin.cuda(), B, T, nh)
    ref = PB.reference(qrot, dout, B, T, nh, hd, ds, rope=(cos, sin))
    late = PB.late_rescales(PB.scores_log2(qrot, B, T, nh, hd), PB.allow_mask(B, T, ds))
    _train[key] = dict(ds=ds, dsg=None if ds is None else ds.cuda(), dout=dout, doutg=dout.cuda(), cos=cos.cuda(), sin=sin.cuda(),
                       qrot=qrot, ref=ref, late=late)
  return _train[key]


def with_delta_of(ref, out, dout, B, T, nh, hd):
  """A copy of the shared reference whose delta is rowsum(dO * O) of the kernel's own bf16 out: what its backward sums."""
  r = dict(ref)
  r['delta'], r['delta_abs'] = PB.delta_reference(PB.heads(out, B, T, nh, hd), PB.heads(dout, B, T, nh, hd))
  return r


@pytest.mark.parametrize('cls', CLASSES)
@pytest.mark.parametrize('hd,B,T,nh,masked', TRAIN_SHAPES)
def test_attention_classes_fwd_bwd(ops, hd, B, T, nh, masked, cls):
  """out, LSE, delta and dQ / dK / dV of attn_fwd / attn_bwd against fp64, as test_attention_fwd_bwd judges them."""
  c = train_case(ops, cls, hd, B, T, nh, masked)
  tag = f'{cls} hd {hd} B={B} T={T} nh={nh} masked={masked}'
  PB.assert_class_precondition(cls, c['late'], tag)
  out, lse = ops.attn_fwd(c['qrot'], B, T, nh, c['dsg'])
  assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
  dqkv, delta = ops.attn_bwd(c['qrot'], out, c['doutg'], lse, c['cos'], c['sin'], B, T, nh, c['dsg'], return_delta=True)
  assert torch.isfinite(dqkv.float()).all()
  ref = with_delta_of(c['ref'], out, c['dout'], B, T, nh, hd)
  PB.check(PB.kernel_result(B, T, nh, hd, out, lse, dqkv, delta), ref, f'classes late={int(c["late"].sum())} {tag}', cls)


@pytest.mark.parametrize('B,T,nh,masked', [s[1:] for s in TRAIN_SHAPES if s[0] == 64])
def test_attention_classes_bwd_decoupled_from_fwd(ops, B, T, nh, masked):
  """The hd-64 backward fed the fp64 reference's out (rounded to bf16) and LSE on peaked data: |s c2| of ~100 in its exp2, dS = P (dP - D)
  cancelling on near one-hot rows, with no help from a quirk of the forward's own out / lse."""
  c = train_case(ops, 'peaked', 64, B, T, nh, masked)
  PB.assert_class_precondition('peaked', c['late'])
  out_ref = PB.to_rows(c['ref']['out']).to(BF16)
  ref = with_delta_of(c['ref'], out_ref, c['dout'], B, T, nh, 64)
  dqkv, delta = ops.attn_bwd(c['qrot'], out_ref.cuda(), c['doutg'], c['ref']['lse'].float().cuda(), c['cos'], c['sin'], B, T, nh, c['dsg'],
                             return_delta=True)
  PB.check(PB.kernel_result(B, T, nh, 64, dqkv=dqkv, delta=delta), ref, f'classes decoupled peaked B={B} T={T} nh={nh} masked={masked}', 'peaked')


def _scaled(x, k):
  return (x.float() * 2.0 ** k).to(x.dtype)


def _train_invariants(run, qrot, dout, d):
  """run(qrot, dout) -> (out, lse, dqkv, delta).  A power of two commutes with every rounding of these kernels (the PV and dP MFMAs, the
  alpha rescale, the bf16 stores): v * 2^k scales out, delta, dq, dk by exactly 2^k and leaves lse and dv alone; dout * 2^k scales
  dq, dk, dv and delta by exactly 2^k."""
  out, lse, dqkv, delta = run(qrot, dout)
  for k in KS:
    q2 = qrot.clone()
    q2[:, 2 * d:] = _scaled(qrot[:, 2 * d:], k)
    assert torch.equal(q2[:, 2 * d:].float(), qrot[:, 2 * d:].float() * 2.0 ** k)  # the scaling itself is exact
    o2, l2, g2, d2 = run(q2, dout)
    assert biteq(o2, _scaled(out, k)) and torch.equal(l2, lse), ('v', k, 'out / lse')
    assert biteq(d2, _scaled(delta, k)), ('v', k, 'delta')
    assert biteq(g2[:, :2 * d], _scaled(dqkv[:, :2 * d], k)), ('v', k, 'dq | dk')
    assert biteq(g2[:, 2 * d:], dqkv[:, 2 * d:]), ('v', k, 'dv')
    o3, l3, g3, d3 = run(qrot, _scaled(dout, k))
    assert biteq(o3, out) and torch.equal(l3, lse)
    assert biteq(g3, _scaled(dqkv, k)), ('dout', k, 'dqkv')
    assert biteq(d3, _scaled(delta, k)), ('dout', k, 'delta')


@pytest.mark.parametrize('hd,B,T,nh,masked', [(64, 1, 836, 1, False), (64, 1, 836, 1, True), (32, 2, 512, 2, False), (32, 1, 328, 1, True),
                                              (128, 2, 512, 2, False), (128, 1, 328, 1, True)])
def test_attention_power_of_two_invariants(ops, hd, B, T, nh, masked):
  c = train_case(ops, 'peaked', hd, B, T, nh, masked)
  PB.assert_class_precondition('peaked', c['late'])

  def run(qrot, dout):
    out, lse = ops.attn_fwd(qrot, B, T, nh, c['dsg'])
    dqkv, delta = ops.attn_bwd(qrot, out, dout, lse, c['cos'], c['sin'], B, T, nh, c['dsg'], return_delta=True)
    return out, lse, dqkv, delta

  _train_invariants(run, c['qrot'], c['doutg'], nh * hd)


# --------------------------------------------------------------------------------------
# the bit-packed masked family
# --------------------------------------------------------------------------------------
M_B, M_T, M_NH = 2, 200, 2
M_MASKS = ('causal', 'bern0.5')  # the dense causal mask; a non-block-diagonal one of test_attn_masked_gpu.MASKS
_masked = {}


def masked_case(ops, cls, hd, kind):
  key = (cls, hd, kind)
  if key not in _masked:
    assert kind in TM.MASKS
    B, T, nh = M_B, M_T, M_NH
    qkv, dout = PB.attn_inputs(cls, B, T, nh, hd, 77 * hd + TM.MASKS.index(kind))
    mask = TM.make_mask(kind, B, T, hd)
    cos, sin = O.rope_table(hd, T)
    qrot = ops.rope_qk_(qkv.cuda(), cos.cuda(), sin.cuda(), B, T, nh)
    ref, empty = TM.masked_reference(qrot, dout, mask, B, T, nh, hd, torch.zeros(B * T, nh * hd), (cos, sin))
    assert not empty.any()
    late = PB.late_rescales(PB.scores_log2(qrot, B, T, nh, hd), mask.view(B, 1, T, T))
    bits_, tcls = ops.attn_mask_pack(mask.cuda())
    _masked[key] = dict(dout=dout, doutg=dout.cuda(), cos=cos.cuda(), sin=sin.cuda(), qrot=qrot, ref=ref, late=late, bits=bits_, tcls=tcls)
  return _masked[key]


def _run_masked(ops, c, qrot, dout):
  out, lse = ops.attn_fwd_masked(qrot, c['bits'], c['tcls'], M_B, M_T, M_NH)
  dqkv, delta = ops.attn_bwd_masked(qrot, out, dout, lse, c['cos'], c['sin'], c['bits'], c['tcls'], M_B, M_T, M_NH, return_delta=True)
  return out, lse, dqkv, delta


@pytest.mark.parametrize('cls', CLASSES)
@pytest.mark.parametrize('kind', M_MASKS)
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_masked_attention_classes(ops, hd, kind, cls):
  c = masked_case(ops, cls, hd, kind)
  tag = f'{cls} masked {kind} hd {hd} B={M_B} T={M_T} nh={M_NH}'
  PB.assert_class_precondition(cls, c['late'], tag)
  out, lse, dqkv, delta = _run_masked(ops, c, c['qrot'], c['doutg'])
  for t in (out, lse, dqkv, delta):
    assert torch.isfinite(t.float()).all()
  ref = with_delta_of(c['ref'], out, c['dout'], M_B, M_T, M_NH, hd)
  PB.check(PB.kernel_result(M_B, M_T, M_NH, hd, out, lse, dqkv, delta), ref, f'classes late={int(c["late"].sum())} {tag}', cls)


@pytest.mark.parametrize('hd', [32, 64, 128])
def test_masked_attention_power_of_two_invariants(ops, hd):
  c = masked_case(ops, 'peaked', hd, 'bern0.5')
  PB.assert_class_precondition('peaked', c['late'])
  _train_invariants(lambda qrot, dout: _run_masked(ops, c, qrot, dout), c['qrot'], c['doutg'], M_NH * hd)


# --------------------------------------------------------------------------------------
# the cached families: decode and extend
# --------------------------------------------------------------------------------------
C_TMAX, C_NH = 1100, 2
C_LENS = (1, 64, 65, 257, 1024, 1100)
C_SPLITS = (1, 7, 0)
E_LENS0 = (0, 70, 900)
E_SPLITS = (1, 3, 0)
_cache = {}


def _rows_ref(q, kv, pos, nh, hd):
  """fp64 attention of rotated query rows q [R, nh*hd] of ONE sequence, row r over keys 0 .. pos[r] of its cache kv [Tmax, 2*nh*hd]:
  (out [nh, R, hd], base-2 lse [nh, R])."""
  R, d = q.shape
  Tm = kv.shape[0]
  qh = q.double().cpu().view(R, nh, hd).transpose(0, 1)
  k, v = (kv[:, i * d:(i + 1) * d].double().cpu().view(Tm, nh, hd).transpose(0, 1) for i in range(2))
  s = torch.matmul(qh, k.transpose(-1, -2)) / math.sqrt(hd)
  s = s.masked_fill(torch.arange(Tm).view(1, 1, Tm) > torch.as_tensor(pos).view(1, R, 1), float('-inf'))
  return torch.matmul(torch.softmax(s, dim=-1), v), torch.logsumexp(s, dim=-1) * PB.LOG2E


def cache_case(ops, cls, hd):
  """Six sequences of C_TMAX rotated rows of one class: the cache = their k | v columns, the queries = their q columns."""
  key = (cls, hd)
  if key not in _cache:
    B, T, nh, d = len(C_LENS), C_TMAX, C_NH, C_NH * hd
    qkv, _ = PB.attn_inputs(cls, B, T, nh, hd, 31 * hd + 5)
    cos, sin = O.rope_table(hd, T)
    qrot = ops.rope_qk_(qkv.cuda(), cos.cuda(), sin.cuda(), B, T, nh)
    q3 = qrot.view(B, T, 3 * d)
    late = torch.cat([PB.late_rescales(PB.scores_log2(q3[b].contiguous(), 1, T, nh, hd), PB.allow_mask(1, T, None)) for b in range(B)])
    _cache[key] = dict(kv=q3[:, :, d:].contiguous(), q=q3[:, :, :d].contiguous(), late=late, ref={})
  return _cache[key]


def _cache_metrics(got_o, got_l, want_o, want_l):
  m = {'row_out': PB.row_local(got_o, want_o)}
  m['proj_out'], m['proj_slice_out'] = PB.projection(got_o, want_o)
  m['lse'] = (got_l - want_l).abs().max().item()
  return m


@pytest.mark.parametrize('cls', ['randn', 'peaked', 'sink'])
@pytest.mark.parametrize('splits', C_SPLITS)
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_decode_classes(ops, hd, splits, cls):
  """plm_attn_decode at lengths up to 1100: the partials' maxima differ by tens of log2 units on peaked data and the first split holds all
  the weight on sink data.  randn: at hd 32 one trip of the decode loop covers 4 waves * 16 keys * 4 loads = 256 keys, so only lengths
  above 256 at splits = 1 take a second trip.  sink: proj_slice_out is printed, not asserted - a slice here is ONE row, out = v_0 (1 - w) +
  ... with the other keys' weight w below bf16's half-ulp (2^-9 .. 2^-8 of an element), so every element of an honest kernel's row rounds
  back to v_0 and the coefficient is 1 / (1 - w): up to 3.9e-3 from the output format alone (measured 1.7e-3 at hd 128), no 2x below the
  1e-2 of the scale defect the metric is there for.  row_out, the whole-tensor coefficient and lse carry the class."""
  assert max(C_LENS) > 4 * 16 * 4 and 1 in C_SPLITS
  c = cache_case(ops, cls, hd)
  PB.assert_class_precondition(cls, c['late'], f'decode {cls} hd {hd}')
  B, d = len(C_LENS), C_NH * hd
  rows = torch.tensor(C_LENS) - 1
  if 'decode' not in c['ref']:
    refs = [_rows_ref(c['q'][b, rows[b]:rows[b] + 1], c['kv'][b], rows[b:b + 1], C_NH, hd) for b in range(B)]
    c['ref']['decode'] = (torch.stack([o for o, _ in refs]), torch.stack([l for _, l in refs]))  # [B, nh, 1, hd], [B, nh, 1]
  want_o, want_l = c['ref']['decode']
  q = c['q'][torch.arange(B).cuda(), rows.cuda()].contiguous()
  lens = torch.tensor(C_LENS, dtype=torch.int32).cuda()
  out, lse = ops.attn_decode(q, c['kv'], lens, C_NH, splits=splits, want_lse=True)
  assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
  m = _cache_metrics(out.double().cpu().view(B, C_NH, 1, hd), lse.double().cpu().view(B, C_NH, 1), want_o, want_l)
  print(f'parity classes {cls} decode hd={hd} splits={splits}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  if cls == 'sink':
    del m['proj_slice_out']
  bad = PB.violations(m, cls)
  assert not bad, bad
  assert q.shape == (B, d)


@pytest.mark.parametrize('cls', ['peaked', 'ramp'])
@pytest.mark.parametrize('splits', E_SPLITS)
@pytest.mark.parametrize('n', [33, 130])
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_extend_classes(ops, hd, n, splits, cls):
  """plm_attn_extend: chunks of n rows appended at lengths 0, 70 and 900 of an 1100-row cache."""
  c = cache_case(ops, cls, hd)
  B = len(E_LENS0)
  PB.assert_class_precondition(cls, c['late'][:B], f'extend {cls} hd {hd}')
  assert max(E_LENS0) + n <= C_TMAX
  if ('extend', n) not in c['ref']:
    refs = [_rows_ref(c['q'][b, l0:l0 + n], c['kv'][b], torch.arange(l0, l0 + n), C_NH, hd) for b, l0 in enumerate(E_LENS0)]
    c['ref'][('extend', n)] = (torch.stack([o for o, _ in refs]), torch.stack([l for _, l in refs]))  # [B, nh, n, hd], [B, nh, n]
  want_o, want_l = c['ref'][('extend', n)]
  q = torch.stack([c['q'][b, l0:l0 + n] for b, l0 in enumerate(E_LENS0)]).reshape(B * n, C_NH * hd).contiguous()
  lens0 = torch.tensor(E_LENS0, dtype=torch.int32).cuda()
  out, lse = ops.attn_extend(q, c['kv'][:B].contiguous(), lens0, C_NH, splits=splits, want_lse=True)
  assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
  m = _cache_metrics(out.double().cpu().view(B, n, C_NH, hd).transpose(1, 2), lse.double().cpu().view(B, C_NH, n), want_o, want_l)
  print(f'parity classes {cls} extend hd={hd} n={n} splits={splits}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  bad = PB.violations(m, cls)
  assert not bad, bad


@pytest.mark.parametrize('hd', [32, 64, 128])
def test_cached_attention_power_of_two_invariants(ops, hd):
  """v * 2^k in the cache: out scales by exactly 2^k and lse keeps its bits, through the partials and the combine at every split count."""
  c = cache_case(ops, 'peaked', hd)
  PB.assert_class_precondition('peaked', c['late'])
  B, d = len(C_LENS), C_NH * hd
  rows = torch.tensor(C_LENS) - 1
  qd = c['q'][torch.arange(B).cuda(), rows.cuda()].contiguous()
  lens = torch.tensor(C_LENS, dtype=torch.int32).cuda()
  Be, n = len(E_LENS0), 130
  qe = torch.stack([c['q'][b, l0:l0 + n] for b, l0 in enumerate(E_LENS0)]).reshape(Be * n, d).contiguous()
  lens0 = torch.tensor(E_LENS0, dtype=torch.int32).cuda()
  for k in KS:
    kv2 = c['kv'].clone()
    kv2[:, :, d:] = _scaled(c['kv'][:, :, d:], k)
    for splits in C_SPLITS:
      out, lse = ops.attn_decode(qd, c['kv'], lens, C_NH, splits=splits, want_lse=True)
      o2, l2 = ops.attn_decode(qd, kv2, lens, C_NH, splits=splits, want_lse=True)
      assert biteq(o2, _scaled(out, k)) and torch.equal(l2, lse), ('decode', k, splits)
    for splits in E_SPLITS:
      out, lse = ops.attn_extend(qe, c['kv'][:Be].contiguous(), lens0, C_NH, splits=splits, want_lse=True)
      o2, l2 = ops.attn_extend(qe, kv2[:Be].contiguous(), lens0, C_NH, splits=splits, want_lse=True)
      assert biteq(o2, _scaled(out, k)) and torch.equal(l2, lse), ('extend', k, splits)
