"""The kernels that end a training step on MI355X, held to exact or element-level checks (oracle/parity_tail.py; calibrated on the
CPU by tests/test_parity_budget_tail.py; measured values in profiles/tail_parity.md):

  * reductions (plm_sumsq_f32, plm_mean_f32, plm_colsum_f32_multi, the atomic plm_embed_bwd, plm_axpy_f32, plm_scale_bf16) on
    inputs whose every partial sum is exact in fp32: the result is the same for any order, tree or FMA contraction and is compared
    with ==, at every length where a loop bound, a tail or a launch boundary changes;
  * plm_embed_bwd_sorted bit for bit against the fp32 sum in token order its contract names, plm_embed_fwd against W[ids];
  * the fp32 -> bf16 casts on the rounding edges;
  * the five optimizers against fp64, element by element, on input classes beyond unit-normal data; exact invariants; non-finite
    isolation; the second trip of the flat kernels' grid-stride loops.
Shapes are the smallest at which each path can go wrong; none is the workload's."""

import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import parity_tail as PT  # noqa: E402

F32, BF16, I64 = torch.float32, torch.bfloat16, torch.int64
NAN = float('nan')


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


def span(x, offset=1):
  """x on the GPU as a span that starts ``offset`` elements into a larger buffer (4 bytes off 16-byte alignment for offset 1)"""
  buf = torch.empty(x.numel() + 8, dtype=x.dtype, device='cuda')
  s = buf[offset:offset + x.numel()]
  s.copy_(x.reshape(-1))
  return s


# ---------------------------------------------------------------------------------------------------------------------
# reductions on exact-sum inputs
# ---------------------------------------------------------------------------------------------------------------------
SUMSQ_N = [1, 3, 4, 5, 4095, 4096, 4097, 4 * 1024 * 2048 - 1, 4 * 1024 * 2048, 4 * 1024 * 2048 + 5]  # the last: past the 2048-block cap


@pytest.mark.parametrize('n', SUMSQ_N)
def test_sumsq_exact(ops, n):
  """values in {-1, 0, 1} (n <= 2^23 + 5 < 2^24: every partial sum an exact integer) and, for the short lengths, {+-0.5, +-1, +-2}
  (multiples of 2^-2 below 2^14); then one-hot probes at both ends, the float4 / tail boundary and the block boundaries"""
  sets = [(-1.0, 0.0, 1.0)] + ([(-0.5, 0.5, -1.0, 1.0, -2.0, 2.0)] if n < 1_000_000 else [])
  for vals in sets:
    x = PT.exact_sum_inputs(n, n, vals)
    want = (x.double() ** 2).sum().item()
    assert want / min(abs(v) for v in vals if v) ** 2 < 2 ** 24      # in quanta of the smallest square
    assert ops.sumsq(x.cuda()).item() == want, (n, vals)
  x = torch.zeros(n, device='cuda')
  for i in PT.onehot_indices(n):
    x[i] = 1.0
    got = ops.sumsq(x).item()
    x[i] = 0.0
    assert got == 1.0, (n, i, got)


def test_sumsq_refuses_unaligned_input(ops):
  x = torch.ones(17, device='cuda')
  with pytest.raises(RuntimeError, match='16-byte aligned'):
    ops.sumsq(x[1:])


MEAN_N = [1, 63, 64, 65, 1023, 1024, 1025, 32768, 65537]


def test_mean_exact(ops):
  """integer data in [-8, 8] (|partial sums| <= 2^19.1): where the sum is a multiple of n the mean is that integer exactly; else it is
  within one ulp of fl32(S) / fl32(n) (one correctly rounded division: bit-equal unless the device's division is not)"""
  off = 0
  for n in MEAN_N:
    x = PT.exact_sum_inputs(n, 100 + n, range(-7, 9))
    S = int(x.double().sum().item())
    got = ops.mean(x.cuda()).item()
    want = float(np.float32(S) / np.float32(n))
    off += got != want
    assert abs(got - want) <= float(np.spacing(np.float32(abs(want)))), (n, got, want)
    r = S % n
    x[:r] -= 1.0                                     # values stay >= -8; the sum is now a multiple of n
    S = int(x.double().sum().item())
    assert S % n == 0
    assert ops.mean(x.cuda()).item() == float(S // n), n
    one = torch.zeros(n)
    one[n - 1] = float(n)                            # the last element counts: mean exactly 1
    assert ops.mean(one.cuda()).item() == 1.0, n
  print(f'mean: {off} of {len(MEAN_N)} random-sum cases not bit-equal to fl32(S) / fl32(n)')


COLSUM_ROWS = [1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 1024]   # around the 64-row main loop (r + 48 < rows) and the 16-row remainder
COLSUM_COLS = [1, 63, 64, 65, 768]


@pytest.mark.parametrize('rows', COLSUM_ROWS)
def test_colsum_multi_exact(ops, rows):
  """65 items (two launches: 64 + 1) of integers in [-8, 8]; items 5, 63 and 64 accumulate onto integer contents, the others
  overwrite NaN; then the probe: one 1 per column at row c % rows, every output exactly 1"""
  acc = {5, 63, 64}
  gen = torch.Generator(device='cuda').manual_seed(rows)
  for cols in COLSUM_COLS:
    parts = torch.randint(-8, 9, (65, rows, cols), device='cuda', generator=gen).float()
    prior = torch.randint(-100, 101, (65, cols), device='cuda', generator=gen).float()
    outs = torch.full((65, cols), NAN, device='cuda')
    for i in acc:
      outs[i] = prior[i]
    ops.colsum_multi([(parts[i], outs[i], i in acc) for i in range(65)])
    want = parts.long().sum(1)
    for i in acc:
      want[i] += prior[i].long()
    bad = torch.nonzero(outs != want.float())
    assert bad.numel() == 0, (rows, cols, bad[:4].tolist())
    probe = torch.zeros(2, rows, cols, device='cuda')
    c = torch.arange(cols, device='cuda')
    probe[:, c % rows, c] = 1.0
    po = torch.full((2, cols), NAN, device='cuda')
    po[1] = 0.0
    ops.colsum_multi([(probe[0], po[0], False), (probe[1], po[1], True)])
    assert bool((po == 1.0).all()), (rows, cols)


@pytest.mark.parametrize('M', [1, 5, 1025])
@pytest.mark.parametrize('d', [4, 260])
def test_embed_bwd_atomic_exact(ops, M, d):
  """integer gradients onto integer contents, three ids shared by all tokens, ids outside [0, V) ignored: atomics in any order are exact"""
  g = torch.Generator().manual_seed(M * d)
  V = 3
  ids = torch.randint(-1, V + 1, (M,), generator=g)
  dout = torch.randint(-8, 9, (M, d), generator=g).float()
  dW0 = torch.randint(-50, 51, (V, d), generator=g).float()
  ok = (ids >= 0) & (ids < V)
  want = dW0.double().index_add_(0, ids[ok], dout[ok].double()).float()
  dW = dW0.cuda()
  ops.embed_bwd(ids.cuda(), dout.cuda(), dW)
  assert torch.equal(dW.cpu(), want)


@pytest.mark.parametrize('n', [1, 3, 4, 5, 7, 8, 9, 4099])
def test_axpy_and_scale(ops, n):
  """a power-of-two alpha on integer data is exact; an arbitrary alpha gives the one-rounding results fma(alpha, x, out) and
  bf16(fl32(x alpha))"""
  g = torch.Generator().manual_seed(n)
  x = torch.randint(-64, 65, (n,), generator=g).float()
  o = torch.randint(-64, 65, (n,), generator=g).float()
  for alpha in (0.25, -8.0):
    a = torch.tensor(alpha, device='cuda')
    assert torch.equal(ops.axpy_f32_(o.cuda(), x.cuda(), a).cpu(), (o.double() + alpha * x.double()).float())
    stale = torch.full((n,), NAN, device='cuda')
    assert torch.equal(ops.axpy_f32_(stale, x.cuda(), a, accumulate=False).cpu(), (alpha * x.double()).float())
    assert torch.equal(ops.scale_bf16_(x.to(BF16).cuda(), a).cpu(), (alpha * x.to(BF16).double()).to(BF16))
  assert torch.equal(ops.axpy_f32_(o.cuda(), x.cuda()).cpu(), o + x)                         # alpha None = 1
  xr, orr = torch.randn(n, generator=g), torch.randn(n, generator=g)
  a32 = torch.tensor(0.3712345, dtype=F32)
  want = (a32.double() * xr.double() + orr.double()).float()                                   # the product is exact in fp64
  assert torch.equal(ops.axpy_f32_(orr.cuda(), xr.cuda(), a32.cuda()).cpu(), want)
  assert torch.equal(ops.axpy_f32_(torch.full((n,), NAN, device='cuda'), xr.cuda(), a32.cuda(), accumulate=False).cpu(), (a32.double() * xr.double()).float())
  xb = xr.to(BF16)
  assert torch.equal(ops.scale_bf16_(xb.cuda(), a32.cuda()).cpu(), (a32.double() * xb.double()).float().to(BF16))


# ---------------------------------------------------------------------------------------------------------------------
# embedding: the sorted backward bit for bit, the forward exactly
# ---------------------------------------------------------------------------------------------------------------------
# M over the 1024-token blocks of the sort, V over the one-pass / two-pass switch (V < 256) and the 16-bit limit, d over the lane loop's
# second trip (d > 256)
EMBED_CASES = [(1, 1, 4), (7, 3, 4), (7, 3, 260), (1, 65535, 4), (7, 256, 64), (1023, 255, 64), (1024, 256, 4), (1025, 257, 64), (1024, 3, 64),
               (1025, 255, 260), (1025, 256, 260), (1023, 65535, 64), (4097, 1, 4), (4097, 255, 260), (4097, 257, 4), (4097, 65535, 4)]


def _embed_check(ops, ids, dout, V, tag):
  """overwrite over stale NaN, accumulate onto random contents, and a second run: all bit-equal to the sequential fp32 sum"""
  d = dout.shape[1]
  idc, doc = ids.cuda(), dout.cuda()
  dW = torch.full((V, d), NAN, device='cuda')
  assert ops.embed_bwd_sorted(idc, doc, dW, accumulate=False)
  want = PT.embed_bwd_sequential(ids, dout, None, V)
  assert torch.equal(dW.cpu(), want), (tag, 'overwrite')
  dW0 = torch.randn(V, d, generator=torch.Generator().manual_seed(V + d))
  acc = dW0.cuda()
  ops.embed_bwd_sorted(idc, doc, acc, accumulate=True)
  assert torch.equal(acc.cpu(), PT.embed_bwd_sequential(ids, dout, dW0, V)), (tag, 'accumulate')
  again = torch.full((V, d), NAN, device='cuda')
  ops.embed_bwd_sorted(idc, doc, again, accumulate=False)
  assert torch.equal(again, dW), (tag, 'second run')
  return dW0


@pytest.mark.parametrize('M,V,d', EMBED_CASES)
def test_embed_bwd_sorted_bit_exact(ops, M, V, d):
  """unit-normal gradients; id patterns: a quarter of the tokens on one id with ids 0 and V - 1 present and two ids out of range; all
  tokens on one id; all ids out of range (every row 0 when overwriting, untouched when accumulating)"""
  g = torch.Generator().manual_seed(M * 7 + V)
  dout = torch.randn(M, d, generator=g)
  ids = torch.randint(0, V, (M,), generator=g)
  ids[torch.randperm(M, generator=g)[: M // 4]] = ids[0].item()
  if M >= 7:
    ids[1], ids[M - 2], ids[3], ids[M - 1] = 0, V - 1, -1, V
  _embed_check(ops, ids, dout, V, 'quarter')
  _embed_check(ops, torch.full((M,), V - 1, dtype=I64), dout, V, 'all equal')
  oor = torch.where(torch.arange(M) % 2 == 0, -1, V + 5).to(I64)
  dW0 = _embed_check(ops, oor, dout, V, 'all out of range')
  assert bool((PT.embed_bwd_sequential(oor, dout, None, V) == 0).all()) and torch.equal(PT.embed_bwd_sequential(oor, dout, dW0, V), dW0)


def test_embed_bwd_sorted_continues_across_slices(ops):
  """M = 65537: the wrapper's second slice of one token accumulates onto the first; the sequential sum just goes on"""
  g = torch.Generator().manual_seed(65537)
  M, V, d = 65537, 300, 4
  ids = torch.randint(0, V, (M,), generator=g)
  ids[torch.randperm(M, generator=g)[: M // 4]] = 7
  ids[M - 1] = 7
  _embed_check(ops, ids, torch.randn(M, d, generator=g), V, 'two slices')


def test_embed_fwd_exact(ops):
  g = torch.Generator().manual_seed(3)
  V, d = 5, 260
  W = torch.randn(V, d, generator=g)
  ids = torch.tensor([0, V - 1, 2, 2, 0, V - 1, 1], dtype=I64)   # M % 4 != 0
  assert torch.equal(ops.embed_fwd(ids.cuda(), W.cuda()).cpu(), W[ids])


# ---------------------------------------------------------------------------------------------------------------------
# casts on the rounding edges
# ---------------------------------------------------------------------------------------------------------------------
def _edge_values():
  """fp32 values whose low 16 bits are 0x7FFF / 0x8000 / 0x8001 (below, at and above the tie) under even and odd upper halves, both
  signs; the same under the largest finite upper half (rounds to inf from the tie on); +-0, +-inf, the largest finite fp32; quiet NaNs and
  one whose upper half alone reads as inf (0x7F800001: truncating it would make an inf)"""
  bits = []
  for up in (0x3F80, 0x3F81, 0x0080, 0x7F7E, 0x7F7F):
    for low in (0x7FFF, 0x8000, 0x8001, 0x0000, 0xFFFF):
      for sign in (0, 0x80000000):
        bits.append(sign | (up << 16) | low)
  bits += [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF]
  return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def _same_bf16(got, want):
  got, want = got.cpu(), want.cpu()
  nan = torch.isnan(want)
  assert torch.equal(torch.isnan(got), nan)
  assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))   # bits: +-0 told apart


def _as_matrix(vals):
  """the values, repeated up to a multiple of 64, as an [8, 8 k] matrix (the transposing casts take multiples of 8)"""
  size = -(-vals.numel() // 64) * 64
  return vals.repeat(-(-size // vals.numel()))[:size].reshape(8, -1)


def test_casts_on_rounding_edges(ops):
  e = _edge_values()
  want = e.to(BF16)
  _same_bf16(ops.cast_bf16(e.cuda()), want)                       # 60 values: vector body and scalar tail
  _same_bf16(ops.cast_bf16(e[:7].cuda()), want[:7])
  mat = _as_matrix(e)
  y, yt = ops.cast_bf16_t(mat.cuda())
  _same_bf16(y, mat.to(BF16))
  _same_bf16(yt, mat.to(BF16).t().contiguous())
  _same_bf16(ops.scale_bf16_(want.clone().cuda(), torch.tensor(1.0, device='cuda')), want)
  # the shadows of the optimizer tail: signSGD with lr = 0, wd = 0 (decay = 1) on g = 1, m = 0 returns fma(-0, 1, p) = p itself, +-0,
  # inf and NaN included, so dst = bf16(p)
  p = mat.cuda()
  dst = torch.empty(mat.shape, dtype=BF16, device='cuda')
  dst_t = torch.empty(mat.shape[::-1], dtype=BF16, device='cuda')
  ops.optim_cast_multi_(ops.optim_hparams('signSGD', 0.0, 0.0, momentum=0.9), [(p, torch.ones_like(p), torch.zeros_like(p), None, dst, dst_t)])
  _same_bf16(dst, mat.to(BF16))
  _same_bf16(dst_t, mat.to(BF16).t().contiguous())


def test_casts_of_fp32_denormals(ops):
  """what v_cvt_pk_bf16_f32 makes of fp32 denormal inputs is recorded, not fixed: the result is printed, and must be finite with the
  input's sign (profiles/tail_parity.md has the MI355X's answer)"""
  bits = np.array([0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007F8000, 0x007FFFFF, 0x00400000], dtype=np.uint32)
  x = torch.from_numpy(np.concatenate([bits, bits | 0x80000000]).view(np.float32).copy())
  got = ops.cast_bf16(x.cuda()).cpu()
  mat = _as_matrix(x)
  got_t = ops.cast_bf16_t(mat.cuda())[0].cpu().reshape(-1)[:x.numel()]
  ref = x.to(BF16)
  show = lambda t: ' '.join(f'{b & 0xffff:04x}' for b in t.view(torch.int16).tolist())  # noqa: E731
  print(f'denormal fp32 -> bf16: cast_bf16 {show(got)} | cast_bf16_t {show(got_t)} | torch {show(ref)} | equal to torch: {torch.equal(got, ref)}')
  for t in (got, got_t):
    assert bool(torch.isfinite(t.float()).all())
    assert torch.equal(torch.signbit(t.float()), torch.signbit(x))


# ---------------------------------------------------------------------------------------------------------------------
# optimizers: element budget
# ---------------------------------------------------------------------------------------------------------------------
N = 4099
SHAPES = [(8, 8), (72, 136), (200, 40)]
NMULTI = sum(r * c for r, c in SHAPES)


def _buffers(kind, cls, first, n, seed):
  """fp32 CPU (p, g, m, v) as the reference reads them, and what the kernel is handed: NaN in every buffer a first step must not read"""
  p, g, m, v = PT.optim_inputs(cls, n, seed)
  if kind in ('adamw', 'nadamw') and first:
    m, v = torch.zeros_like(m), torch.zeros_like(v)
  km, kv = m, v
  if first and kind in ('sgd', 'signSGD', 'sfo_adamw'):
    km = torch.full_like(m, NAN)
    kv = torch.full_like(v, NAN)
  has_m = kind != 'sgd0'
  has_v = kind in ('adamw', 'nadamw', 'sfo_adamw')
  return (p, g, m if has_m else None, v if has_v else None), (km if has_m else None, kv if has_v else None)


@pytest.mark.parametrize('first', [True, False], ids=['first', 'steady'])
@pytest.mark.parametrize('kind', PT.KINDS)
def test_optimizer_element_budget(ops, kind, first):
  """every class x {no clip, device clip 0.37}: plm_optim_f32 on 4099 elements of a span one element into its buffer, and
  plm_optim_cast_multi on one list of three matrices (its shadows equal to bf16 of the p it wrote)"""
  hp = PT.tail_hparams(kind, first)
  for cls in PT.CLASSES:
    for clip in (None, PT.CLIP):
      cl = None if clip is None else torch.tensor([clip], device='cuda')
      seed = 31 * PT.CLASSES.index(cls) + (7 if clip else 0)
      (p, g, m, v), (km, kv) = _buffers(kind, cls, first, N, seed)
      dp, dg = span(p), span(g)
      dm = None if km is None else span(km)
      dv = None if kv is None else span(kv)
      assert dp.data_ptr() % 16 == 4
      ops.optim_(hp, dp, dg, dm, dv, cl)
      flat = PT.optim_metrics(PT.optim_reference(kind, hp, p, g, m, v, clip), dp, dm, dv)
      (p, g, m, v), (km, kv) = _buffers(kind, cls, first, NMULTI, seed + 1)
      items, o = [], 0
      for r, c in SHAPES:
        cut = lambda t: None if t is None else t[o:o + r * c].reshape(r, c).cuda()  # noqa: E731,B023
        items.append((cut(p), cut(g), cut(km), cut(kv), torch.empty(r, c, dtype=BF16, device='cuda'), torch.empty(c, r, dtype=BF16, device='cuda')))
        o += r * c
      ops.optim_cast_multi_(hp, items, cl)
      cat = lambda i: None if items[0][i] is None else torch.cat([it[i].reshape(-1) for it in items])  # noqa: E731
      multi = PT.optim_metrics(PT.optim_reference(kind, hp, p, g, m, v, clip), cat(0), cat(2), cat(3))
      for it in items:
        assert torch.equal(it[4], it[0].to(BF16)) and torch.equal(it[5], it[0].to(BF16).t())
      met = {k: max(flat[k], multi[k]) for k in flat}
      PT.check(kind, met, f'{kind} {"first" if first else "steady"} {cls} clip={clip}')


@pytest.mark.parametrize('kind', PT.KINDS)
def test_non_finite_gradients_stay_in_their_elements(ops, kind):
  """a NaN and an inf in g: those elements of the outputs are not finite (signSGD's p' of the inf is the finite p decay - lr, the sign
  of +inf being 1: equal to the run on a large finite gradient), every other element is bit-equal to the run without them"""
  hp = PT.tail_hparams(kind, False)
  (p, g, m, v), _ = _buffers(kind, 'randn', False, N, 5)
  i_nan, i_inf = 5, 1000
  gb = g.clone()
  gb[i_nan], gb[i_inf] = NAN, float('inf')
  gc = g.clone()
  gc[i_inf] = 1e30
  runs = []
  for grad in (g, gb, gc if kind == 'signSGD' else g):   # the large finite gradient only where it is compared (elsewhere g^2 would overflow)
    bufs = [span(p), span(grad), None if m is None else span(m), None if v is None else span(v)]
    ops.optim_(hp, *bufs)
    runs.append([None if t is None else t.cpu() for t in (bufs[0], bufs[2], bufs[3])])
  keep = torch.ones(N, dtype=torch.bool)
  keep[i_nan] = keep[i_inf] = False
  for name, clean, bad, big in zip('pmv', *runs):
    if clean is None:
      continue
    assert torch.equal(clean[keep], bad[keep]), (kind, name)
    assert bool(torch.isfinite(clean).all()) and not torch.isfinite(bad[i_nan]), (kind, name)
    if kind == 'signSGD' and name == 'p':
      assert bad[i_inf] == big[i_inf] and torch.isfinite(bad[i_inf])
    else:
      assert not torch.isfinite(bad[i_inf]), (kind, name)


# ---------------------------------------------------------------------------------------------------------------------
# optimizers: exact invariants
# ---------------------------------------------------------------------------------------------------------------------
def _step(ops, hp, p, g, m, v, clip=None):
  """one flat step on offset spans of copies; returns (p', m', v') on the GPU"""
  bufs = [span(p), span(g), None if m is None else span(m), None if v is None else span(v)]
  ops.optim_(hp, *bufs, clip)
  return bufs[0], bufs[2], bufs[3]


def _equal(a, b):
  return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('kind', PT.KINDS)
def test_clip_is_the_gradient_scaled_once(ops, kind):
  """optim_(g, clip = c) is bit-equal to optim_(fl32(g c), no clip): optim_elem forms gi = g * cs first and reads g nowhere else"""
  (p, g, m, v), _ = _buffers(kind, 'mixed', False, N, 9)
  for first in (True, False):
    hp = PT.tail_hparams(kind, first)
    c = torch.tensor([0.37123], device='cuda')
    a = _step(ops, hp, p, g, m, v, c)
    b = _step(ops, hp, p, (g.cuda() * c).cpu(), m, v)
    assert _equal(a, b), (kind, first)


def test_power_of_two_scaling_with_eps_zero(ops):
  """eps = 0, g != 0.  AdamW / NAdamW: (g, m, v) -> (4 g, 4 m, 16 v) multiplies every term of m' by 4 and of v' by 16 exactly (powers of
  two commute with every rounding), sqrt(16 v') = 4 sqrt(v'), so d scales by 4 and m' / d, g / d and with them p' keep their bits.
  sfo_adamw with weight_decay = 0: (g, v) -> (4 g, 16 v) keeps gn = g / d, hence z' = z - lr gn and y' bit for bit (z is not scaled),
  v' scales by 16.  signSGD: (g, m) -> (8 g, 8 m) scales m' by 8 and keeps its sign, hence p'."""
  (p, g, m, v), _ = _buffers('adamw', 'randn', False, N, 13)
  assert bool((g != 0).all())
  for kind in ('adamw', 'nadamw'):
    hp = PT.tail_hparams(kind, False, eps=0.0)
    a, b = _step(ops, hp, p, g, m, v), _step(ops, hp, p, 4 * g, 4 * m, 16 * v)
    assert torch.equal(a[0], b[0]) and torch.equal(4 * a[1], b[1]) and torch.equal(16 * a[2], b[2]), kind
  hp = PT.tail_hparams('sfo_adamw', False, eps=0.0, wd=0.0)
  a, b = _step(ops, hp, p, g, m, v), _step(ops, hp, p, 4 * g, m, 16 * v)
  assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(16 * a[2], b[2])
  hp = PT.tail_hparams('signSGD', False)
  a, b = _step(ops, hp, p, g, m, None), _step(ops, hp, p, 8 * g, 8 * m, None)
  assert torch.equal(a[0], b[0]) and torch.equal(8 * a[1], b[1])


def test_zero_gradient_first_step(ops):
  """AdamW's first step on g = 0: m' = v' = 0 and p' = fl32(p decay) exactly (0 / eps = 0, and -coef * 0 adds nothing);
  SGD with weight_decay = 0: p' = p"""
  (p, g, m, v), _ = _buffers('adamw', 'zero_g0', True, N, 21)
  hp = PT.tail_hparams('adamw', True)
  a = _step(ops, hp, p, g, m, v)
  decay = torch.tensor(PT.fields(hp)['decay'], dtype=F32)
  assert float(decay) == PT.fields(hp)['decay']
  assert torch.equal(a[0].cpu(), p * decay) and bool((a[1] == 0).all()) and bool((a[2] == 0).all())
  for kind in ('sgd', 'sgd0'):
    hs = PT.tail_hparams(kind, True, wd=0.0)
    b = _step(ops, hs, p, g, None if kind == 'sgd0' else torch.full_like(p, NAN), None)
    assert torch.equal(b[0].cpu(), p), kind


def test_lerp_end_points(ops):
  p, _, z, _ = PT.optim_inputs('mixed', N, 4)
  assert torch.equal(ops.lerp_(span(p), span(z), 0.0).cpu(), p)
  assert torch.equal(ops.lerp_(span(p), span(z), 1.0).cpu(), z)


# ---------------------------------------------------------------------------------------------------------------------
# the second trip of the flat kernels' grid-stride loops (grids capped at 2^20 blocks of 256)
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_stride_second_trip(ops):
  """n = 2^28 + 257.  SGD without momentum, wd = 0, lr = 2^-3: p' = fl32(p - g / 8) (the product is exact: one rounding on both
  sides); lerp_ with w = 0.5: z - (z - p) 0.5.  Two fp32 buffers of 1.07 GB and torch's temporaries; compared on the GPU."""
  n = (1 << 28) + 257
  gen = torch.Generator(device='cuda').manual_seed(28)
  p = torch.randn(n, device='cuda', generator=gen)
  g = torch.randn(n, device='cuda', generator=gen)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  want = p - g * 0.125
  ops.optim_(ops.optim_hparams('sgd', 0.125, 0.0), p, g, None, None)
  ok = torch.equal(p, want)
  torch.cuda.synchronize()
  t1 = time.perf_counter()
  want = g - (g - p) * 0.5
  ops.lerp_(p, g, 0.5)
  ok2 = torch.equal(p, want)
  torch.cuda.synchronize()
  t2 = time.perf_counter()
  print(f'grid-stride second trip: sgd {t1 - t0:.4f} s, lerp {t2 - t1:.4f} s (after {n} x 2 random values)')
  assert ok and ok2, (ok, ok2)
