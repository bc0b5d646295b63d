"""Dense, bit-packed attention masks on MI355X (csrc/attn_masked.hip): the pack kernel against numpy, the masked forward / backward against a
float64 masked softmax on the exact bf16 operands (oracle/parity.py's bounds), empty rows, agreement with the causal and document-mask families,
determinism, the C ABI's argument checks, and the model API (DenseMask, attn_mask_mode: 'dense') against the fp32 oracle."""

import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity as PB  # noqa: E402

LOSS_RTOL = 1e-4
PLM_E_INVALID = -1


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


def bf(x):
  return x.to(torch.bfloat16)


def relerr(a, ref):
  a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
  return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def close(a, ref, tol, what=''):
  e = relerr(a, ref)
  assert e <= tol, f'{what}: rel-to-max error {e:.3e} > {tol:.1e}'
  return e


# --------------------------------------------------------------------------------------
# masks (bool [B, T, T], True = may attend)
# --------------------------------------------------------------------------------------
def _ij(T):
  return torch.arange(T).view(T, 1), torch.arange(T).view(1, T)


def causal_mask(B, T):
  return torch.ones(T, T, dtype=torch.bool).tril().expand(B, T, T).clone()


def window_mask(B, T, w):
  i, j = _ij(T)
  return ((j <= i) & (j > i - w)).expand(B, T, T).clone()


def prefix_mask(B, T, p):
  i, j = _ij(T)
  return ((j <= i) | (j < p)).expand(B, T, T).clone()


def doc_mask(B, T, seed):
  rng = np.random.default_rng(seed)
  docs = []
  for _ in range(B):
    lens, tot = [], 0
    while tot < T + 1:
      n = int(min(rng.integers(1, max(2, T // 3)), T + 1 - tot))
      lens.append(n)
      tot += n
    docs.append(lens)
  ds = O.doc_start_from_lengths(docs, T)
  return O.mask_from_doc_start(ds), ds


def make_mask(kind, B, T, seed):
  g = torch.Generator().manual_seed(seed)
  if kind == 'causal':
    return causal_mask(B, T)
  if kind == 'docs':
    return doc_mask(B, T, seed)[0]
  if kind.startswith('window'):
    return window_mask(B, T, int(kind[6:]))
  if kind.startswith('prefix'):
    p = kind[6:]
    return prefix_mask(B, T, T // 2 if p == 'half' else int(p))
  if kind == 'full':
    return torch.ones(B, T, T, dtype=torch.bool)
  if kind.startswith('bern'):
    return torch.rand(B, T, T, generator=g) < float(kind[4:])
  if kind == 'empty_rows':
    m = torch.rand(B, T, T, generator=g) < 0.5
    m[:, ::7] = False
    m[0, :min(T, 40)] = False  # a run of empty rows across a wave
    return m
  if kind == 'empty_tiles':
    m = torch.rand(B, T, T, generator=g) < 0.9
    m[:, :128, 64:128] = False  # whole 128 x 64 tiles with no bit
    m[:, 128:, :64] = False
    return m
  if kind == 'single_key':
    m = torch.zeros(B, T, T, dtype=torch.bool)
    j = torch.randint(0, T, (B, T), generator=g)
    m.scatter_(2, j.unsqueeze(-1), True)
    return m
  raise ValueError(kind)


MASKS = ['causal', 'docs', 'window1', 'window64', 'window200', 'prefix0', 'prefix37', 'prefixhalf', 'full', 'bern0.05', 'bern0.5', 'bern0.95',
         'empty_rows', 'empty_tiles', 'single_key']
SHAPES = [(1, 256, 2), (2, 200, 3), (3, 132, 1), (2, 384, 2)]  # (B, T, nh): ragged tiles, 1-3 sequences and heads


# --------------------------------------------------------------------------------------
# packing and references
# --------------------------------------------------------------------------------------
def numpy_pack(mask):
  """bool [M, T, T] -> (uint64 [M, T, W], uint8 [M, NQT, W]) as plm_attn_mask_pack defines them."""
  m = mask.numpy()
  M, T, _ = m.shape
  W, NQT = (T + 63) // 64, (T + 127) // 128
  padded = np.zeros((M, T, W * 64), dtype=bool)
  padded[:, :, :T] = m
  bits = np.packbits(padded.reshape(M, T, W, 64), axis=-1, bitorder='little').view('<u8').reshape(M, T, W)
  cls = np.zeros((M, NQT, W), dtype=np.uint8)
  for qt in range(NQT):
    for jt in range(W):
      blk = m[:, qt * 128:(qt + 1) * 128, jt * 64:(jt + 1) * 64]
      cls[:, qt, jt] = np.where(blk.all(axis=(1, 2)), 1, np.where(blk.any(axis=(1, 2)), 2, 0))
  return bits, cls


def masked_reference(qkv_rot, dout, mask, B, T, nh, hd, out_kernel, rope):
  """float64 masked softmax attention on the exact bf16 rotated operands; rows with no allowed key give 0 (torch's SDPA).  Gradients by
  the closed form (dS = P (dP - rowsum(P dP))), dQ / dK taken back through the inverse rotation as the kernels return them."""
  q, k, v = PB.split_qkv(qkv_rot, B, T, nh, hd)
  do = PB.heads(dout, B, T, nh, hd)
  allow = mask.view(mask.shape[0], 1, T, T).expand(B, nh, T, T)
  s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(hd)
  s = s.masked_fill(~allow, float('-inf'))
  mx = s.amax(-1, keepdim=True)
  empty = torch.isinf(mx) & (mx < 0)
  mx = torch.where(empty, torch.zeros_like(mx), mx)
  e = torch.exp(s - mx)
  l = e.sum(-1, keepdim=True)
  p = torch.where(empty, torch.zeros_like(e), e / torch.where(empty, torch.ones_like(l), l))
  o = torch.matmul(p, v)
  dp = torch.matmul(do, v.transpose(-1, -2))
  ds = p * (dp - (p * dp).sum(-1, keepdim=True))
  ref = {'out': o, 'dq': torch.matmul(ds, k) / math.sqrt(hd), 'dk': torch.matmul(ds.transpose(-1, -2), q) / math.sqrt(hd),
         'dv': torch.matmul(p.transpose(-1, -2), do)}
  ref['lse'] = torch.where(empty, torch.zeros_like(mx), (mx + torch.log(l)) * PB.LOG2E).squeeze(-1)
  ref['delta'], ref['delta_abs'] = PB.delta_reference(PB.heads(out_kernel, B, T, nh, hd), do)
  ref['dq'], ref['dk'] = (PB.rope64(ref[n], rope[0], rope[1], -1.0) for n in ('dq', 'dk'))
  return ref, empty.squeeze(-1)


def run_masked(ops, qkv, dout, mask_dev, B, T, nh, return_delta=True):
  hd = qkv.shape[1] // (3 * nh)
  cos, sin = (t.cuda() for t in O.rope_table(hd, T))
  qrot = ops.rope_qk_(qkv.cuda(), cos, sin, B, T, nh)
  bits, cls = ops.attn_mask_pack(mask_dev)
  out, lse = ops.attn_fwd_masked(qrot, bits, cls, B, T, nh)
  dqkv, delta = ops.attn_bwd_masked(qrot, out, dout.cuda(), lse, cos, sin, bits, cls, B, T, nh, return_delta=True)
  return qrot, out, lse, dqkv, delta, (cos, sin)


# --------------------------------------------------------------------------------------
# pack kernel
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [4, 68, 200, 1000])
@pytest.mark.parametrize('shared', [False, True])
def test_pack_matches_numpy(ops, T, shared):
  """plm_attn_mask_pack bit for bit against numpy: bit j % 64 of word (m, i, j // 64) is mask[m, i, j], bits past T are 0, and the class of
  every 128 x 64 tile (0 empty, 1 every in-range bit, 2 mixed); [B, T, T] masks and one [T, T] mask for all sequences."""
  B = 1 if shared else 3
  g = torch.Generator().manual_seed(T + shared)
  m = torch.rand(B, T, T, generator=g) < 0.5
  m[-1, :min(T, 128), -4:] = False  # class-0 tiles on the ragged edge
  m[0, :, :min(T, 64)] = True       # class-1 tiles
  if T >= 200:
    m[:, 128:, 64:128] = True
    m[:, :128, 128:192] = False
  bits, cls = ops.attn_mask_pack((m[0] if shared else m).cuda())
  rb, rc = numpy_pack(m[:1] if shared else m)
  assert bits.shape == rb.shape and cls.shape == rc.shape
  assert np.array_equal(bits.cpu().numpy().view('<u8'), rb)
  assert np.array_equal(cls.cpu().numpy(), rc)
  assert set(np.unique(rc).tolist()) >= ({0, 1, 2} if T >= 200 else {1})


# --------------------------------------------------------------------------------------
# kernels vs fp64
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize('hd', [32, 64, 128])
@pytest.mark.parametrize('kind', MASKS)
def test_masked_attention_vs_fp64(ops, hd, kind):
  """out, LSE, delta and dQ / dK / dV against the float64 masked softmax, judged with oracle/parity.py's bounds (row-local, projection, LSE in
  log2 units, delta relative to rowsum |dO * O|).  Rows with no allowed key: out and every gradient exactly 0, LSE +inf, nothing NaN."""
  B, T, nh = SHAPES[(MASKS.index(kind) + hd // 32) % len(SHAPES)]
  seed = hd * 1000 + MASKS.index(kind)
  g = torch.Generator().manual_seed(seed)
  d = nh * hd
  qkv = bf(torch.randn(B * T, 3 * d, generator=g))
  dout = bf(torch.randn(B * T, d, generator=g))
  mask = make_mask(kind, B, T, seed)
  qrot, out, lse, dqkv, delta, rope = run_masked(ops, qkv, dout, mask.cuda(), B, T, nh)
  for t in (out, dqkv, delta):
    assert torch.isfinite(t.float()).all(), kind
  ref, empty = masked_reference(qrot, dout, mask, B, T, nh, hd, out, tuple(t.cpu() for t in rope))
  got = PB.kernel_result(B, T, nh, hd, out, lse, dqkv, delta)
  if empty.any():
    assert torch.isposinf(got['lse'][empty]).all()
    assert (got['out'][empty] == 0).all() and (got['dq'][empty] == 0).all() and (got['delta'][empty] == 0).all()
    got['lse'] = torch.where(empty, torch.zeros_like(got['lse']), got['lse'])
  assert torch.isfinite(got['lse']).all()
  PB.check(got, ref, f'masked {kind} hd {hd} B={B} T={T} nh={nh}')


def test_empty_rows_give_exact_zeros(ops):
  """torch's SDPA returns 0 (and 0 gradients) for a row with no allowed key.  Empty rows in every position of a tile, a whole empty query
  tile, and keys that no query sees: out, dQ, and the rows' contributions to dK / dV are exactly 0; no NaN / inf in out, dqkv or delta."""
  B, T, nh, hd = 2, 256, 2, 64
  g = torch.Generator().manual_seed(5)
  d = nh * hd
  qkv = bf(torch.randn(B * T, 3 * d, generator=g))
  dout = bf(torch.randn(B * T, d, generator=g))
  mask = torch.rand(B, T, T, generator=g) < 0.3
  mask[:, ::3] = False
  mask[1, 128:] = False         # a whole empty query tile
  mask[:, :, 200:] = False      # keys nobody sees
  _, out, lse, dqkv, delta, _ = run_masked(ops, qkv, dout, mask.cuda(), B, T, nh)
  for t in (out, dqkv, delta):
    assert torch.isfinite(t.float()).all()
  empty = ~mask.any(-1)  # [B, T]
  rows = empty.reshape(B * T).cuda()
  assert (out[rows] == 0).all() and (dqkv[rows, :d] == 0).all()
  assert (delta.transpose(1, 2)[empty.cuda()] == 0).all()
  assert torch.isposinf(lse.transpose(1, 2)[empty.cuda()]).all()
  unseen = (~mask.any(1)).reshape(B * T).cuda()  # keys no query sees: dK = dV = 0
  assert (dqkv[unseen, d:] == 0).all()
  # an all-False mask: everything is 0
  _, out0, lse0, dqkv0, delta0, _ = run_masked(ops, qkv, dout, torch.zeros(B, T, T, dtype=torch.bool).cuda(), B, T, nh)
  assert (out0 == 0).all() and (dqkv0 == 0).all() and (delta0 == 0).all() and torch.isposinf(lse0).all()


@pytest.mark.parametrize('hd', [32, 64, 128])
def test_dense_mask_agrees_with_the_causal_and_document_families(ops, hd):
  """A causal mask and a block-diagonal document mask given as dense masks against the causal kernels and the doc_start kernels, with the
  tolerance test_kernels_gpu.py uses between families (out 8e-3; gradients 2e-2 rel-to-max); a [T, T] mask shared by the batch gives the same
  bits as the same mask repeated per sequence."""
  B, T, nh = 2, 320, 2
  g = torch.Generator().manual_seed(hd)
  d = nh * hd
  qkv = bf(torch.randn(B * T, 3 * d, generator=g))
  dout = bf(torch.randn(B * T, d, generator=g)).cuda()
  cos, sin = (t.cuda() for t in O.rope_table(hd, T))
  qrot = ops.rope_qk_(qkv.cuda(), cos, sin, B, T, nh)
  dmask, ds = doc_mask(B, T, 7 + hd)
  for dense, doc in ((causal_mask(B, T), None), (dmask, ds.cuda())):
    bits, cls = ops.attn_mask_pack(dense.cuda())
    out, lse = ops.attn_fwd_masked(qrot, bits, cls, B, T, nh)
    dqkv = ops.attn_bwd_masked(qrot, out, dout, lse, cos, sin, bits, cls, B, T, nh)
    out_f, lse_f = ops.attn_fwd(qrot, B, T, nh, doc)
    dqkv_f = ops.attn_bwd(qrot, out_f, dout, lse_f, cos, sin, B, T, nh, doc)
    tag = 'causal' if doc is None else 'documents'
    close(out.float(), out_f.float(), 8e-3, f'{tag} as a dense mask vs its own family (out, hd {hd})')
    for name, a, b in zip('qkv', dqkv.split(d, dim=1), dqkv_f.split(d, dim=1)):
      close(a.float(), b.float(), 2e-2, f'{tag} as a dense mask vs its own family (d{name}, hd {hd})')
  shared = causal_mask(1, T)[0].cuda()
  bits1, cls1 = ops.attn_mask_pack(shared)
  bitsB, clsB = ops.attn_mask_pack(causal_mask(B, T).cuda())
  o1, l1 = ops.attn_fwd_masked(qrot, bits1, cls1, B, T, nh)
  oB, lB = ops.attn_fwd_masked(qrot, bitsB, clsB, B, T, nh)
  assert torch.equal(o1, oB) and torch.equal(l1, lB)
  assert torch.equal(ops.attn_bwd_masked(qrot, o1, dout, l1, cos, sin, bits1, cls1, B, T, nh),
                     ops.attn_bwd_masked(qrot, oB, dout, lB, cos, sin, bitsB, clsB, B, T, nh))


@pytest.mark.parametrize('hd', [32, 64, 128])
def test_masked_attention_is_deterministic(ops, hd):
  """No atomics on outputs: two runs of pack, forward and backward give the same bits."""
  B, T, nh = 2, 520, 2
  g = torch.Generator().manual_seed(hd + 1)
  d = nh * hd
  qkv = bf(torch.randn(B * T, 3 * d, generator=g))
  dout = bf(torch.randn(B * T, d, generator=g))
  mask = (torch.rand(B, T, T, generator=g) < 0.4).cuda()
  a = run_masked(ops, qkv, dout, mask, B, T, nh)
  b = run_masked(ops, qkv, dout, mask, B, T, nh)
  for x, y in zip(a[1:5], b[1:5]):
    assert torch.equal(x, y)


def test_masked_entry_points_refuse_bad_arguments(ops):
  """NULL pointers, an unsupported head dim, T <= 0, a batch_stride other than 0 / 1 and storage that is not 16-byte aligned give
  PLM_E_INVALID before anything is launched (the outputs keep their sentinel values)."""
  from plainlm_amd import _lib
  lib = _lib.load()
  B, T, nh, hd = 1, 128, 1, 64
  st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
  null = C.c_void_p(0)
  mask = torch.ones(B, T, T, dtype=torch.bool, device='cuda')
  buf = torch.full((lib.plm_attn_mask_bytes(B, T) + 64,), 7, dtype=torch.uint8, device='cuda')
  nb = B * T * 2 * 8
  bits, cls = p(buf), p(buf, nb)
  assert lib.plm_attn_mask_bytes(B, 0) == 0 and lib.plm_attn_mask_bytes(0, T) == 0

  def untouched():
    torch.cuda.synchronize()
    return bool((buf == 7).all())

  for args in ((null, 1, bits, cls, B, T), (p(mask), 1, null, cls, B, T), (p(mask), 1, bits, null, B, T), (p(mask), 1, p(buf, 8), cls, B, T),
               (p(mask), 1, bits, p(buf, nb + 4), B, T), (p(mask), 1, bits, cls, B, 0), (p(mask), 1, bits, cls, 0, T), (p(mask), 2, bits, cls, B, T),
               (p(mask), 1, bits, cls, B, 6)):
    assert lib.plm_attn_mask_pack(*args, st) == PLM_E_INVALID, args
  assert untouched()
  assert lib.plm_attn_mask_pack(p(mask), 1, bits, cls, B, T, st) == 0
  torch.cuda.synchronize()
  d = nh * hd
  qkv = torch.zeros(B * T, 3 * d + 8, dtype=torch.bfloat16, device='cuda')
  out = torch.full((B * T, d + 8), 3.0, dtype=torch.bfloat16, device='cuda')
  lse = torch.full((B, nh, T), 5.0, device='cuda')
  dout = torch.zeros(B * T, d, dtype=torch.bfloat16, device='cuda')
  dqkv = torch.full((B * T, 3 * d + 8), 3.0, dtype=torch.bfloat16, device='cuda')
  delta = torch.full((B, nh, T), 5.0, device='cuda')
  cos, sin = (t.cuda() for t in O.rope_table(hd, T))

  def clean():
    torch.cuda.synchronize()
    return bool((out == 3).all() and (lse == 5).all() and (dqkv == 3).all() and (delta == 5).all())

  fwd = lambda q=p(qkv), b=bits, c=cls, bs=1, o=p(out), l=p(lse), T_=T, h=hd: lib.plm_attn_fwd_masked(q, b, c, bs, o, l, B, T_, nh, h, st)
  for kw in (dict(q=null), dict(b=null), dict(c=null), dict(o=null), dict(l=null), dict(h=48), dict(h=256), dict(T_=0), dict(T_=-4), dict(bs=3),
             dict(q=p(qkv, 2)), dict(o=p(out, 8)), dict(b=p(buf, 8)), dict(c=p(buf, nb + 1))):
    assert fwd(**kw) == PLM_E_INVALID, kw
  assert clean()

  def bwd(q=p(qkv), o=p(out), do=p(dout), l=p(lse), rc=p(cos), rs=p(sin), b=bits, c=cls, bs=1, dq=p(dqkv), de=p(delta), T_=T, h=hd):
    return lib.plm_attn_bwd_masked(q, o, do, l, rc, rs, b, c, bs, dq, de, B, T_, nh, h, st)
  for kw in (dict(q=null), dict(o=null), dict(do=null), dict(l=null), dict(rc=null), dict(rs=null), dict(b=null), dict(c=null), dict(dq=null),
             dict(de=null), dict(h=16), dict(T_=0), dict(bs=-1), dict(dq=p(dqkv, 2)), dict(do=p(dout, 4)), dict(rc=p(cos, 4)), dict(b=p(buf, 4))):
    assert bwd(**kw) == PLM_E_INVALID, kw
  assert clean()


# --------------------------------------------------------------------------------------
# model API
# --------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def P():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  import plainlm_amd
  return plainlm_amd


def relmax(a, ref):
  a, ref = a.double().cpu(), ref.double().cpu()
  return ((a - ref).abs().max() / ref.abs().max()).item()


def _oracle_with_mask(monkeypatch, mask):
  """The test's copy of the fp32 oracle with its attention honouring ``mask`` (bool [B, T, T]) instead of causal / doc_start."""
  def attention(q, k, v, doc_start=None):
    B, T, nh, hd = q.shape
    qh, kh, vh = (t.transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(hd)
    s = s.masked_fill(~mask.view(mask.shape[0], 1, T, T), float('-inf'))
    o = torch.matmul(torch.softmax(s, dim=-1), vh)
    return o.transpose(1, 2).reshape(B, T, nh * hd)
  monkeypatch.setattr(O, 'attention', attention)


MODEL_MASKS = {'prefix': lambda B, T: prefix_mask(B, T, 45), 'window': lambda B, T: window_mask(B, T, 24)}


@pytest.mark.parametrize('nh', [2, 1])  # d = 128: head dims 64 and 128
@pytest.mark.parametrize('kind', sorted(MODEL_MASKS))
@pytest.mark.parametrize('how', ['DenseMask', 'mode'])
def test_model_dense_mask_vs_oracle(P, monkeypatch, nh, kind, how):
  """A 2-layer model with a prefix-LM and a sliding-window mask, given as functional.DenseMask and as a plain bool mask under
  attn_mask_mode: 'dense': logits, loss and all 15 parameter gradients against the fp32 oracle whose attention honours the same mask."""
  from plainlm_amd import functional as Fn
  B, T, V = 2, 128, 512
  ocfg = O.OracleConfig(vocab_size=V, seq_len=T, dim=128, n_layers=2, n_heads=nh)
  w = O.init_params(ocfg, seed=31 + nh)
  rng = np.random.default_rng(nh + len(kind))
  tok = torch.from_numpy(rng.integers(0, V, size=(B, T + 1)))
  ids, tgt = tok[:, :T], tok[:, 1:].contiguous()
  mask = MODEL_MASKS[kind](B, T)
  m = P.Transformer(P.ModelConfig(vocab_size=V, seq_len=T, dim=128, expand=8 / 3, n_layers=2, n_heads=nh, mlp='glu',
                                  attn_mask_mode='dense' if how == 'mode' else 'doc'))
  m.load_state_dict(w)
  m = m.cuda()
  am = Fn.DenseMask(mask.cuda(), nh) if how == 'DenseMask' else mask.cuda()
  logits = m(ids.cuda(), am)
  loss = m.loss(ids.cuda(), tgt.cuda(), am)
  loss.backward()
  _oracle_with_mask(monkeypatch, mask)
  olog = O.forward(w, ocfg, ids)
  oloss, og = O.loss_and_grads(w, ocfg, ids, tgt)
  assert relmax(logits.float(), olog) < 2e-2
  assert abs(loss.item() - oloss.item()) <= LOSS_RTOL * abs(oloss.item()), (loss.item(), oloss.item())
  worst = {n: relmax(p.grad.float().cpu(), og[n]) for n, p in m.named_parameters()}
  assert len(worst) == 15 and max(worst.values()) < 4e-2, worst


def test_reference_style_loss_path_with_a_dense_mask(P, monkeypatch):
  """engine/engine.py:109-112 as written, under attn_mask_mode: 'dense' built by construct_model: model(inputs, mask) -> torch
  CrossEntropyLoss -> backward, with a prefix-LM mask, against the oracle."""
  from types import SimpleNamespace
  B, T, V, nh = 2, 128, 512, 2
  cfg = SimpleNamespace(model='transformer', vocab_size=V, d_model=128, expand='8/3', n_layers=2, n_heads=nh, mlp_class='glu', seq_len=T,
                        tie_embeddings=False, attn_mask_mode='dense')
  m, mcfg = P.construct_model(cfg)
  assert mcfg.attn_mask_mode == 'dense'
  ocfg = O.OracleConfig(vocab_size=V, seq_len=T, dim=128, n_layers=2, n_heads=nh)
  w = O.init_params(ocfg, seed=5)
  m.load_state_dict(w)
  m = m.cuda()
  tok = torch.from_numpy(np.random.default_rng(9).integers(0, V, size=(B, T + 1)))
  ids, tgt = tok[:, :T], tok[:, 1:].contiguous()
  mask = prefix_mask(B, T, 64)
  logits = m(ids.cuda(), mask.cuda())
  loss = torch.nn.CrossEntropyLoss()(logits.float().view(-1, V), tgt.reshape(-1).cuda())
  loss.backward()
  _oracle_with_mask(monkeypatch, mask)
  oloss, og = O.loss_and_grads(w, ocfg, ids, tgt)
  assert abs(loss.item() - oloss.item()) <= LOSS_RTOL * abs(oloss.item()), (loss.item(), oloss.item())
  for n, p in m.named_parameters():
    assert relmax(p.grad, og[n]) < 4e-2, n


def test_default_mode_still_refuses_a_non_block_diagonal_mask(P):
  """attn_mask_mode 'doc' (the default) keeps today's behaviour: a bool mask that is not block-diagonal causal is refused with the existing
  error at the next conversion; the error now points at the dense mode."""
  B, T = 2, 64
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=T, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu')).cuda()
  ids = torch.randint(0, 256, (B, T)).cuda()
  P.Transformer._mask_status = None
  m(ids, prefix_mask(B, T, 20).cuda())  # queries of the prefix see keys after them: not expressible as doc_start
  with pytest.raises(ValueError, match='block-diagonal') as e:
    P.Transformer.check_mask_status()
  assert 'dense' in str(e.value)
  with pytest.raises(ValueError):
    from plainlm_amd import functional as Fn
    m(ids, Fn.DenseMask(window_mask(B, 2 * T, 16).cuda(), 2))  # a DenseMask of another T
