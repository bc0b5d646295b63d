"""Where the launches over the FP8 KV cache read and write, on a real MI355X: the footprint cases of the plm_kv8_* / *_kv8 entry points
(DESIGN.md section 20).  Same machinery as tests/test_footprint_gpu.py (tests/footprint.py: every buffer between margins, two runs that
differ in one fill byte; W / I / C+R / U are bit equality): a padded cache row stride (the four bytes between a row's payload and its
16-byte multiple are nobody's), ragged chunks, one sequence outside the cache, rows at and beyond the valid length marked unread, the
status word written only on refusal, workspaces of exactly the queried size.  That file's completeness test counts these rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
import kv8_ref as R  # noqa: E402
from footprint import L, P, call  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8
CASES = {}      # id -> (entry points covered, case function)
NH, HD, TMAX, HIDDEN = 3, 32, 37, 288
D = NH * HD
RB = R.row_bytes(D)          # 208: 192 codes, 12 scale bytes, 4 bytes of padding
USED = 2 * D + D // 8        # the bytes of a row that hold something
LD8 = RB + 16
EPS = 1e-6
KINDS = {'glu': 0, 'silu': 1, 'relu_sq': 2}
CHUNKS = {  # tag -> (B, n, lens0, n_new or None): test_footprint_extend_fused_gpu.py's
  'ragged-B5-n3': (5, 3, (0, 34, 17, 36, 20), (3, 3, 0, 1, 7)),
  'refused-B5-n3': (5, 3, (0, 35, 17, 1, 20), None),
  'ragged-B4-n8': (4, 8, (0, 29, 17, 36), (8, 8, 0, 1)),
  'decode-B5-n1': (5, 1, (36, 0, TMAX, 5, 20), None),
}


def rnd(seed, *shape, dtype=F32, scale=1.0):
  return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _rope(T):
  from oracle import cpu_ref as O
  return O.rope_table(HD, T)


def cache_rows(seed, B):
  """A valid cache: kv8_ref's rows of random bf16 k | v, uint8 [B * TMAX, RB]."""
  return R.pack_rows(rnd(seed, B * TMAX, 2 * D, dtype=BF16))


def row_mask(rows):
  """rows bool [B * TMAX] -> the bytes those rows hold, bool [B * TMAX, RB]: codes and scales, not the row's padding."""
  m = torch.zeros(rows.shape[0], RB, dtype=torch.bool)
  m[:, :USED] = rows[:, None]
  return m


def _chunk(ar, B, n, lens0, n_new):
  """(lens0, n_new or None, the appended rows, the rows at and beyond lens0 + c_b, status) of one chunk; the row sets are bool [B * TMAX]."""
  counts = [n] * B if n_new is None else [min(max(c, 0), n) for c in n_new]
  refused = [b for b in range(B) if lens0[b] < 0 or lens0[b] + counts[b] > TMAX]
  l0 = ar.inp('lens0', torch.tensor(lens0, dtype=I32), index_margin=(0, TMAX - n))
  nn = None if n_new is None else ar.inp('n_new', torch.tensor(n_new, dtype=I32), index_margin=(0, 1))
  appended = torch.zeros(B * TMAX, dtype=torch.bool)
  beyond = torch.ones(B * TMAX, dtype=torch.bool)
  for b in range(B):
    if b not in refused:
      appended[b * TMAX + lens0[b]:b * TMAX + lens0[b] + counts[b]] = True
    beyond[b * TMAX:b * TMAX + min(lens0[b] + counts[b], TMAX)] = False
  st = torch.tensor([bool(refused)])  # the caller-zeroed status word: written (to 1, under both fills) only when a sequence is refused
  status = ar.inout('status', torch.zeros(1, dtype=I32), written=st, untouched=~st)
  return l0, nn, appended, beyond, status


def _append_only(ar, seed, B, appended):
  """The cache of a launch that appends and reads nothing: the appended rows' bytes are written, every other byte stays."""
  w = row_mask(appended)
  return ar.inout('kv8', cache_rows(seed, B), ld=LD8, written=w, untouched=~w, unread=torch.ones(B * TMAX, RB, dtype=torch.bool))


def _read_cache(ar, seed, B, beyond):
  """The cache of a launch that only attends: rows at and beyond the valid length hold the fill and are never read; nothing is written."""
  everything = torch.ones(B * TMAX, RB, dtype=torch.bool)
  u = everything & beyond[:, None]
  return ar.inout('kv8', cache_rows(seed, B), ld=LD8, written=torch.zeros_like(everything), untouched=u, unread=u)


def _quant_cases():
  B, T = 3, 21
  rows = torch.zeros(B * TMAX, dtype=torch.bool)
  for b in range(B):
    rows[b * TMAX:b * TMAX + T] = True

  def quant(ar):
    src = ar.inp('src', rnd(501, B * T, 2 * D, dtype=BF16), ld=3 * D, misalign=True)  # the k | v columns of a wider row
    kv8 = _append_only(ar, 502, B, rows)
    return lambda: call('plm_kv8_quant_rows', P(src), 3 * D, P(kv8), LD8, B, T, TMAX, NH, HD)
  CASES['kv8_quant_rows'] = (('plm_kv8_quant_rows',), quant)

  def dequant(ar):
    kv8 = _read_cache(ar, 503, B, ~rows)
    dst = ar.out('dst', BF16, B * T, 2 * D, ld=2 * D + 8, misalign=True)
    return lambda: call('plm_kv8_dequant_rows', P(kv8), LD8, P(dst), 2 * D + 8, B, T, TMAX, NH, HD)
  CASES['kv8_dequant_rows'] = (('plm_kv8_dequant_rows',), dequant)


def _append_cases():
  for tag, (B, n, lens0, n_new) in CHUNKS.items():
    def fn(ar, B=B, n=n, lens0=lens0, n_new=n_new):
      ld_qkv = 3 * D + 8
      qkv = ar.inp('qkv', rnd(511, B * n, 3 * D, dtype=BF16), ld=ld_qkv, misalign=True)
      l0, nn, appended, _, status = _chunk(ar, B, n, lens0, n_new)
      cos, sin = _rope(TMAX)
      rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
      q_out = ar.out('q_out', BF16, B * n, D)  # wholly written: rotated q, or zeros
      kv8 = _append_only(ar, 512, B, appended)
      return lambda: call('plm_kv8_append_rope_rows', P(qkv), ld_qkv, P(l0), P(nn), P(rc), P(rs), TMAX, P(q_out), P(kv8), LD8, P(status), B, n,
                          TMAX, NH, HD)
    CASES[f'kv8_append_rope_rows-{tag}'] = (('plm_kv8_append_rope_rows',), fn)


def _attend_cases():
  B = 5
  lens = (TMAX, 1, 0, 36, 13)
  beyond = torch.ones(B * TMAX, dtype=torch.bool)
  for b, n in enumerate(lens):
    beyond[b * TMAX:b * TMAX + n] = False
  for splits, want_lse in ((7, 1), (0, 0), (64, 1), (1, 0)):
    def fn(ar, splits=splits, want_lse=want_lse):
      nbytes = int(L().plm_attn_decode_workspace_bytes(B, NH, HD, TMAX, splits))
      assert nbytes > 0
      q = ar.inp('q', rnd(521, B, D, dtype=BF16), misalign=True)
      kv8 = _read_cache(ar, 522, B, beyond)
      ln = ar.inp('lens', torch.tensor(lens, dtype=I32), index_margin=(1, TMAX))
      out = ar.out('out', BF16, B, D)
      lse = ar.out('lse', F32, B * NH) if want_lse else None
      ws = ar.ws('workspace', nbytes)
      return lambda: call('plm_attn_decode_kv8', P(q), P(kv8), LD8, P(ln), P(out), P(lse), B, TMAX, NH, HD, splits, P(ws), nbytes)
    CASES[f'attn_decode_kv8-splits{splits}-{"lse" if want_lse else "nolse"}'] = (('plm_attn_decode_kv8',), fn)
  n, lens0, n_new = 5, (TMAX - 5, 1, 0, 30, 13), (5, 5, 0, 2, 9)
  beyond_e = torch.ones(B * TMAX, dtype=torch.bool)
  for b in range(B):
    beyond_e[b * TMAX:b * TMAX + lens0[b] + min(n_new[b], n)] = False
  for splits, want_lse in ((1, 1), (7, 1), (0, 0)):
    def fn(ar, splits=splits, want_lse=want_lse):
      nbytes = int(L().plm_attn_extend_workspace_bytes(B, n, NH, HD, TMAX, splits))
      assert nbytes > 0
      q = ar.inp('q', rnd(531, B * n, D, dtype=BF16), misalign=True)
      kv8 = _read_cache(ar, 532, B, beyond_e)
      l0 = ar.inp('lens0', torch.tensor(lens0, dtype=I32), index_margin=(0, TMAX - n))
      nn = ar.inp('n_new', torch.tensor(n_new, dtype=I32), index_margin=(0, 1))
      out = ar.out('out', BF16, B * n, D)
      lse = ar.out('lse', F32, B * NH * n) if want_lse else None
      ws = ar.ws('workspace', nbytes)
      return lambda: call('plm_attn_extend_kv8', P(q), P(kv8), LD8, P(l0), P(nn), P(out), P(lse), B, n, TMAX, NH, HD, splits, P(ws), nbytes)
    CASES[f'attn_extend_kv8-splits{splits}-{"lse" if want_lse else "nolse"}'] = (('plm_attn_extend_kv8',), fn)


def _stage_cases():
  for tag, (B, n, lens0, n_new) in CHUNKS.items():
    def fn(ar, B=B, n=n, lens0=lens0, n_new=n_new):
      x = ar.inp('x', rnd(541, B * n, D), misalign=True)  # read-only in the stage
      nw = ar.inp('norm_w', 1 + 0.1 * rnd(542, D))
      w = ar.inp('w_qkv', rnd(543, 3 * D, D, dtype=BF16, scale=0.1))
      l0, nn, appended, _, status = _chunk(ar, B, n, lens0, n_new)
      cos, sin = _rope(TMAX)
      rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
      q_out = ar.out('q_out', BF16, B * n, D)
      kv8 = _append_only(ar, 544, B, appended)
      return lambda: call('plm_extend_norm_qkv_append_kv8_bf16', P(x), P(nw), EPS, P(w), P(l0), P(nn), P(rc), P(rs), TMAX, P(q_out), P(kv8), LD8,
                          P(status), B, n, TMAX, NH, HD)
    CASES[f'extend_norm_qkv_append_kv8-{tag}'] = (('plm_extend_norm_qkv_append_kv8_bf16',), fn)


def _layer_cases():
  rows = [('extend', tag, kind, splits) for tag, (kind, splits) in zip(('ragged-B5-n3', 'refused-B5-n3', 'ragged-B4-n8'),
                                                                         (('glu', 0), ('silu', 7), ('relu_sq', 64)))]
  rows += [('decode', 'decode-B5-n1', 'glu', 0), ('decode', 'decode-B5-n1', 'silu', 7)]
  for which, tag, kind, splits in rows:
    B, n, lens0, n_new = CHUNKS[tag]

    def fn(ar, which=which, B=B, n=n, lens0=lens0, n_new=n_new, kind=kind, splits=splits):
      nbytes = int(L().plm_decode_layer_workspace_bytes(B, NH, HD, HIDDEN, TMAX, splits) if which == 'decode' else
                   L().plm_extend_layer_workspace_bytes(B, n, NH, HD, HIDDEN, TMAX, splits))
      assert nbytes > 0
      x = ar.inout('x', rnd(551, B * n, D), misalign=True)  # the residual stream, updated in place
      an, mn = ar.inp('attn_norm_w', 1 + 0.1 * rnd(552, D)), ar.inp('mlp_norm_w', 1 + 0.1 * rnd(553, D))
      w_qkv = ar.inp('w_qkv', rnd(554, 3 * D, D, dtype=BF16, scale=0.1))
      w_out = ar.inp('w_out', rnd(555, D, D, dtype=BF16, scale=0.1))
      w_fc1 = ar.inp('w_fc1', rnd(556, (2 if kind == 'glu' else 1) * HIDDEN, D, dtype=BF16, scale=0.1))
      w_fc2 = ar.inp('w_fc2', rnd(557, D, HIDDEN, dtype=BF16, scale=0.1))
      l0, nn, appended, beyond, status = _chunk(ar, B, n, lens0, n_new)
      cos, sin = _rope(TMAX)
      rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
      # the appended rows are written before the attention reads them; rows at and beyond lens0[b] + c_b may hold anything and stay
      everything = torch.ones(B * TMAX, RB, dtype=torch.bool)
      w = row_mask(appended)
      kv8 = ar.inout('kv8', cache_rows(558, B), ld=LD8, written=w, untouched=(everything & beyond[:, None]) & ~w,
                     unread=(everything & beyond[:, None]) | w)
      ws = ar.ws('workspace', nbytes)  # exactly the queried size, between margins
      if which == 'decode':  # pos = lens0, lens = pos + 1 (clamped by the kernel for the sequence outside the cache)
        lens = ar.inp('lens', torch.tensor([min(a + 1, TMAX) for a in lens0], dtype=I32), index_margin=(1, TMAX))
        return lambda: call('plm_decode_layer_kv8_bf16', P(x), P(an), P(mn), EPS, P(w_qkv), P(w_out), P(w_fc1), P(w_fc2), P(l0), P(lens), P(rc),
                            P(rs), TMAX, P(kv8), LD8, P(status), B, TMAX, NH, HD, HIDDEN, KINDS[kind], splits, P(ws), nbytes)
      return lambda: call('plm_extend_layer_kv8_bf16', P(x), P(an), P(mn), EPS, P(w_qkv), P(w_out), P(w_fc1), P(w_fc2), P(l0), P(nn), P(rc), P(rs),
                          TMAX, P(kv8), LD8, P(status), B, n, TMAX, NH, HD, HIDDEN, KINDS[kind], splits, P(ws), nbytes)
    CASES[f'{which}_layer_kv8-{kind}-{tag}-splits{splits}'] = ((f'plm_{which}_layer_kv8_bf16',), fn)


_quant_cases()
_append_cases()
_attend_cases()
_stage_cases()
_layer_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
