"""Where the launches of shared-prefix decoding read and write, on a real MI355X: one footprint case per new entry
point on tests/footprint.py's machinery.  The prefix cache is an input: rows at and beyond lens_p lie under NaN fill like every margin."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
CASES = {}
NP, G, NH, HD, TP, TS, HIDDEN = 2, 5, 2, 64, 300, 9, 96
D, M = NH * HD, NP * G
LENS_P = (257, 0)
ROW = (0, 8, 3, 1, 7, 0, 2, 8, 4, 5)  # the suffix row every sample appends at
EPS = 1e-6


def rnd(seed, *shape, dtype=F32, scale=1.0):
  return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _rope(T):
  from oracle import cpu_ref as O
  return O.rope_table(HD, T)


def _suffix(ar, row, append_only=False):
  """The suffix cache around a step that appends at ``row`` (None: a sample outside it): (buffer, status).  append_only: nothing is read."""
  ok = [r is not None for r in row]
  rows = torch.zeros(M * TS, 2 * D, dtype=torch.bool)
  beyond = torch.ones(M * TS, 2 * D, dtype=torch.bool)
  for i, r in enumerate(row):
    if ok[i]:
      rows[i * TS + r] = True
    beyond[i * TS:i * TS + (r + 1 if ok[i] else 2)] = False  # a refused sample attends 2 rows it did not extend
  st = torch.tensor([not all(ok)])
  status = ar.inout('status', torch.zeros(1, dtype=I32), written=st, untouched=~st)
  kv = ar.inout('kv_s', rnd(402, M * TS, 2 * D, dtype=BF16), ld=2 * D + 8, written=rows, untouched=beyond & ~rows, unread=beyond | rows | append_only)
  return kv, status


def _attn_case(splits_p, want_lse):
  def fn(ar):
    nbytes = int(L().plm_attn_decode_shared_workspace_bytes(NP, G, NH, HD, TP, TS, splits_p, 0))
    assert nbytes > 0
    q = ar.inp('q', rnd(401, M, D, dtype=BF16), misalign=True)
    kv_p = ar.inp('kv_p', rnd(403, NP * TP, 2 * D, dtype=BF16), ld=2 * D + 8)
    kv_s = ar.inp('kv_s', rnd(402, M * TS, 2 * D, dtype=BF16), ld=2 * D + 8)
    lp = ar.inp('lens_p', torch.tensor(LENS_P, dtype=I32), index_margin=(1, TP))
    ls = ar.inp('lens_s', torch.tensor([r + 1 for r in ROW[:-1]] + [0], dtype=I32), index_margin=(1, TS))
    out = ar.out('out', BF16, M, D)
    lse = ar.out('lse', F32, M * NH) if want_lse else None
    ws = ar.ws('workspace', nbytes)
    return lambda: call('plm_attn_decode_shared', P(q), P(kv_p), 2 * D + 8, P(lp), P(kv_s), 2 * D + 8, P(ls), P(out), P(lse), NP, G, TP, TS, NH, HD,
                        splits_p, 0, P(ws), nbytes)
  return ('plm_attn_decode_shared', 'plm_attn_decode_shared_workspace_bytes'), fn


def _append_case(fused, outside):
  def fn(ar):
    row = list(ROW)
    rot0 = [LENS_P[i // G] for i in range(M)]
    if outside:
      row[3], rot0[6] = TS, TP + TS  # a row past the cache, a position past the RoPE table
    refused = [not 0 <= r < TS or rot0[i] + r >= TP + TS for i, r in enumerate(row)]
    rw = ar.inp('row', torch.tensor(row, dtype=I32), index_margin=(0, TS - 1))
    r0 = ar.inp('rot0', torch.tensor(rot0, dtype=I32), index_margin=(0, 1))
    cos, sin = _rope(TP + TS)
    rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
    q_out = ar.out('q_out', BF16, M, D)  # every row is written: a refused sample's is zeros
    kv, status = _suffix(ar, [None if bad else r for r, bad in zip(row, refused)], append_only=True)
    if fused:
      x = ar.inp('x', rnd(411, M, D), misalign=True)
      nw = ar.inp('norm_w', 1 + 0.1 * rnd(412, D))
      w = ar.inp('w_qkv', rnd(413, 3 * D, D, dtype=BF16, scale=0.1))
      return lambda: call('plm_decode_norm_qkv_append_at_bf16', P(x), P(nw), EPS, P(w), P(rw), P(r0), P(rc), P(rs), TP + TS, P(q_out), P(kv),
                          2 * D + 8, P(status), M, TS, NH, HD)
    qkv = ar.inp('qkv', rnd(414, M, 3 * D, dtype=BF16), ld=3 * D + 8, misalign=True)
    return lambda: call('plm_kv_append_rope_at', P(qkv), 3 * D + 8, P(rw), P(r0), P(rc), P(rs), TP + TS, P(q_out), P(kv), 2 * D + 8, P(status), M,
                        TS, NH, HD)
  return ('plm_decode_norm_qkv_append_at_bf16' if fused else 'plm_kv_append_rope_at',), fn


def _layer_case(splits_p):
  def fn(ar):
    nbytes = int(L().plm_decode_layer_shared_workspace_bytes(NP, G, NH, HD, HIDDEN, TP, TS, splits_p, 0))
    assert nbytes > 0
    x = ar.inout('x', rnd(421, M, D), misalign=True)
    an, mn = ar.inp('attn_norm_w', 1 + 0.1 * rnd(422, D)), ar.inp('mlp_norm_w', 1 + 0.1 * rnd(423, D))
    w_qkv = ar.inp('w_qkv', rnd(424, 3 * D, D, dtype=BF16, scale=0.1))
    w_out = ar.inp('w_out', rnd(425, D, D, dtype=BF16, scale=0.1))
    w_fc1 = ar.inp('w_fc1', rnd(426, 2 * HIDDEN, D, dtype=BF16, scale=0.1))
    w_fc2 = ar.inp('w_fc2', rnd(427, D, HIDDEN, dtype=BF16, scale=0.1))
    rw = ar.inp('row', torch.tensor(ROW, dtype=I32), index_margin=(0, TS - 1))
    ls = ar.inp('lens_s', torch.tensor([r + 1 for r in ROW], dtype=I32), index_margin=(1, TS))
    r0 = ar.inp('rot0', torch.tensor([LENS_P[i // G] for i in range(M)], dtype=I32), index_margin=(0, 1))
    lp = ar.inp('lens_p', torch.tensor(LENS_P, dtype=I32), index_margin=(1, TP))
    cos, sin = _rope(TP + TS)
    rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
    kv_p = ar.inp('kv_p', rnd(403, NP * TP, 2 * D, dtype=BF16), ld=2 * D + 8)
    kv_s, status = _suffix(ar, list(ROW))
    ws = ar.ws('workspace', nbytes)
    return lambda: call('plm_decode_layer_shared_bf16', P(x), P(an), P(mn), EPS, P(w_qkv), P(w_out), P(w_fc1), P(w_fc2), P(rw), P(ls), P(r0), P(lp),
                        P(rc), P(rs), TP + TS, P(kv_p), 2 * D + 8, P(kv_s), 2 * D + 8, P(status), NP, G, TP, TS, NH, HD, HIDDEN, 0, splits_p, 0,
                        P(ws), nbytes)
  return ('plm_decode_layer_shared_bf16', 'plm_decode_layer_shared_workspace_bytes'), fn


CASES['attn_decode_shared-auto-lse'] = _attn_case(0, True)
CASES['attn_decode_shared-splits3-nolse'] = _attn_case(3, False)
CASES['kv_append_rope_at-inside'] = _append_case(False, False)
CASES['kv_append_rope_at-outside'] = _append_case(False, True)
CASES['decode_norm_qkv_append_at-outside'] = _append_case(True, True)
CASES['decode_layer_shared-auto'] = _layer_case(0)
CASES['decode_layer_shared-splits2'] = _layer_case(2)


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
