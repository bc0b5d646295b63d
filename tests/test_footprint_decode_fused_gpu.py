"""Where the launches of the fused decode step read and write, on a real MI355X: the footprint cases of the plm_decode_* entry points
(DESIGN.md section 17).  Same machinery as tests/test_footprint_gpu.py (tests/footprint.py: every buffer between margins, two runs that
differ in one fill byte; W / I / C+R / U are bit equality): ragged B, a padded cache row stride, one refused position, x as ``inout``.
That file's completeness test counts these rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
CASES = {}      # id -> (entry points covered, case function)
NH, HD, TMAX, HIDDEN = 3, 32, 37, 288
D = NH * HD
EPS = 1e-6
KINDS = {'glu': 0, 'silu': 1, 'relu_sq': 2}


def rnd(seed, *shape, dtype=F32, scale=1.0):
  return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _rope(T):
  from oracle import cpu_ref as O
  return O.rope_table(HD, T)


def _positions(B, outside):
  pos = [(0, TMAX - 1, 17, 1, 35)[b % 5] for b in range(B)]
  if outside:
    pos[min(2, B - 1)] = TMAX
  return pos


def _cache(ar, B, pos):
  """(kv as inout between margins with a padded row stride, status): the rows of the stored positions are written, nothing else is, and
  nothing of the cache is read by an append."""
  skipped = [b for b, t in enumerate(pos) if not 0 <= t < TMAX]
  rows = torch.zeros(B * TMAX, 2 * D, dtype=torch.bool)
  for b, t in enumerate(pos):
    if b not in skipped:
      rows[b * TMAX + t] = True
  st = torch.tensor([bool(skipped)])
  status = ar.inout('status', torch.zeros(1, dtype=I32), written=st, untouched=~st)
  return rows, status


def _qkv_cases():
  for tag, B, outside in (('inside-B5', 5, False), ('one-outside-B5', 5, True), ('one-outside-B17', 17, True)):
    def fn(ar, B=B, outside=outside):
      ld_kv = 2 * D + 8
      pos = _positions(B, outside)
      x = ar.inp('x', rnd(301, B, D), misalign=True)
      nw = ar.inp('norm_w', 1 + 0.1 * rnd(302, D))
      w = ar.inp('w_qkv', rnd(303, 3 * D, D, dtype=BF16, scale=0.1))
      p = ar.inp('pos', torch.tensor(pos, dtype=I32), index_margin=(0, TMAX - 1))
      cos, sin = _rope(TMAX)
      rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
      q_out = ar.out('q_out', BF16, B, D)  # every row is written: a refused sequence's is zeros
      rows, status = _cache(ar, B, pos)
      everything = torch.ones(B * TMAX, 2 * D, dtype=torch.bool)
      kv = ar.inout('kv', rnd(304, B * TMAX, 2 * D, dtype=BF16), ld=ld_kv, written=rows, untouched=~rows, unread=everything)
      return lambda: call('plm_decode_norm_qkv_append_bf16', P(x), P(nw), EPS, P(w), P(p), P(rc), P(rs), TMAX, P(q_out), P(kv), ld_kv, P(status),
                          B, TMAX, NH, HD)
    CASES[f'decode_norm_qkv_append-{tag}'] = (('plm_decode_norm_qkv_append_bf16',), fn)


def _residual_cases():
  for M, K in ((5, D), (5, HIDDEN), (17, HIDDEN), (32, 1056)):  # K = 1056 at M = 32: three chunks of the LDS tile (512 + 512 + 32)
    def fn(ar, M=M, K=K):
      x = ar.inout('x', rnd(311, M, D), misalign=True)
      a = ar.inp('A', rnd(312, M, K, dtype=BF16))
      w = ar.inp('W', rnd(313, D, K, dtype=BF16, scale=0.1))
      return lambda: call('plm_decode_gemm_residual_bf16', P(x), P(a), P(w), M, D, K)
    CASES[f'decode_gemm_residual-M{M}-K{K}'] = (('plm_decode_gemm_residual_bf16',), fn)


def _fc1_cases():
  for kind, M in (('glu', 5), ('silu', 5), ('relu_sq', 5), ('glu', 17)):
    def fn(ar, kind=kind, M=M):
      rows = (2 if kind == 'glu' else 1) * HIDDEN
      x = ar.inp('x', rnd(321, M, D), misalign=True)
      nw = ar.inp('norm_w', 1 + 0.1 * rnd(322, D))
      w = ar.inp('w_fc1', rnd(323, rows, D, dtype=BF16, scale=0.1))
      act = ar.out('act', BF16, M, HIDDEN)
      return lambda: call('plm_decode_norm_fc1_act_bf16', P(x), P(nw), EPS, P(w), P(act), M, D, HIDDEN, KINDS[kind])
    CASES[f'decode_norm_fc1_act-{kind}-M{M}'] = (('plm_decode_norm_fc1_act_bf16',), fn)


def _layer_cases():
  for kind, B, splits in (('glu', 5, 0), ('silu', 5, 7), ('relu_sq', 17, 0), ('glu', 17, 64)):
    def fn(ar, kind=kind, B=B, splits=splits):
      ld_kv = 2 * D + 8
      nbytes = int(L().plm_decode_layer_workspace_bytes(B, NH, HD, HIDDEN, TMAX, splits))
      assert nbytes > 0
      pos = _positions(B, True)
      lens = [min(max(t + 1, 0), TMAX) if 0 <= t < TMAX else 9 for t in pos]  # the refused sequence attends 9 rows it did not extend
      x = ar.inout('x', rnd(331, B, D), misalign=True)
      an, mn = ar.inp('attn_norm_w', 1 + 0.1 * rnd(332, D)), ar.inp('mlp_norm_w', 1 + 0.1 * rnd(333, D))
      w_qkv = ar.inp('w_qkv', rnd(334, 3 * D, D, dtype=BF16, scale=0.1))
      w_out = ar.inp('w_out', rnd(335, D, D, dtype=BF16, scale=0.1))
      w_fc1 = ar.inp('w_fc1', rnd(336, (2 if kind == 'glu' else 1) * HIDDEN, D, dtype=BF16, scale=0.1))
      w_fc2 = ar.inp('w_fc2', rnd(337, D, HIDDEN, dtype=BF16, scale=0.1))
      p = ar.inp('pos', torch.tensor(pos, dtype=I32), index_margin=(0, TMAX - 1))
      ln = ar.inp('lens', torch.tensor(lens, dtype=I32), index_margin=(1, TMAX))
      cos, sin = _rope(TMAX)
      rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
      rows, status = _cache(ar, B, pos)
      # the attention reads rows 0 .. lens[b] - 1 and the appended row is written before it is read: every row beyond may hold anything and
      # stays as it is, the appended rows hold the fill before the launch
      beyond = torch.ones(B * TMAX, 2 * D, dtype=torch.bool)
      for b, n in enumerate(lens):
        beyond[b * TMAX:b * TMAX + n] = False
      kv = ar.inout('kv', rnd(338, B * TMAX, 2 * D, dtype=BF16), ld=ld_kv, written=rows, untouched=beyond & ~rows, unread=beyond | rows)
      ws = ar.ws('workspace', nbytes)
      return lambda: call('plm_decode_layer_bf16', P(x), P(an), P(mn), EPS, P(w_qkv), P(w_out), P(w_fc1), P(w_fc2), P(p), P(ln), P(rc), P(rs),
                          TMAX, P(kv), ld_kv, P(status), B, TMAX, NH, HD, HIDDEN, KINDS[kind], splits, P(ws), nbytes)
    CASES[f'decode_layer-{kind}-B{B}-splits{splits}'] = (('plm_decode_layer_bf16', 'plm_decode_layer_workspace_bytes'), fn)


_qkv_cases()
_residual_cases()
_fc1_cases()
_layer_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
