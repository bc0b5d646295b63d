"""Where the launches of the fused extend read and write, on a real MI355X: the footprint cases of plm_extend_norm_qkv_append_bf16 and
plm_extend_layer_bf16.  Same machinery as tests/test_footprint_gpu.py (tests/footprint.py: every buffer between
margins, two runs that differ in one fill byte; W / I / C+R / U are bit equality): 15 and 32 chunk rows, a ragged chunk, a refused
sequence, a padded cache row stride, x read-only in the stage and ``inout`` in the layer, a workspace of exactly the queried size.
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
# tag -> (B, n, lens0, n_new or None).  Ragged: n_new holds 0, 1 and n, and one value above n (clamped); the chunks end at the cache's
# last row and start at its first.  Refused: one sequence is one row too long - nothing of it is stored, the status word is
CHUNKS = {
  'ragged-B5-n3': (5, 3, (0, 34, 17, 36, 20), (3, 3, 0, 1, 7)),
  'refused-B5-n3': (5, 3, (0, 35, 17, 1, 20), None),
  'ragged-B4-n8': (4, 8, (0, 29, 17, 36), (8, 8, 0, 1)),
  'refused-B4-n8': (4, 8, (0, 30, 17, 1), (8, 8, 3, 1)),
}


def rnd(seed, *shape, dtype=F32, scale=1.0):
  return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dtype)


def _rope(T):
  from oracle import cpu_ref as O
  return O.rope_table(HD, T)


def _chunk(ar, B, n, lens0, n_new):
  """(lens0, n_new or None, appended rows of the cache as a mask, rows at and beyond lens0 + c_b as a mask, status) of one chunk."""
  counts = [n] * B if n_new is None else [min(max(c, 0), n) for c in n_new]
  refused = [b for b in range(B) if lens0[b] < 0 or lens0[b] + counts[b] > TMAX]
  l0 = ar.inp('lens0', torch.tensor(lens0, dtype=I32), index_margin=(0, TMAX - n))
  nn = None if n_new is None else ar.inp('n_new', torch.tensor(n_new, dtype=I32), index_margin=(0, 1))
  appended = torch.zeros(B * TMAX, 2 * D, dtype=torch.bool)
  beyond = torch.ones(B * TMAX, 2 * D, dtype=torch.bool)
  for b in range(B):
    if b not in refused:
      appended[b * TMAX + lens0[b]:b * TMAX + lens0[b] + counts[b]] = True
    beyond[b * TMAX:b * TMAX + min(lens0[b] + counts[b], TMAX)] = False
  # the caller-zeroed status word: written (to 1, under both fills) only when a sequence is refused
  st = torch.tensor([bool(refused)])
  status = ar.inout('status', torch.zeros(1, dtype=I32), written=st, untouched=~st)
  return l0, nn, appended, beyond, status


def _qkv_cases():
  for tag, (B, n, lens0, n_new) in CHUNKS.items():
    def fn(ar, B=B, n=n, lens0=lens0, n_new=n_new):
      ld_kv = 2 * D + 8
      x = ar.inp('x', rnd(401, B * n, D), misalign=True)  # read-only in the stage
      nw = ar.inp('norm_w', 1 + 0.1 * rnd(402, D))
      w = ar.inp('w_qkv', rnd(403, 3 * D, D, dtype=BF16, scale=0.1))
      l0, nn, appended, _, status = _chunk(ar, B, n, lens0, n_new)
      cos, sin = _rope(TMAX)
      rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
      q_out = ar.out('q_out', BF16, B * n, D)  # wholly written: rotated q, or zeros
      everything = torch.ones(B * TMAX, 2 * D, dtype=torch.bool)  # an append reads nothing of the cache
      kv = ar.inout('kv', rnd(404, B * TMAX, 2 * D, dtype=BF16), ld=ld_kv, written=appended, untouched=~appended, unread=everything)
      return lambda: call('plm_extend_norm_qkv_append_bf16', P(x), P(nw), EPS, P(w), P(l0), P(nn), P(rc), P(rs), TMAX, P(q_out), P(kv), ld_kv,
                          P(status), B, n, TMAX, NH, HD)
    CASES[f'extend_norm_qkv_append-{tag}'] = (('plm_extend_norm_qkv_append_bf16',), fn)


def _layer_cases():
  for tag, (B, n, lens0, n_new) in CHUNKS.items():
    for kind, splits in (('glu', 0), ('silu', 7), ('relu_sq', 64)):
      def fn(ar, B=B, n=n, lens0=lens0, n_new=n_new, kind=kind, splits=splits):
        ld_kv = 2 * D + 8
        nbytes = int(L().plm_extend_layer_workspace_bytes(B, n, NH, HD, HIDDEN, TMAX, splits))
        assert nbytes > 0
        x = ar.inout('x', rnd(411, B * n, D), misalign=True)  # the residual stream, updated in place: every row, padding rows too
        an, mn = ar.inp('attn_norm_w', 1 + 0.1 * rnd(412, D)), ar.inp('mlp_norm_w', 1 + 0.1 * rnd(413, D))
        w_qkv = ar.inp('w_qkv', rnd(414, 3 * D, D, dtype=BF16, scale=0.1))
        w_out = ar.inp('w_out', rnd(415, D, D, dtype=BF16, scale=0.1))
        w_fc1 = ar.inp('w_fc1', rnd(416, (2 if kind == 'glu' else 1) * HIDDEN, D, dtype=BF16, scale=0.1))
        w_fc2 = ar.inp('w_fc2', rnd(417, D, HIDDEN, dtype=BF16, scale=0.1))
        l0, nn, appended, beyond, status = _chunk(ar, B, n, lens0, n_new)
        cos, sin = _rope(TMAX)
        rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
        # the attention reads rows 0 .. lens0[b] + c_b - 1 and the appended rows are written before they are read: every row at and
        # beyond lens0[b] + c_b may hold anything and stays as it is, the appended rows hold the fill before the launch
        kv = ar.inout('kv', rnd(418, B * TMAX, 2 * D, dtype=BF16), ld=ld_kv, written=appended, untouched=beyond & ~appended,
                      unread=beyond | appended)
        ws = ar.ws('workspace', nbytes)  # exactly the queried size, between margins
        return lambda: call('plm_extend_layer_bf16', P(x), P(an), P(mn), EPS, P(w_qkv), P(w_out), P(w_fc1), P(w_fc2), P(l0), P(nn), P(rc), P(rs),
                            TMAX, P(kv), ld_kv, P(status), B, n, TMAX, NH, HD, HIDDEN, KINDS[kind], splits, P(ws), nbytes)
      CASES[f'extend_layer-{kind}-{tag}-splits{splits}'] = (('plm_extend_layer_bf16', 'plm_extend_layer_workspace_bytes'), fn)


_qkv_cases()
_layer_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
