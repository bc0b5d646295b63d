"""Where the launches of cache extension read and write, on a real MI355X: the footprint cases of plm_kv_append_rope_rows and
plm_attn_extend.  Same machinery as tests/test_footprint_gpu.py (tests/footprint.py: every buffer between
margins, two runs that differ in one fill byte; W / I / C+R / U are bit equality), ragged chunks, padded row strides where the ABI takes
one.  That file's completeness test counts these rows."""
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
B, NH, HD, TMAX = 5, 3, 64, 37
D = NH * HD


def rnd(seed, *shape, dtype=F32):
  return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _rope(T):
  from oracle import cpu_ref as O
  return O.rope_table(HD, T)


def _append_cases():
  # full chunks; ragged chunks at both ends of the cache; one sequence that does not fit (nothing of it is stored, the status word is)
  rows = (('full', 3, (0, 34, 17, 1, 20), None),
          ('ragged', 6, (0, 31, 17, 36, 20), (6, 6, 0, 1, 3)),
          ('one-outside', 6, (0, 32, 17, 36, 20), (6, 6, 0, 1, 3)))
  for tag, n, lens0, n_new in rows:
    def fn(ar, n=n, lens0=lens0, n_new=n_new):
      ld_qkv, ld_kv = 3 * D + 8, 2 * D + 8
      counts = (n,) * B if n_new is None else n_new
      refused = [b for b in range(B) if lens0[b] + counts[b] > TMAX]
      qkv = ar.inp('qkv', rnd(91, B * n, 3 * D, dtype=BF16), ld=ld_qkv, misalign=True)
      l0 = ar.inp('lens0', torch.tensor(lens0, dtype=I32), index_margin=(0, TMAX - n))
      nn = None if n_new is None else ar.inp('n_new', torch.tensor(n_new, dtype=I32), index_margin=(0, 1))
      cos, sin = _rope(TMAX)
      rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
      q_out = ar.out('q_out', BF16, B * n, D)  # every row is written: rotated q, or zeros
      rows_w = torch.zeros(B * TMAX, 2 * D, dtype=torch.bool)
      for b in range(B):
        if b not in refused:
          rows_w[b * TMAX + lens0[b]:b * TMAX + lens0[b] + counts[b]] = True
      everything = torch.ones(B * TMAX, 2 * D, dtype=torch.bool)
      kv = ar.inout('kv', rnd(92, B * TMAX, 2 * D, dtype=BF16), ld=ld_kv, written=rows_w, untouched=~rows_w, unread=everything)
      # the caller-zeroed status word: written (to 1, under both fills) only when a sequence is refused
      st = torch.tensor([bool(refused)])
      status = ar.inout('status', torch.zeros(1, dtype=I32), written=st, untouched=~st)
      return lambda: call('plm_kv_append_rope_rows', P(qkv), ld_qkv, P(l0), P(nn), P(rc), P(rs), TMAX, P(q_out), P(kv), ld_kv, P(status), B, n,
                          TMAX, NH, HD)
    CASES[f'kv_append_rope_rows-{tag}'] = (('plm_kv_append_rope_rows',), fn)


def _extend_cases():
  # (n, lens0, n_new or None, splits, lse): full and ragged chunks, one launch (S = 1) and split + combine, a chunk wider than 32 rows
  rows = (('full-auto', 3, (0, 34, 17, 1, 20), None, 0, 1),
          ('ragged-auto', 6, (0, 31, 17, 36, 20), (6, 6, 0, 1, 3), 0, 0),
          ('ragged-splits1', 6, (0, 31, 17, 36, 20), (6, 6, 0, 1, 3), 1, 1),
          ('ragged-splits7', 6, (0, 31, 17, 36, 20), (6, 6, 0, 1, 3), 7, 1),
          ('ragged-splits64', 6, (0, 31, 17, 36, 20), (6, 6, 0, 1, 3), 64, 0),
          ('wide-splits2', 35, (0, 2, 1, 36, 20), (35, 35, 33, 1, 0), 2, 1))
  for tag, n, lens0, n_new, splits, want_lse in rows:
    def fn(ar, n=n, lens0=lens0, n_new=n_new, splits=splits, want_lse=want_lse):
      ld_kv = 2 * D + 8
      nbytes = int(L().plm_attn_extend_workspace_bytes(B, n, NH, HD, TMAX, splits))
      assert nbytes > 0
      q = ar.inp('q', rnd(93, B * n, D, dtype=BF16), misalign=True)
      kv = ar.inp('kv', rnd(94, B * TMAX, 2 * D, dtype=BF16), ld=ld_kv)
      l0 = ar.inp('lens0', torch.tensor(lens0, dtype=I32), index_margin=(0, TMAX - n))
      nn = None if n_new is None else ar.inp('n_new', torch.tensor(n_new, dtype=I32), index_margin=(0, 1))
      out = ar.out('out', BF16, B * n, D)  # every row is written: padded rows are zeros
      lse = ar.out('lse', F32, B * NH * n) if want_lse else None
      ws = ar.ws('workspace', nbytes)
      return lambda: call('plm_attn_extend', P(q), P(kv), ld_kv, P(l0), P(nn), P(out), P(lse), B, n, TMAX, NH, HD, splits, P(ws), nbytes)
    CASES[f'attn_extend-{tag}'] = (('plm_attn_extend', 'plm_attn_extend_workspace_bytes'), fn)


_append_cases()
_extend_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
