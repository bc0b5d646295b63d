"""Where the launches of KV-cached generation read and write, on a real MI355X: the footprint cases of the KV-cache entry points.
Same machinery as tests/test_footprint_gpu.py (tests/footprint.py: every buffer between margins, two runs that differ in one fill byte;
W / I / C+R / U are bit equality), ragged shapes, padded row strides where the ABI takes one.  That file's completeness test counts
these rows."""
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
  # positions at both ends of the cache; then one sequence outside it (nothing of it is written, the status word is)
  for tag, positions in (('inside', (0, 36, 17, 1, 35)), ('one-outside', (36, 0, TMAX, 5, 20))):
    def fn(ar, positions=positions):
      ld_qkv, ld_kv = 3 * D + 8, 2 * D + 8
      skipped = [b for b, t in enumerate(positions) if not 0 <= t < TMAX]
      qkv = ar.inp('qkv', rnd(91, B, 3 * D, dtype=BF16), ld=ld_qkv, misalign=True)
      pos = ar.inp('pos', torch.tensor(positions, dtype=I32), index_margin=(0, TMAX - 1))
      cos, sin = _rope(TMAX)
      rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
      q_rows = torch.ones(B, D, dtype=torch.bool)
      q_rows[skipped] = False
      q_out = ar.out('q_out', BF16, B, D, written=q_rows, untouched=~q_rows)
      rows = torch.zeros(B * TMAX, 2 * D, dtype=torch.bool)
      for b, t in enumerate(positions):
        if b not in skipped:
          rows[b * TMAX + t] = True
      everything = torch.ones(B * TMAX, 2 * D, dtype=torch.bool)
      kv = ar.inout('kv', rnd(92, B * TMAX, 2 * D, dtype=BF16), ld=ld_kv, written=rows, untouched=~rows, unread=everything)
      # the caller-zeroed status word: written (to 1, under both fills) only when a position is refused
      st = torch.tensor([bool(skipped)])
      status = ar.inout('status', torch.zeros(1, dtype=I32), written=st, untouched=~st)
      return lambda: call('plm_kv_append_rope', P(qkv), ld_qkv, P(pos), P(rc), P(rs), TMAX, P(q_out), P(kv), ld_kv, P(status), B, TMAX, NH, HD)
    CASES[f'kv_append_rope-{tag}'] = (('plm_kv_append_rope',), fn)


def _decode_cases():
  for splits, want_lse in ((7, 1), (0, 0), (64, 1), (0, 1), (1, 0)):
    def fn(ar, splits=splits, want_lse=want_lse):
      ld_kv = 2 * D + 8
      nbytes = int(L().plm_attn_decode_workspace_bytes(B, NH, HD, TMAX, splits))
      assert nbytes > 0
      q = ar.inp('q', rnd(93, B, D, dtype=BF16), misalign=True)
      kv = ar.inp('kv', rnd(94, B * TMAX, 2 * D, dtype=BF16), ld=ld_kv)
      lens = ar.inp('lens', torch.tensor([TMAX, 1, 0, 36, 13], dtype=I32), index_margin=(1, TMAX))
      out = ar.out('out', BF16, B, D)
      lse = ar.out('lse', F32, B * NH) if want_lse else None
      ws = ar.ws('workspace', nbytes)
      return lambda: call('plm_attn_decode', P(q), P(kv), ld_kv, P(lens), P(out), P(lse), B, TMAX, NH, HD, splits, P(ws), nbytes)
    CASES[f'attn_decode-splits{splits}-{"lse" if want_lse else "nolse"}'] = (('plm_attn_decode', 'plm_attn_decode_workspace_bytes'), fn)


_append_cases()
_decode_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
