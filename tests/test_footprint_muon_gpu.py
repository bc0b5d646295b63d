"""Where the launches of the Muon tail read and write, on a real MI355X: the footprint cases of plm_gemm_bf16_nt_batched,
plm_muon_prepare, plm_muon_orthogonalize, plm_muon_apply and the workspace query they share.  Same machinery as
tests/test_footprint_gpu.py (tests/footprint.py: every buffer between margins, two runs that differ in one fill byte; W / I / C+R / U are
bit equality); that file's completeness test counts these rows.  The workspace is an operand here, not scratch: each call's case claims
the blocks the header says it writes, marks the blocks it must leave alone as untouched, and fills every block it must not read."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
CASES = {}      # id -> (entry points covered, case function)
PAD = 8


def _table(struct, rows):
  t = (struct * len(rows))()
  for i, r in enumerate(rows):
    t[i] = struct(*r)
  return t


def _gemm_cases():
  from plainlm_amd import _lib
  # (tag, [(M, N, K)], D: None | 'd' | 'inplace', Ct): the smallest shapes, ragged edges in M, N and K, the optional operands absent
  rows = (('plain', [(64, 64, 64)], None, False),
          ('d-ct', [(64, 64, 64), (72, 136, 40), (200, 8, 24)], 'd', True),
          ('inplace', [(72, 136, 40), (64, 64, 64)], 'inplace', True),
          ('ct-only', [(200, 8, 24), (72, 136, 40)], None, True))
  for tag, mnk, dmode, with_ct in rows:
    def fn(ar, mnk=mnk, dmode=dmode, with_ct=with_ct):
      g = torch.Generator().manual_seed(len(mnk) * 7 + int(with_ct))
      items = []
      for i, (M, N, K) in enumerate(mnk):
        A = ar.inp(f'A{i}', torch.randn(M, K, generator=g).to(BF16), ld=K + PAD, misalign=(i == 0))
        B = ar.inp(f'B{i}', torch.randn(N, K, generator=g).to(BF16), ld=K + PAD)
        d = torch.randn(M, N, generator=g).to(BF16)
        if dmode == 'inplace':
          Cb = ar.inout(f'C{i}', d, ld=N + PAD)
          D, ldd = Cb, N + PAD
        else:
          Cb = ar.out(f'C{i}', BF16, M, N, ld=N + PAD)
          D = ar.inp(f'D{i}', d, ld=N + 2 * PAD) if dmode == 'd' else None
          ldd = N + 2 * PAD if D is not None else 0
        Ct = ar.out(f'Ct{i}', BF16, N, M, ld=M + PAD) if with_ct else None
        items.append((A.ptr, K + PAD, B.ptr, K + PAD, Cb.ptr, N + PAD, D.ptr if D is not None else None, ldd,
                      Ct.ptr if Ct is not None else None, M + PAD if Ct is not None else 0, M, N, K, 0.7, -1.3))
      table = _table(_lib.NtBatchItem, items)
      return lambda: call('plm_gemm_bf16_nt_batched', table, len(items))
    CASES[f'nt_batched-{tag}'] = (('plm_gemm_bf16_nt_batched',), fn)


SHAPES = ((64, 96), (96, 64), (72, 200))   # wide, tall, ragged 64-tiles and ragged 128-tiles


def _ws(shapes):
  """(layout, bf16 elements of the whole workspace, mask maker) of the shared workspace, asked of the library."""
  from plainlm_amd import ops
  nbytes = ops.muon_workspace_bytes(list(shapes))
  blocks, block_bytes, tiles = ops.muon_layout(list(shapes))
  assert nbytes == block_bytes + -(-tiles * 4 // 16) * 16
  n = nbytes // 2

  def mask(*names, partials=False):
    m = torch.zeros(n, dtype=torch.bool)
    for b in blocks:
      ext = {'x0': (b.x[0], b.m * b.n), 'x0t': (b.xt[0], b.m * b.n), 'x1': (b.x[1], b.m * b.n), 'x1t': (b.xt[1], b.m * b.n),
             'a': (b.a, b.m * b.m), 'bm': (b.bm, b.m * b.m)}
      for k in names:
        m[ext[k][0]:ext[k][0] + ext[k][1]] = True
    if partials:
      m[block_bytes // 2:block_bytes // 2 + 2 * tiles] = True
    return m
  return blocks, n, nbytes, mask


def _muon_cases():
  from plainlm_amd import _lib
  query = 'plm_muon_workspace_bytes'

  def shape_arrays(shapes):
    k = len(shapes)
    return (C.c_int64 * k)(*[r for r, _ in shapes]), (C.c_int64 * k)(*[c for _, c in shapes]), k

  for nesterov in (1, 0):
    def prep(ar, nesterov=nesterov):
      g = torch.Generator().manual_seed(11 + nesterov)
      blocks, n, nbytes, mask = _ws(SHAPES)
      wr = mask('x0', 'x0t', partials=True)
      ws = ar.out('workspace', BF16, n, written=wr, untouched=~wr, misalign=True)
      items = []
      for i, (r, c) in enumerate(SHAPES):
        gb = ar.inp(f'g{i}', torch.randn(r, c, generator=g))
        bb = ar.inout(f'buf{i}', torch.randn(r, c, generator=g))
        items.append((None, gb.ptr, bb.ptr, None, None, r, c, r, 0.0))
      clip = ar.inp('clip', torch.tensor([0.37]))
      nrm = ar.out('nrm', F32, len(SHAPES))
      table = _table(_lib.MuonItem, items)
      return lambda: call('plm_muon_prepare', table, len(items), 0.95, nesterov, 1e-7, P(clip), P(nrm), P(ws), nbytes)
    CASES[f'muon_prepare-nesterov{nesterov}'] = (('plm_muon_prepare', query), prep)

  for steps in (1, 2):
    def ortho(ar, steps=steps):
      g = torch.Generator().manual_seed(20 + steps)
      blocks, n, nbytes, mask = _ws(SHAPES)
      data = torch.zeros(n, dtype=BF16)
      for b in blocks:
        x = (torch.randn(b.m, b.n, generator=g) / (b.m * b.n) ** 0.5).to(BF16)
        data[b.x[0]:b.x[0] + b.m * b.n] = x.reshape(-1)
        data[b.xt[0]:b.xt[0] + b.m * b.n] = x.t().reshape(-1)
      wr = mask('x1', 'x1t', 'a', 'bm') | (mask('x0', 'x0t') if steps > 1 else torch.zeros(n, dtype=torch.bool))
      keep = ~mask('x0', 'x0t', 'x1', 'x1t', 'a', 'bm')   # the partial sums (and the tail pad): not this call's
      ws = ar.inout('workspace', data, written=wr, untouched=keep, unread=~mask('x0', 'x0t'), misalign=True)
      rows, cols, k = shape_arrays(SHAPES)
      return lambda: call('plm_muon_orthogonalize', rows, cols, k, steps, 3.4445, -4.775, 2.0315, P(ws), nbytes)
    CASES[f'muon_orthogonalize-steps{steps}'] = (('plm_muon_orthogonalize', query, 'plm_gemm_bf16_nt_batched'), ortho)

  for steps in (0, 5):
    def apply(ar, steps=steps):
      g = torch.Generator().manual_seed(30 + steps)
      blocks, n, nbytes, mask = _ws(SHAPES)
      data = torch.zeros(n, dtype=BF16)
      read = torch.zeros(n, dtype=torch.bool)
      for (r, c), b in zip(SHAPES, blocks):
        off = (b.x if r <= c else b.xt)[steps & 1]
        data[off:off + r * c] = torch.randn(r * c, generator=g).to(BF16)
        read[off:off + r * c] = True
      ws = ar.inout('workspace', data, written=torch.zeros(n, dtype=torch.bool), unread=~read, misalign=True)
      items = []
      for i, (r, c) in enumerate(SHAPES):
        p = ar.inout(f'p{i}', torch.randn(r, c, generator=g))
        dst = ar.out(f'dst{i}', BF16, r, c)
        dst_t = ar.out(f'dst_t{i}', BF16, c, r, ld=r + PAD * (i + 1))
        items.append((p.ptr, None, None, dst.ptr, dst_t.ptr, r, c, r + PAD * (i + 1), 0.01 * (i + 1)))
      table = _table(_lib.MuonItem, items)
      return lambda: call('plm_muon_apply', table, len(items), 0.9997, steps, P(ws), nbytes)
    CASES[f'muon_apply-steps{steps}'] = (('plm_muon_apply', query), apply)


_gemm_cases()
_muon_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  arenas = FP.run_on_gpu(cid, *CASES[cid])
  for ar in arenas:
    for b in ar.bufs:
      if b.role in ('out', 'inout') and b.name != 'workspace' and b.dtype in (BF16, F32):
        assert torch.isfinite(b.t.float()).all(), (cid, b.name)   # a result computed from a fill byte is a NaN under 0xFF
  assert L() is not None
