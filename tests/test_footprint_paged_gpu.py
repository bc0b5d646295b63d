"""Where the launches of the paged KV cache read and write, on a real MI355X: the footprint cases of its entry points (DESIGN.md section
24).  Same machinery as tests/test_footprint_gpu.py (tests/footprint.py).  The pool is an in-out buffer of which only the addressed rows
may change; pages no table entry names, and the rows past a sequence's length, hold the fill and must not reach a result.  That file's
completeness test counts these rows."""
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
B, NH, HD, PG, MAXP, NP = 4, 3, 64, 64, 5, 11
D = NH * HD
LD = 2 * D + 8
# pages out of order, with holes; -1: none
TABLE = torch.tensor([[7, 2, 9, -1, -1], [0, -1, -1, -1, -1], [5, 10, 1, 3, 8], [-1, -1, -1, -1, -1]], dtype=I32)
LENS = (130, 1, 5 * PG, 0)


def rnd(seed, *shape, dtype=F32):
  return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _rope(T):
  from oracle import cpu_ref as O
  return O.rope_table(HD, T)


def _rows(ranges):
  """bool [NP * PG, 2 * D]: token rows [a, b) of every sequence, at their pages."""
  m = torch.zeros(NP * PG, 2 * D, dtype=torch.bool)
  for b, (a, e) in enumerate(ranges):
    for t in range(a, e):
      m[int(TABLE[b, t // PG]) * PG + t % PG] = True
  return m


def _table(ar):
  return ar.inp('table', TABLE.reshape(-1), index_margin=(0, NP - 1))


def _append_case():
  lens0, n_new, n = (125, 0, 5 * PG - 2, 0), (5, 1, 3, 2), 5  # across a page edge; sequences 2 (past max_pages) and 3 (no page) are refused
  def fn(ar):
    ld_qkv = 3 * D + 8
    qkv = ar.inp('qkv', rnd(11, B * n, 3 * D, dtype=BF16), ld=ld_qkv, misalign=True)
    l0 = ar.inp('lens0', torch.tensor(lens0, dtype=I32), index_margin=(0, 1))
    nn = ar.inp('n_new', torch.tensor(n_new, dtype=I32), index_margin=(0, 1))
    cos, sin = _rope(MAXP * PG)
    rc, rs = ar.inp('rope_cos', cos), ar.inp('rope_sin', sin)
    q_out = ar.out('q_out', BF16, B * n, D)  # every row is written: rotated q, or zeros
    rows = _rows([(125, 130), (0, 1), (0, 0), (0, 0)])
    pool = ar.inout('pool', rnd(12, NP * PG, 2 * D, dtype=BF16), ld=LD, written=rows, untouched=~rows,
                    unread=torch.ones(NP * PG, 2 * D, dtype=torch.bool))
    tb = _table(ar)
    status = ar.inout('status', torch.zeros(1, dtype=I32))
    return lambda: call('plm_kv_paged_append_rope_rows', P(qkv), ld_qkv, P(l0), P(nn), P(rc), P(rs), MAXP * PG, P(q_out), P(pool), LD, P(tb),
                        P(status), B, n, MAXP, NP, NH, HD)
  CASES['kv_paged_append_rope_rows'] = (('plm_kv_paged_append_rope_rows',), fn)


def _store_case():
  T = 132
  def fn(ar):
    ld_rows = 3 * D
    real = torch.zeros(B * T, 2 * D, dtype=torch.bool)
    for b, n in enumerate((130, 1, 132, 0)):
      real[b * T:b * T + n] = True
    src = rnd(13, B * T, 2 * D, dtype=BF16)
    src[~real] = float('nan')  # padding rows past lens: they have no page and are never stored
    rows_in = ar.inp('rows', src, ld=ld_rows, misalign=True)
    lens = ar.inp('lens', torch.tensor((130, 1, 132, 0), dtype=I32), index_margin=(0, 1))
    rows = _rows([(0, 130), (0, 1), (0, 132), (0, 0)])
    pool = ar.inout('pool', rnd(14, NP * PG, 2 * D, dtype=BF16), ld=LD, written=rows, untouched=~rows,
                    unread=torch.ones(NP * PG, 2 * D, dtype=torch.bool))
    tb = _table(ar)
    st = torch.tensor([False])
    status = ar.inout('status', torch.zeros(1, dtype=I32), written=st, untouched=~st)
    return lambda: call('plm_kv_paged_store_rows', P(rows_in), ld_rows, P(lens), P(pool), LD, P(tb), P(status), B, T, MAXP, NP, NH, HD)
  CASES['kv_paged_store_rows'] = (('plm_kv_paged_store_rows',), fn)


def _pool_in(ar, seed, lens):
  """The pool of an attention launch: nothing of it is written, and every row outside the sequences' lengths - unreferenced pages, the
  tail of a last page - holds the run's fill (0x00, then NaN), so a result that took one in differs between the runs."""
  stale = ~_rows([(0, n) for n in lens])
  return ar.inout('pool', rnd(seed, NP * PG, 2 * D, dtype=BF16), ld=LD, written=torch.zeros_like(stale), untouched=stale, unread=stale)


def _decode_cases():
  for Lcap, want_lse in ((MAXP * PG, 1), (3 * PG, 0)):
    def fn(ar, Lcap=Lcap, want_lse=want_lse):
      lens = tuple(min(n, Lcap) for n in LENS)  # the kernel clamps lens to Lcap: rows beyond it are stale
      assert L().plm_kv_page_rows() == PG and L().plm_kv_paged_chunk_rows() in (128, 256, 512)
      nbytes = int(L().plm_attn_decode_paged_workspace_bytes(B, NH, HD, Lcap))
      assert nbytes > 0
      q = ar.inp('q', rnd(15, B, D, dtype=BF16), misalign=True)
      pool = _pool_in(ar, 16, lens)
      tb = _table(ar)
      ln = ar.inp('lens', torch.tensor(LENS, dtype=I32), index_margin=(0, 1))
      out = ar.out('out', BF16, B, D)
      lse = ar.out('lse', F32, B * NH) if want_lse else None
      ws = ar.ws('workspace', nbytes)
      return lambda: call('plm_attn_decode_paged', P(q), P(pool), LD, P(tb), P(ln), P(out), P(lse), B, Lcap, MAXP, NP, NH, HD, P(ws), nbytes)
    CASES[f'attn_decode_paged-Lcap{Lcap}'] = (('plm_attn_decode_paged', 'plm_attn_decode_paged_workspace_bytes', 'plm_kv_page_rows',
                                               'plm_kv_paged_chunk_rows'), fn)


def _extend_cases():
  n = 5
  for splits in (1, 3, 0):
    def fn(ar, splits=splits):
      lens0, n_new = (125, 0, 5 * PG - 5, 0), (5, 1, 5, 0)
      Lcap = MAXP * PG
      nbytes = int(L().plm_attn_extend_paged_workspace_bytes(B, n, NH, HD, Lcap, splits))
      assert nbytes > 0
      qd = rnd(17, B * n, D, dtype=BF16)
      for b, c in enumerate(n_new):
        qd[b * n + c:(b + 1) * n] = float('nan')  # padded q rows are never loaded
      q = ar.inp('q', qd, misalign=True)
      pool = _pool_in(ar, 18, [a + c for a, c in zip(lens0, n_new)])
      tb = _table(ar)
      l0 = ar.inp('lens0', torch.tensor(lens0, dtype=I32), index_margin=(0, 1))
      nn = ar.inp('n_new', torch.tensor(n_new, dtype=I32), index_margin=(0, 1))
      out = ar.out('out', BF16, B * n, D)
      lse = ar.out('lse', F32, B * NH * n)
      ws = ar.ws('workspace', nbytes)
      return lambda: call('plm_attn_extend_paged', P(q), P(pool), LD, P(tb), P(l0), P(nn), P(out), P(lse), B, n, Lcap, MAXP, NP, NH, HD, splits,
                          P(ws), nbytes)
    CASES[f'attn_extend_paged-splits{splits}'] = (('plm_attn_extend_paged', 'plm_attn_extend_paged_workspace_bytes'), fn)


def _fused_cases():
  """The fused stage and layers (B * n <= 32 rows): the appended rows are written through the table before the attention stage reads them."""
  HIDDEN, EPS, n = 256, 1e-6, 5
  w = lambda seed, *shape: (0.1 * rnd(seed, *shape)).to(BF16)  # noqa: E731

  def common(ar, rows_x, held, appended, layer):
    x = (ar.inout if layer else ar.inp)('x', rnd(21, rows_x, D), misalign=True)
    norms = [ar.inp('attn_norm_w', 1 + 0.1 * rnd(22, D))] + ([ar.inp('mlp_norm_w', 1 + 0.1 * rnd(23, D))] if layer else [])
    ws = [ar.inp('w_qkv', w(24, 3 * D, D))]
    if layer:
      ws += [ar.inp('w_out', w(25, D, D)), ar.inp('w_fc1', w(26, 2 * HIDDEN, D)), ar.inp('w_fc2', w(27, D, HIDDEN))]
    cos, sin = _rope(MAXP * PG)
    rope = (ar.inp('rope_cos', cos), ar.inp('rope_sin', sin))
    wr = _rows(appended)
    stale = ~_rows([(0, e) for e in held]) if layer else ~wr  # a layer attends the rows below `held`; the stage reads no pool row
    pool = ar.inout('pool', rnd(28, NP * PG, 2 * D, dtype=BF16), ld=LD, written=wr, untouched=stale, unread=stale | wr)
    return x, norms, ws, rope, pool, _table(ar), ar.inout('status', torch.zeros(1, dtype=I32))

  def i32(ar, name, v):
    return ar.inp(name, torch.tensor(v, dtype=I32), index_margin=(0, 1))

  def stage(ar):  # _append_case's chunk: sequences 2 (past max_pages) and 3 (no page) are refused
    x, (nw,), (wq,), (rc, rs), pool, tb, status = common(ar, B * n, None, [(125, 130), (0, 1), (0, 0), (0, 0)], False)
    l0, nn = i32(ar, 'lens0', (125, 0, 5 * PG - 2, 0)), i32(ar, 'n_new', (5, 1, 3, 2))
    q_out = ar.out('q_out', BF16, B * n, D)
    return lambda: call('plm_extend_norm_qkv_append_paged_bf16', P(x), P(nw), EPS, P(wq), P(l0), P(nn), P(rc), P(rs), MAXP * PG, P(q_out), P(pool),
                        LD, P(tb), P(status), B, n, MAXP, NP, NH, HD)
  CASES['extend_norm_qkv_append_paged'] = (('plm_extend_norm_qkv_append_paged_bf16',), stage)

  def extend(ar):
    lens0, n_new = (125, 0, 5 * PG - 5, 0), (5, 1, 5, 0)
    Lcap, splits = MAXP * PG, 3
    nbytes = int(L().plm_extend_layer_paged_workspace_bytes(B, n, NH, HD, HIDDEN, Lcap, splits))
    assert nbytes > 0
    x, (an, mn), (wq, wo, w1, w2), (rc, rs), pool, tb, status = common(ar, B * n, [a + c for a, c in zip(lens0, n_new)],
                                                                         [(a, a + c) for a, c in zip(lens0, n_new)], True)
    l0, nn = i32(ar, 'lens0', lens0), i32(ar, 'n_new', n_new)
    wsp = ar.ws('workspace', nbytes)
    return lambda: call('plm_extend_layer_paged_bf16', P(x), P(an), P(mn), EPS, P(wq), P(wo), P(w1), P(w2), P(l0), P(nn), P(rc), P(rs), MAXP * PG,
                        P(pool), LD, P(tb), P(status), B, n, Lcap, MAXP, NP, NH, HD, HIDDEN, 0, splits, P(wsp), nbytes)
  CASES['extend_layer_paged'] = (('plm_extend_layer_paged_bf16', 'plm_extend_layer_paged_workspace_bytes'), extend)

  def decode(ar):
    pos, lens, live = (129, 0, 5 * PG - 1, 0), (130, 1, 5 * PG, 0), (1, 1, 1, 0)  # slot 3 is idle: it appends nothing and attends nothing
    Lcap = MAXP * PG
    nbytes = int(L().plm_decode_layer_paged_workspace_bytes(B, NH, HD, HIDDEN, Lcap))
    assert nbytes > 0
    x, (an, mn), (wq, wo, w1, w2), (rc, rs), pool, tb, status = common(ar, B, lens, [(a, a + c) for a, c in zip(pos, live)], True)
    ps, ln, lv = i32(ar, 'pos', pos), i32(ar, 'lens', lens), i32(ar, 'live', live)
    wsp = ar.ws('workspace', nbytes)
    return lambda: call('plm_decode_layer_paged_bf16', P(x), P(an), P(mn), EPS, P(wq), P(wo), P(w1), P(w2), P(ps), P(ln), P(lv), P(rc), P(rs),
                        MAXP * PG, P(pool), LD, P(tb), P(status), B, Lcap, MAXP, NP, NH, HD, HIDDEN, 0, P(wsp), nbytes)
  CASES['decode_layer_paged'] = (('plm_decode_layer_paged_bf16', 'plm_decode_layer_paged_workspace_bytes'), decode)


_append_case()
_store_case()
_decode_cases()
_extend_cases()
_fused_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
