"""Shared-prefix pages without a GPU: the pool's holder counts, cascade_plan on hand-checked counts, admit_prefix /
release on the table's host mirror, the refusals of step_ragged / serve_shared / set_lens, and the argument refusals and workspace
arithmetic of the two entry points (every check comes before any HIP call)."""

import dataclasses
import os
import sys

import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib, generate as G, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_paged_host import _cfg, _rc, p  # noqa: E402

# name -> (good arguments, [(index, bad value, word of the message)])
CALLS = {
  # q, pool, ld_kv, table, lens0, key_lo, cu_rows, row_seq, tile_rows, tile_seq, tile_keys, out, lse, R, B, NT, NTg, Lcap, Pcap, max_pages,
  # n_pages, nh, hd, ws, bytes, stream
  'plm_attn_ragged_paged_cascade': ([p(), p(), 256, p(), p(), p(), p(), p(), p(), p(), p(), p(), None, 65, 3, 4, 3, 512, 128, 8, 30, 2, 64, p(),
                                     1 << 24, None],
                                    [(5, None, 'null'), (8, None, 'null'), (10, None, 'null'), (0, None, 'null'), (22, 48, 'head_dim'),
                                     (2, 250, 'stride'), (15, 66, 'NT='), (16, 0, 'NTg'), (16, 66, 'NTg'), (17, 513, 'Lcap'), (18, 96, 'Pcap'),
                                     (18, 0, 'Pcap'), (18, 576, 'Pcap'), (9, p(4098), 'aligned'), (23, p(4104), 'aligned')]),
  # x, norms x2, eps, w x4, lens0, key_lo, cu_rows, row_seq, tile_rows, tile_seq, tile_keys, cos, sin, rope_T, pool, ld_kv, table, status, R, B,
  # NT, NTg, Lcap, Pcap, max_pages, n_pages, nh, hd, hidden, kind, ws, bytes, stream
  'plm_ragged_layer_paged_wide_cascade_bf16': ([p(), p(), p(), 1e-6, p(), p(), p(), p(), p(), p(), p(), p(), p(), p(), p(), p(), p(), 512, p(), 256,
                                                p(), p(), 65, 3, 4, 3, 512, 128, 8, 30, 2, 64, 352, 0, p(), 1 << 24, None],
                                               [(9, None, 'null'), (12, None, 'null'), (20, None, 'null'), (34, None, 'null'), (31, 96, 'head_dim'),
                                                (19, 128, 'stride'), (26, 513, 'Lcap'), (22, 257, 'rows'), (24, 66, 'NT='), (25, 0, 'NTg'),
                                                (25, 66, 'NTg'), (27, 96, 'Pcap'), (27, 576, 'Pcap'), (32, 40, 'hidden = 40'),
                                                (13, p(4098), 'aligned'), (34, p(4104), 'aligned')]),
}


@pytest.mark.parametrize('name', list(CALLS))
def test_entry_points_refuse_bad_arguments_without_a_gpu(name):
  assert name in _lib.header_functions() and name in _lib.SIGNATURES
  good, bad = CALLS[name]
  for i, v, word in bad:
    args = list(good)
    args[i] = v
    rc, msg = _rc(name, *args)
    assert rc == -1 and name in msg and word in msg, (i, rc, msg)
  args = list(good)
  args[-2] = 16  # a short workspace is refused with its own code, still before any HIP call
  rc, msg = _rc(name, *args)
  assert rc == -4 and 'workspace' in msg, (rc, msg)


def test_the_workspace_queries_and_the_abi():
  lib, r16 = _lib.load(), lambda n: (n + 15) // 16 * 16
  for R, nh, hd, hidden, Lcap, NTg, Pcap in ((1, 3, 32, 288, 64, 1, 64), (65, 2, 64, 352, 1024, 3, 576), (256, 12, 128, 2048, 4608, 9, 4096)):
    part = lambda keys: r16(R * nh * -(-keys // 512) * (2 + hd) * 4)  # noqa: E731
    att = lib.plm_attn_ragged_paged_cascade_workspace_bytes(R, nh, hd, Lcap, NTg, Pcap)
    assert att == r16(4 * R) + part(Pcap) + part(Lcap)  # claim words | prefix partials | own partials
    assert part(Lcap) == lib.plm_attn_ragged_paged_workspace_bytes(R, nh, hd, Lcap)
    assert lib.plm_ragged_layer_paged_wide_cascade_workspace_bytes(R, nh, hd, hidden, Lcap, NTg, Pcap) == \
        2 * r16(R * nh * hd * 2) + r16(R * hidden * 2) + att
  for bad in ((0, 2, 64, 512, 1, 64), (65, 2, 48, 512, 1, 64), (65, 2, 64, 0, 1, 64), (65, 2, 64, 512, 0, 64), (65, 2, 64, 512, 66, 64),
              (65, 2, 64, 512, 1, 0), (65, 2, 64, 512, 1, 96), (65, 2, 64, 512, 1, 65 * 512)):
    assert lib.plm_attn_ragged_paged_cascade_workspace_bytes(*bad) == 0, bad
  assert lib.plm_ragged_layer_paged_wide_cascade_workspace_bytes(257, 2, 64, 352, 512, 1, 64) == 0
  assert ops.attn_ragged_paged_cascade.__module__ == ops.cascade_plan.__module__ == 'plainlm_amd.ops_cascade'
  assert _lib.EXPECTED_ABI == 112 == lib.plm_version()  # additive: the number did not move


def test_page_pool_counts_holders():
  pool = G.PagePool(1, 6, 2, 64, 'cpu')
  a = pool.alloc(3)
  pool.share(a[:2])
  pool.share(a[:1])
  assert pool.n_free == 3 and pool.bytes_in_use() == 3 * pool.kv[0][0].numel() * 2  # a shared page counts once
  pool.free(a)  # page a[2] was held once: it is free again, the shared ones are not
  assert pool.n_free == 4 and pool.alloc(1) == [a[2]]
  pool.free(a[:2])
  assert pool.n_free == 4  # a[1] is free, a[0] has a holder left
  pool.free(a[:1])
  assert pool.n_free == 5
  for bad in (a[:1], [6], [-1]):  # a free page, ids outside the pool
    with pytest.raises(ValueError, match='not all pages in use'):
      pool.free(bad)
    with pytest.raises(ValueError, match='not all pages in use'):
      pool.share(bad)
  with pytest.raises(ValueError, match='not all pages in use'):
    pool.free([a[2], a[2]])


def test_cascade_plan_on_hand_checked_counts():
  # slots: a group 'x' member of 40 rows, no prefix, an idle sharing slot, another 'x' member, a one-row group 'y'
  cu, row_seq, last_row, NT, key_lo, tile_rows, tile_seq, tile_keys, NTg, Pcap = ops.cascade_plan([40, 3, 0, 1, 1], [128, 0, 64, 128, 576], 'x-yxy')
  want = ops.ragged_plan([40, 3, 0, 1, 1])
  assert all(torch.equal(a, b) for a, b in zip((cu, row_seq, last_row), want)) and NT == want[3] == 5
  assert key_lo.tolist() == [128, 0, 64, 128, 576] and key_lo.dtype == tile_rows.dtype == tile_seq.dtype == tile_keys.dtype == torch.int32
  assert (NTg, Pcap) == (3, 576) and tile_seq.tolist() == [0, 0, 4] and tile_keys.tolist() == [128, 128, 576]
  assert tile_rows.tolist() == [list(range(32)), list(range(32, 40)) + [43] + [-1] * 23, [44] + [-1] * 31]  # a group's rows fill its tiles
  none = ops.cascade_plan([2, 0], [0, 64], [None, 'x'])  # no sharing slot has a row: one tile without columns
  assert none[4].tolist() == [0, 64] and none[5].tolist() == [[-1] * 32] and none[6].tolist() == [-1] and none[7].tolist() == [0] and none[8:] == (1, 64)
  with pytest.raises(ValueError, match='64 and 128 shared keys'):
    ops.cascade_plan([1, 1], [64, 128], 'xx')
  with pytest.raises(ValueError, match='multiple of 64'):
    ops.cascade_plan([1, 1], [64, 100], 'xy')


def test_admit_prefix_and_release_on_the_host_mirror():
  pool = G.PagePool(1, 8, 2, 64, 'cpu')
  pages = pool.alloc(2)
  prefix = G.PagedPrefix(pool, pages, torch.arange(3))
  cache = G.PagedKVCache(pool, 3, 256)
  cache.admit_prefix(0, prefix)
  cache.admit_prefix(2, prefix)
  cache.admit(1)
  assert cache._mirror[:, :3].tolist() == [pages + [-1], [-1, -1, -1], pages + [-1]] and torch.equal(cache.table, cache._mirror)
  assert cache.key_lo == [128, 0, 128] and cache.group == [prefix.group, None, prefix.group] and cache.bound == [128, 0, 128]
  assert cache.lens.tolist() == [128, 0, 128] and cache.pos.tolist() == [127, -1, 127] and cache.live.tolist() == [1, 1, 1]
  assert pool.n_free == 6  # three holders, two pages
  cache.reserve([1, 1, 70])  # appends take fresh pages: a shared page is never written
  assert [len(q) for q in cache.pages] == [3, 1, 4] and set(cache.pages[0][2:] + cache.pages[2][2:]).isdisjoint(pages) and pool.n_free == 2
  with pytest.raises(ValueError, match='cut into the shared prefixes'):
    cache.set_lens([127, 0, 128])
  with pytest.raises(ValueError, match='holds a sequence'):
    cache.admit_prefix(0, prefix)
  cache.release(0)
  assert cache._mirror[0].tolist() == [-1] * 4 and cache.key_lo[0] == 0 and cache.group[0] is None and pool.n_free == 3
  cache.release(2)
  prefix.release()
  cache.release(1)
  assert pool.n_free == 8 and prefix.pages == [] and prefix.n_tokens == 0
  short = G.PagedPrefix(pool, [], torch.arange(5))  # no whole page: admit_prefix is admit
  cache.admit_prefix(1, short)
  assert cache.key_lo == [0, 0, 0] and cache.pages[1] == [] and cache._live[1]
  with pytest.raises(ValueError, match='same pool'):
    cache.admit_prefix(0, G.PagedPrefix(G.PagePool(1, 2, 2, 64, 'cpu'), [], torch.arange(5)))


def test_step_ragged_and_serve_shared_refusals():
  wide = lambda **kw: dataclasses.replace(_cfg(**kw), seq_len=256)  # noqa: E731  (room for a one-page prefix)
  m = P.Transformer(wide())
  pool = G.PagePool(1, 8, 2, 64, 'cpu')
  prefix = G.PagedPrefix(pool, pool.alloc(1), torch.zeros(2, dtype=torch.int64))
  cache = G.PagedKVCache(pool, 2, 256)
  cache.admit_prefix(0, prefix)
  tok = torch.zeros(6, dtype=torch.int64)
  with pytest.raises(ValueError, match='fused=True has no cascade variant'):
    m.step_ragged(tok, [6, 0], cache, fused=True)
  assert pool.n_free == 7 and cache.bound == [64, 0]  # a refused step takes no page
  with pytest.raises(RuntimeError, match='MI355X only'):  # fused='wide' and fused=False pass the host refusals
    m.step_ragged(tok, [6, 0], cache, fused='wide')
  with pytest.raises(ValueError, match='fused=True has no cascade variant'):
    m.serve_shared(prefix, [tok], 4, 2, fused=True)
  with pytest.raises(ValueError, match="fused must be False, True or 'wide'"):
    m.serve_shared(prefix, [tok], 4, 2, fused='narrow')
  with pytest.raises(ValueError, match=r"at most 256 rows a step, got max_batch 8 \+ prefill_chunk 249"):
    m.serve_shared(prefix, [tok], 4, 8, fused='wide', prefill_chunk=249)
  with pytest.raises(TypeError, match='1-D int64 tensor or a PagedPrefix'):
    m.serve_shared([1, 2], [tok], 4, 2)
  with pytest.raises(ValueError, match='another pool'):
    m.serve_shared(prefix, [tok], 4, 2, pool=G.PagePool(1, 8, 2, 64, 'cpu'))
  with pytest.raises(RuntimeError, match='MI355X only'):
    m.serve_shared(prefix, [tok], 4, 2, fused='wide')
  for bad, word in ((wide(kv_cache='fp8'), 'FP8 pages'), (wide(linear_precision='mxfp8'), 'mxfp8')):
    for call in (lambda mm: mm.serve_shared(tok, [tok], 4, 2), lambda mm: mm.prefill_prefix(tok, pool)):
      with pytest.raises(ValueError, match=word):
        call(P.Transformer(bad))
