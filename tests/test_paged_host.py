"""The paged KV cache without a GPU: PagePool / PagedKVCache bookkeeping on CPU tensors, the C entry points'
argument refusals (every check comes before any HIP call), the bindings, and the refusals of what a paged cache does not serve."""

import ctypes as C

import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib, generate as G, ops

NEW = ('plm_kv_page_rows', 'plm_kv_paged_chunk_rows', 'plm_kv_paged_append_rope_rows', 'plm_kv_paged_store_rows',
       'plm_attn_decode_paged_workspace_bytes', 'plm_attn_decode_paged', 'plm_attn_extend_paged_workspace_bytes', 'plm_attn_extend_paged',
       'plm_extend_norm_qkv_append_paged_bf16', 'plm_decode_layer_paged_workspace_bytes', 'plm_decode_layer_paged_bf16',
       'plm_extend_layer_paged_workspace_bytes', 'plm_extend_layer_paged_bf16')


def test_bindings_and_constants():
  lib = _lib.load()
  for name in NEW:
    assert name in _lib.header_functions() and name in _lib.SIGNATURES and hasattr(lib, name), name
  assert _lib.EXPECTED_ABI == 112 == lib.plm_version()  # additive: the number did not move
  assert lib.plm_kv_page_rows() == ops.KV_PAGE_ROWS == 64 and '#define PLM_KV_PAGE_ROWS 64' in open(_lib.HEADER_PATH).read()
  assert lib.plm_kv_paged_chunk_rows() == ops.KV_PAGED_CHUNK and ops.KV_PAGED_CHUNK in (128, 256, 512)
  assert ops.attn_decode_paged.__module__ == 'plainlm_amd.ops_paged'


def test_pool_alloc_free_and_exhaustion():
  pool = G.PagePool(2, 4, 2, 32, 'cpu')
  assert pool.n_free == 4 and len(pool.kv) == 2 and tuple(pool.kv[0].shape) == (4, 64, 128)
  a = pool.alloc(3)
  assert sorted(a) == [0, 1, 2] and pool.n_free == 1
  with pytest.raises(RuntimeError, match='2 pages asked for, 1 of 4 free'):
    pool.alloc(2)
  assert pool.n_free == 1  # a refused request takes nothing
  pool.free(a[:1])
  with pytest.raises(ValueError, match='not all pages in use'):
    pool.free(a[:1])
  assert pool.alloc(1) == a[:1] and pool.n_free == 1  # a freed page is reused first
  with pytest.raises(ValueError, match='fp8'):
    G.PagePool(2, 4, 2, 32, 'cpu', 'fp8')


def test_cache_takes_pages_at_page_edges_and_mirrors_the_table():
  pool = G.PagePool(1, 6, 2, 32, 'cpu')
  c = G.PagedKVCache(pool, 2, 200)
  assert c.max_pages == 4 and c.table.tolist() == [[-1] * 4] * 2 and c.live.tolist() == [0, 0]
  c.set_lens([64, 3])
  assert [len(p) for p in c.pages] == [1, 1] and c.lens.tolist() == [64, 3] and c.pos.tolist() == [63, 2] and c.lcap() == min(256, ops.KV_PAGED_CHUNK)
  c.advance()  # sequence 0 crosses a page edge, sequence 1 does not
  assert [len(p) for p in c.pages] == [2, 1] and c.bound == [65, 4] and c.lens.tolist() == [65, 4]
  t = c.table.tolist()
  assert t[0][:2] == c.pages[0] and t[0][2:] == [-1, -1] and t[1] == c.pages[1] + [-1] * 3 and c._dirty is None
  c.reserve([0, 61])  # to 65 tokens: the second page of sequence 1, before its chunk is launched
  c.advance_by(torch.tensor([0, 61], dtype=torch.int32))
  assert [len(p) for p in c.pages] == [2, 2] and c.lens.tolist() == [65, 65] and pool.n_free == 2
  with pytest.raises(RuntimeError, match='pages asked for'):
    c.reserve([200, 200])
  assert c.bound == [65, 65] and pool.n_free == 2  # all or nothing
  # release: pages back, row cleared, the slot idle - it no longer moves
  freed = list(c.pages[0])
  c.release(0)
  assert pool.n_free == 4 and c.table.tolist()[0] == [-1] * 4 and c.lens.tolist() == [0, 65] and c.live.tolist() == [0, 1]
  c.advance()
  assert c.lens.tolist() == [0, 66] and c.pos.tolist() == [0, 65] and c.pages[0] == []
  # adopt: page ids move between caches of one pool, no page is allocated
  one = G.PagedKVCache(pool, 1, 100)
  one.set_lens([70])
  ids, free = list(one.pages[0]), pool.n_free
  assert set(ids) == set(freed)  # the freed pages are reused
  c.adopt(0, one, 0)
  assert c.pages[0] == ids and one.pages[0] == [] and pool.n_free == free and c.table.tolist()[0] == ids + [-1, -1]
  assert c.lens.tolist() == [70, 66] and c.pos.tolist() == [69, 65] and one.lens.tolist() == [0] and one.table.tolist() == [[-1, -1]]
  with pytest.raises(ValueError, match='holds a sequence'):
    c.adopt(0, one, 0)
  with pytest.raises(ValueError, match='same pool'):
    c.adopt(0, G.PagedKVCache(G.PagePool(1, 2, 2, 32, 'cpu'), 1, 64), 0)
  assert tuple(c.gather(0).shape) == (2, 256, 128)


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------------------
def _rc(name, *args):
  lib = _lib.load()
  rc = getattr(lib, name)(*args)
  return rc, (lib.plm_last_error_string() or b'').decode()


p = lambda a=4096: C.c_void_p(a)  # noqa: E731  (a fake, 16-byte aligned device pointer: refused calls never touch it)
# name -> (good arguments, [(index, bad value, word of the message)])
CALLS = {
  # qkv, ld_qkv, lens0, n_new, cos, sin, rope_T, q_out, pool, ld_kv, table, status, B, n, max_pages, n_pages, nh, hd, stream
  'plm_kv_paged_append_rope_rows': ([p(), 384, p(), None, p(), p(), 256, p(), p(), 256, p(), p(), 2, 3, 4, 9, 2, 64, None],
                                    [(0, None, 'null'), (10, None, 'null'), (17, 48, 'head_dim'), (9, 250, 'stride'), (1, 380, 'stride'),
                                     (14, 0, 'max_pages'), (15, 0, 'n_pages'), (8, p(4104), 'aligned')]),
  # rows, ld_rows, lens, pool, ld_kv, table, status, B, T, max_pages, n_pages, nh, hd, stream
  'plm_kv_paged_store_rows': ([p(), 384, p(), p(), 256, p(), p(), 2, 70, 4, 9, 2, 64, None],
                              [(3, None, 'null'), (12, 16, 'head_dim'), (1, 250, 'stride'), (4, 257, 'stride'), (8, 0, 'bad shape')]),
  # q, pool, ld_kv, table, lens, out, lse, B, Lcap, max_pages, n_pages, nh, hd, workspace, bytes, stream
  'plm_attn_decode_paged': ([p(), p(), 256, p(), p(), p(), None, 2, 256, 4, 9, 2, 64, p(), 1 << 20, None],
                            [(0, None, 'null'), (13, None, 'null'), (12, 96, 'head_dim'), (2, 128, 'stride'), (8, 257, 'Lcap'), (8, 0, 'Lcap')]),
  # q, pool, ld_kv, table, lens0, n_new, out, lse, B, n, Lcap, max_pages, n_pages, nh, hd, splits, workspace, bytes, stream
  'plm_attn_extend_paged': ([p(), p(), 256, p(), p(), None, p(), None, 2, 5, 256, 4, 9, 2, 64, 0, p(), 1 << 20, None],
                            [(3, None, 'null'), (14, 256, 'head_dim'), (2, 260, 'stride'), (10, 300, 'Lcap'), (15, 65, 'splits'), (9, 0, 'bad shape')]),
  # x, norm_w, eps, w_qkv, lens0, n_new, cos, sin, rope_T, q_out, pool, ld_kv, table, status, B, n, max_pages, n_pages, nh, hd, stream
  'plm_extend_norm_qkv_append_paged_bf16': ([p(), p(), 1e-6, p(), p(), None, p(), p(), 256, p(), p(), 256, p(), p(), 2, 3, 4, 9, 2, 64, None],
                                            [(12, None, 'null'), (10, None, 'null'), (19, 48, 'head_dim'), (11, 250, 'stride'), (15, 17, 'rows'),
                                             (16, 0, 'max_pages'), (17, 0, 'n_pages')]),
  # x, norms x2, eps, w x4, pos, lens, live, cos, sin, rope_T, pool, ld_kv, table, status, B, Lcap, max_pages, n_pages, nh, hd, hidden, kind, ws, bytes, stream
  'plm_decode_layer_paged_bf16': ([p(), p(), p(), 1e-6, p(), p(), p(), p(), p(), p(), None, p(), p(), 256, p(), 256, p(), p(), 2, 256, 4, 9, 2, 64,
                                   352, 0, p(), 1 << 22, None],
                                  [(16, None, 'null'), (9, None, 'null'), (23, 96, 'head_dim'), (15, 128, 'stride'), (19, 257, 'Lcap'), (18, 33, 'rows')]),
  # x, norms x2, eps, w x4, lens0, n_new, cos, sin, rope_T, pool, ld_kv, table, status, B, n, Lcap, max_pages, n_pages, nh, hd, hidden, kind, splits, ws, ..
  'plm_extend_layer_paged_bf16': ([p(), p(), p(), 1e-6, p(), p(), p(), p(), p(), None, p(), p(), 256, p(), 256, p(), p(), 2, 3, 256, 4, 9, 2, 64,
                                   352, 0, 0, p(), 1 << 22, None],
                                  [(15, None, 'null'), (13, None, 'null'), (23, 96, 'head_dim'), (19, 0, 'Lcap'), (18, 17, 'rows'), (26, 65, 'splits')]),
}


@pytest.mark.parametrize('name', list(CALLS))
def test_entry_points_refuse_bad_arguments_without_a_gpu(name):
  good, bad = CALLS[name]
  for i, v, word in bad:
    args = list(good)
    args[i] = v
    rc, msg = _rc(name, *args)
    assert rc == -1 and name in msg and word in msg, (i, rc, msg)
  if 'attn' in name or 'layer' in name:  # a short workspace is refused with its own code, still before any HIP call
    args = list(good)
    args[-2] = 16
    rc, msg = _rc(name, *args)
    assert rc == -4 and 'workspace' in msg, (rc, msg)


def test_the_split_cap_and_the_workspace_queries():
  lib, Cn = _lib.load(), ops.KV_PAGED_CHUNK
  # Lcap beyond CACHE_MAX_SPLITS = 64 chunks: the query answers 0, the launch is refused
  assert lib.plm_attn_decode_paged_workspace_bytes(2, 2, 64, 64 * Cn) == 2 * 2 * 64 * (2 + 64) * 4
  assert lib.plm_attn_decode_paged_workspace_bytes(2, 2, 64, 64 * Cn + 1) == 0
  assert lib.plm_attn_decode_paged_workspace_bytes(2, 2, 48, 256) == 0
  pages = 65 * Cn // 64
  rc, msg = _rc('plm_attn_decode_paged', p(), p(), 256, p(), p(), p(), None, 2, 64 * Cn + 1, pages, 9, 2, 64, p(), 1 << 30, None)
  assert rc == -1 and 'chunks' in msg, (rc, msg)
  assert lib.plm_attn_extend_paged_workspace_bytes(2, 5, 2, 64, 256, 3) == 2 * 2 * 3 * 5 * (2 + 64) * 4
  assert lib.plm_attn_extend_paged_workspace_bytes(2, 5, 2, 64, 256, 65) == 0


# ---- what a paged cache does not serve ------------------------------------------------------------------------------------------------
def _cfg(**kw):
  return P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=1, n_heads=2, mlp='glu', **kw)


def test_unsupported_combinations_are_refused_by_name():
  m = P.Transformer(_cfg())
  pool = G.PagePool(1, 4, 2, 64, 'cpu')
  cache = G.PagedKVCache(pool, 2, 64)
  tok = torch.zeros(2, dtype=torch.int64)
  for call in (lambda: m.fork(cache, 2, 4), lambda: m.fork_beam(cache, 2, 4),
               lambda: m.extend_tree(tok.view(2, 1), torch.full((2, 1), -1, dtype=torch.int32), cache)):
    with pytest.raises(TypeError, match='PagedKVCache'):
      call()
  with pytest.raises(ValueError, match='FP8 pages'):
    P.Transformer(_cfg(kv_cache='fp8')).new_page_pool(4)
  with pytest.raises(ValueError, match='mxfp8'):
    P.Transformer(_cfg(linear_precision='mxfp8')).new_page_pool(4)
  with pytest.raises(ValueError, match='mxfp8'):
    P.Transformer(_cfg(linear_precision='mxfp8')).serve([tok], 4, 2)
  for kw in (dict(temperature=0.8), dict(top_k=5), dict(top_p=0.9), dict(seed=1), dict(sample=lambda x: x)):
    with pytest.raises(ValueError, match='greedy only'):
      m.serve([tok], 4, 2, **kw)
  with pytest.raises(ValueError, match='fused=True serves at most 32'):  # fused beyond the row cap
    m.serve([tok], 4, 33, fused=True)
  with pytest.raises(TypeError, match='1-D int64'):
    m.serve([tok.view(1, 2)], 4, 2)
  with pytest.raises(TypeError, match='PagePool'):
    G.PagedKVCache(object(), 2, 64)
  with pytest.raises(ValueError, match='pages are not served'):
    G.PagePool(1, 4, 2, 64, 'cpu', 'fp8')
