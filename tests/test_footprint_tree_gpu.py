"""Where the launches of tree verification read and write, on a real MI355X: one tests/footprint.py case per new
entry point.  The cache as in tests/test_footprint_extend_gpu.py: chunk rows written, rows beyond untouched, the fill at and beyond lens0."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402
from test_footprint_shared_gpu import rnd  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
B, N, NH, HD, T, HIDDEN, LAYERS = 2, 5, 2, 64, 300, 96, 2
D, M, LD = NH * HD, B * N, 2 * NH * HD + 8
LENS0, N_NEW = (257, 0), (5, 3)
TREE = dict(parent=((-1, 0, 0, 1, 2), (-1, 0, 1, 0, 0)), depth=((0, 1, 1, 2, 2), (0, 1, 2, 0, 0)), anc=((1, 3, 5, 11, 21), (1, 3, 7, 0, 0)))


def idx(ar, name, v, dtype=I32, **kw):  # an index-valued input: its margins hold in-range values
  return ar.inp(name, torch.tensor(v, dtype=dtype).reshape(-1), index_margin=(0, 1), **kw)


def tree(ar, *names):
  """(lens0, n_new) and the named per-row operands of the one tree every case uses; 'rope': the two tables."""
  from oracle import cpu_ref as O
  out = [idx(ar, 'lens0', LENS0), idx(ar, 'n_new', N_NEW)]
  for nm in names:
    out += [ar.inp('rope_cos', O.rope_table(HD, T)[0]), ar.inp('rope_sin', O.rope_table(HD, T)[1])] if nm == 'rope' else [idx(ar, nm, TREE[nm])]
  return out


def cache(ar, name, seed, rows_of, unread='chunk'):
  """A cache [B*T, 2*D] in which sequence b's rows lens0 + r, r in rows_of[b], are written and rows at and beyond lens0 + n_new untouched.
  unread: 'all' (an append reads nothing), 'chunk' (the written rows and those beyond hold the fill), None (a commit reads its sources)."""
  rows, beyond = (torch.zeros(B * T, 2 * D, dtype=torch.bool) for _ in range(2))
  for b in range(B):
    for r in rows_of[b]:
      rows[b * T + LENS0[b] + r] = True
    beyond[b * T + LENS0[b] + N_NEW[b]:(b + 1) * T] = True
  return ar.inout(name, rnd(seed, B * T, 2 * D, dtype=BF16), ld=LD, written=rows, untouched=beyond & ~rows,
                  unread=None if unread is None else (beyond | rows | (unread == 'all')))


def quiet_status(ar):
  return ar.inout('status', torch.zeros(1, dtype=I32), written=torch.tensor([False]), untouched=torch.tensor([True]))


def plan_case(ar):
  pr, nn = idx(ar, 'parent', TREE['parent'], misalign=True), idx(ar, 'n_new', N_NEW)
  depth, anc, st = ar.out('depth', I32, M), ar.out('anc', I32, M), quiet_status(ar)
  return lambda: call('plm_tree_plan', P(pr), P(nn), P(depth), P(anc), P(st), B, N)


def append_case(ar):
  l0, nn, dp, rc, rs = tree(ar, 'depth', 'rope')
  qkv = ar.inp('qkv', rnd(501, M, 3 * D, dtype=BF16), ld=3 * D + 8, misalign=True)
  q_out, kv, st = ar.out('q_out', BF16, M, D), cache(ar, 'kv', 502, [range(c) for c in N_NEW], 'all'), quiet_status(ar)
  return lambda: call('plm_kv_append_rope_tree', P(qkv), 3 * D + 8, P(l0), P(nn), P(dp), P(rc), P(rs), T, P(q_out), P(kv), LD, P(st), B, N, T, NH, HD)


def attn_case(ar):
  nbytes = int(L().plm_attn_extend_tree_workspace_bytes(B, N, NH, HD, T, 3))
  assert nbytes > 0
  l0, nn, an = tree(ar, 'anc')
  q = ar.inp('q', rnd(511, M, D, dtype=BF16), misalign=True)
  kv = ar.inp('kv', rnd(512, B * T, 2 * D, dtype=BF16), ld=LD)
  out, lse, ws = ar.out('out', BF16, M, D), ar.out('lse', F32, M * NH), ar.ws('workspace', nbytes)
  return lambda: call('plm_attn_extend_tree', P(q), P(kv), LD, P(l0), P(nn), P(an), P(out), P(lse), B, N, T, NH, HD, 3, P(ws), nbytes)


def accept_case(ar):
  tok = ar.inp('tok', torch.tensor(((9, 4, 5, 6, 7), (9, 4, 4, 1, 1)), dtype=I64).reshape(-1), misalign=True)
  pr, nn = idx(ar, 'parent', TREE['parent']), idx(ar, 'n_new', N_NEW)
  pred = ar.inp('pred', torch.tensor(((5, 0, 7, 0, 2), (4, 4, 8, 0, 0)), dtype=I64).reshape(-1))  # b0: 0 -> 2 -> 4; b1: 0 -> 1 -> 2
  logp = ar.inp('logp', -torch.rand(M, generator=torch.Generator().manual_seed(5)))
  outs = [ar.out('n_accept', I32, B), ar.out('path', I32, M), ar.out('acc_tok', I64, B * (N - 1)), ar.out('next_tok', I64, B), ar.out('logp_out', F32, M)]
  return lambda: call('plm_tree_accept_greedy', P(tok), P(pr), P(nn), P(pred), P(logp), *map(P, outs), B, N)


def commit_case(ar):
  l0, na = idx(ar, 'lens0', LENS0), idx(ar, 'n_accept', (2, 2))
  path = idx(ar, 'path', ((0, 2, 4, -1, -1), (0, 1, 2, -1, -1)), misalign=True)  # sequence 1's path is the identity
  table = (C.c_void_p * LAYERS)(*[cache(ar, f'kv{i}', 520 + i, [(1, 2), ()], None).ptr for i in range(LAYERS)])
  return lambda: call('plm_kv_tree_commit', table, LAYERS, LD, P(l0), P(path), P(na), B, N, T, NH, HD)


def draft_case(ar):
  ld, lens, n_add, ld_add, Bh = 300, (40, 1, 298), (3, 0, 5), 5, 3  # the last sequence's append does not fit: refused
  g = torch.Generator().manual_seed(7)
  written, beyond, unread = (torch.zeros(Bh, ld, dtype=torch.bool) for _ in range(3))
  for b in range(Bh):
    grown = n_add[b] if lens[b] + n_add[b] <= ld else 0
    unread[b, lens[b]:] = True
    written[b, lens[b]:lens[b] + grown] = True
    beyond[b, lens[b] + grown:] = True
  hist = ar.inout('hist', torch.randint(3, (Bh, ld), generator=g), written=written, untouched=beyond, unread=unread, misalign=True)
  ln = ar.inout('lens', torch.tensor(lens, dtype=I32), written=torch.tensor([True, True, False]))
  add, na = ar.inp('add_tok', torch.randint(3, (Bh, ld_add), generator=g)), idx(ar, 'n_add', n_add)
  outs = [ar.out('tok', I64, Bh * 12), ar.out('parent', I32, Bh * 12), ar.out('n_new', I32, Bh), ar.out('match_len', I32, Bh),
          ar.inout('status', torch.zeros(1, dtype=I32))]
  return lambda: call('plm_lookup_draft_tree_i64', P(hist), ld, P(ln), P(add), ld_add, P(na), *map(P, outs), Bh, 12, 4, 3, 1, 4)


def layer_case(ar):
  nbytes = int(L().plm_extend_layer_tree_workspace_bytes(B, N, NH, HD, HIDDEN, T, 0))
  assert nbytes > 0
  x = ar.inout('x', rnd(531, M, D), misalign=True)
  norms = [ar.inp(nm, 1 + 0.1 * rnd(532 + i, D)) for i, nm in enumerate(('attn_norm_w', 'mlp_norm_w'))]
  ws_ = [ar.inp(nm, rnd(534 + i, *shape, dtype=BF16, scale=0.1))
         for i, (nm, shape) in enumerate((('w_qkv', (3 * D, D)), ('w_out', (D, D)), ('w_fc1', (2 * HIDDEN, D)), ('w_fc2', (D, HIDDEN))))]
  ops_ = tree(ar, 'depth', 'anc', 'rope')
  kv, st, ws = cache(ar, 'kv', 540, [range(c) for c in N_NEW]), quiet_status(ar), ar.ws('workspace', nbytes)
  return lambda: call('plm_extend_layer_tree_bf16', P(x), *map(P, norms), 1e-6, *map(P, ws_), *map(P, ops_), T, P(kv), LD, P(st), B, N, T, NH, HD,
                      HIDDEN, 0, 0, P(ws), nbytes)


CASES = {'tree_plan': (('plm_tree_plan',), plan_case), 'kv_append_rope_tree': (('plm_kv_append_rope_tree',), append_case),
         'attn_extend_tree': (('plm_attn_extend_tree', 'plm_attn_extend_tree_workspace_bytes'), attn_case),
         'tree_accept_greedy': (('plm_tree_accept_greedy',), accept_case), 'kv_tree_commit': (('plm_kv_tree_commit',), commit_case),
         'lookup_draft_tree': (('plm_lookup_draft_tree_i64',), draft_case),
         'extend_layer_tree': (('plm_extend_layer_tree_bf16', 'plm_extend_layer_tree_workspace_bytes'), layer_case)}


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
