"""Tree verification for lookup decoding on a real MI355X: attention against an fp64 softmax under the explicit
ancestor mask, the append, the commit, plan / accept / draft against plain Python walks, the model against extend and generate."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import cpu_ref as O  # noqa: E402
import test_decode_gpu as TD  # noqa: E402
import test_lookup_gpu as TL  # noqa: E402
import test_shared_gpu as TS  # noqa: E402
from test_lookup_gpu import mdl, model, ops  # noqa: E402,F401

pytestmark = pytest.mark.gpu
BF16, I32, I64 = torch.bfloat16, torch.int32, torch.int64
bits, biteq, relmax, i32 = TD.bits, TD.biteq, TD.relmax, TS.i32
NB, NH, TMAX = TS.NP, TS.NH, 340
LENS0 = [(0, 256), (1, 300), (63, 64), (65, 257)]  # the edges of the prefix kernel's 64-key tile and 256-key step; an empty prefix


def trees(n):
  """name -> parent list: a chain, a star, two branches that split at depth 2, a seeded random tree."""
  rng = np.random.default_rng(n)
  split = [-1, 0, 1] + [r - 2 if r > 4 else 2 for r in range(3, n)]
  return {'chain': [r - 1 for r in range(n)], 'star': [-1] + [0] * (n - 1), 'split': split[:n],
          'random': [-1] + [int(rng.integers(0, r)) for r in range(1, n)]}


def walk(parent, cb):
  """The plain walk: (depth, anc) of every row; rows at and beyond cb get 0.  parent[r] < r, so a parent's entries are final."""
  depth, anc = [0] * len(parent), [0] * len(parent)
  for r, p in enumerate(parent[:cb]):
    depth[r], anc[r] = (depth[p] + 1, anc[p] | 1 << r) if p >= 0 else (0, 1 << r)
  return depth, [a - (1 << 32) if a >= 1 << 31 else a for a in anc]


@functools.lru_cache(None)
def data(hd):
  g = torch.Generator().manual_seed(2200 + hd)
  return tuple(torch.randn(*s, generator=g).to(BF16).cuda() for s in ((NB * 32, NH * hd), (NB, TMAX, 2 * NH * hd)))


def reference(q, kv, lens0, n_new, anc, n, hd):
  """test_shared_gpu's fp64 softmax, judged there by oracle/parity.py's bounds: a row's visible chunk keys are its "suffix"."""
  seen = [[j for j in range(n) if r < n_new[b] and (anc[b][r] >> j) & 1] for b in range(NB) for r in range(n)]
  kv_s = torch.zeros(NB * n, n, kv.shape[2], dtype=BF16)
  for i, js in enumerate(seen):
    kv_s[i, :len(js)] = kv[i // n, [lens0[i // n] + j for j in js]].cpu()
  want_o, want_l = TS.reference(q, kv, lens0, kv_s, [len(js) for js in seen], n, hd)
  dead = torch.tensor([not js for js in seen])
  want_o[dead], want_l[dead] = 0.0, float('inf')
  return want_o, want_l


@pytest.mark.parametrize('n', [1, 5, 32])
@pytest.mark.parametrize('lens0', LENS0)
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_extend_tree_vs_fp64_and_bit_equalities(ops, hd, lens0, n):
  q0, kv = data(hd)
  q = q0[:NB * n]
  n_new = (0, n) if lens0[0] == 0 and n > 1 else (n, (3 * n + 4) // 5)
  for name, parent in trees(n).items():
    plan = ops.tree_plan(i32([parent] * NB), i32(n_new))
    want = [walk(parent, cb) for cb in n_new]
    assert plan.depth.tolist() == [w[0] for w in want] and plan.anc.tolist() == [w[1] for w in want], name
    want_o, want_l = reference(q, kv, lens0, n_new, [w[1] for w in want], n, hd)
    run = lambda q_, kv_, sp: ops.attn_extend_tree(q_, kv_, i32(lens0), plan.anc, NH, n_new=i32(n_new), splits=sp, want_lse=True)  # noqa: E731
    for sp in (0, 1, 3):
      out, lse = run(q, kv, sp)
      TS.check_vs_fp64(f'tree hd={hd} lens0={lens0} n={n} {name} splits={sp}', out, lse, want_o, want_l, hd)
      o2, l2 = run(q, kv, sp)
      assert biteq(o2, out) and torch.equal(l2, lse), (name, sp)  # two runs
    if n == 1:
      continue
    # a node's bits do not depend on rows outside its ancestor set: change such a row's k | v and q, and rows past n_new
    b, r = 1, n_new[1] - 1
    outside = [j for j in range(n) if not (want[1][1][r] >> j) & 1]
    q4, kv4 = q.clone(), kv.clone()
    for j in outside:
      q4[b * n + j] += 1
      kv4[b, lens0[b] + j] = float('nan') if j >= n_new[b] else kv4[b, lens0[b] + j] * 2 + 1
    kv4[b, lens0[b] + n:] = float('nan')  # and nothing beyond the chunk is read
    o4, l4 = run(q4, kv4, 3)  # against the loop's last run, splits = 3
    assert biteq(o4[b * n + r], out[b * n + r]) and torch.equal(l4[b * n + r], lse[b * n + r]), (name, len(outside))


@pytest.mark.parametrize('hd', [32, 64, 128])
def test_kv_append_rope_tree_rows_are_kv_append_rope_at_the_depth(ops, hd):
  n, lens0, n_new = 7, (5, 40), (7, 4)
  parent = trees(n)['random']
  g = torch.Generator().manual_seed(hd)
  qkv = torch.randn(NB * n, 3 * NH * hd, generator=g).to(BF16).cuda()
  cos, sin = (t.cuda() for t in O.rope_table(hd, 64))
  blank = lambda: torch.zeros(NB, 64, 2 * NH * hd, dtype=BF16, device='cuda')  # noqa: E731
  plan = ops.tree_plan(i32([parent] * NB), i32(n_new))
  kv = blank()
  q, st = ops.kv_append_rope_tree(qkv, i32(lens0), plan.depth, cos, sin, kv, NH, n_new=i32(n_new))
  assert st.item() == 0
  depth = walk(parent, n)[0]
  for r in range(n):
    one = blank()
    q1, _ = ops.kv_append_rope(qkv.view(NB, n, -1)[:, r].contiguous(), i32([l + depth[r] for l in lens0]), cos, sin, one, NH)
    for b in range(NB):
      if r < n_new[b]:
        assert biteq(q[b * n + r], q1[b]) and biteq(kv[b, lens0[b] + r], one[b, lens0[b] + depth[r]]), (r, b)
      else:
        assert (bits(q[b * n + r]) == 0).all() and (bits(kv[b, lens0[b] + r]) == 0).all(), (r, b)
  # a NULL depth is kv_append_rope_rows, bit for bit
  kv_c, kv_r = blank(), blank()
  qc, _ = ops.kv_append_rope_tree(qkv, i32(lens0), None, cos, sin, kv_c, NH, n_new=i32(n_new))
  qr, _ = ops.kv_append_rope_rows(qkv, i32(lens0), cos, sin, kv_r, NH, n_new=i32(n_new))
  assert biteq(qc, qr) and biteq(kv_c, kv_r)
  # a parent at or after its row refuses the sequence: status, depth -1, nothing stored
  st, kv_b = torch.zeros(1, dtype=I32, device='cuda'), blank()
  p2 = ops.tree_plan(i32([parent, parent[:2] + [2] + parent[3:]]), i32(n_new), status=st)
  ops.kv_append_rope_tree(qkv, i32(lens0), p2.depth, cos, sin, kv_b, NH, n_new=i32(n_new))
  assert st.item() == 1 and p2.depth[1].tolist() == [-1] * n and p2.anc[1].tolist() == [0] * n and biteq(kv_b[0], kv[0]) and (bits(kv_b[1]) == 0).all()


def test_kv_tree_commit_moves_the_path_and_nothing_else(ops):
  n, hd, lens0 = 6, 32, (9, 3)
  path, na = [[0, 2, 3, 5, -1, -1], [0, 1, 2, -1, -1, -1]], [3, 2]  # a destination that is a later source; the identity
  g = torch.Generator().manual_seed(3)
  kvs = [torch.randn(NB, 24, 2 * NH * hd, generator=g).to(BF16).cuda() for _ in range(2)]
  before = [kv.clone() for kv in kvs]
  ops.kv_tree_commit(kvs, i32(lens0), i32(path), i32(na), NH)
  for kv, old in zip(kvs, before):
    want = old.clone()
    want[0, 10:13] = old[0, [11, 12, 14]]  # rows lens0 + 1 .. 3 <- lens0 + path[1 .. 3]
    assert biteq(kv, want) and not biteq(kv[0], old[0]) and biteq(kv[1], old[1])


def py_accept(tok, parent, pred, cb):
  path = [0]
  while kids := [r for r in range(1, cb) if parent[r] == path[-1] and tok[r] == pred[path[-1]]]:
    path.append(kids[0])
  return path


@pytest.mark.parametrize('n', [1, 6, 32])
def test_tree_accept_follows_the_plain_walk(ops, n):
  rng, B = np.random.default_rng(n), 6
  parent = [trees(n)[k] for k in ('chain', 'star', 'split', 'random', 'random', 'chain')]
  n_new = [n, n, n, (n + 1) // 2, 0, n]
  tok, pred = rng.integers(0, 3, (2, B, n))
  pred[0] = np.roll(tok[0], -1)  # the chain is accepted whole
  pred[5, 0] = 7                 # and no child matches at depth 0
  logp = -rng.random((B, n)).astype(np.float32)
  a = ops.tree_accept(torch.tensor(tok).cuda(), i32(parent), torch.tensor(pred).cuda(), torch.tensor(logp).cuda(), n_new=i32(n_new))
  for b in range(B):
    path = py_accept(tok[b], parent[b], pred[b], n_new[b])
    k = len(path) - 1
    assert a.n_accept[b].item() == k and a.path[b].tolist() == path + [-1] * (n - 1 - k), b
    assert a.tokens[b].tolist() == [tok[b, r] for r in path[1:]] + [0] * (n - 1 - k) and a.next_token[b].item() == pred[b, path[-1]], b
    assert a.logprob[b].tolist() == [logp[b, r] for r in path] + [0.0] * (n - 1 - k), b
  assert a.n_accept[0].item() == n - 1 and a.n_accept[5].item() == 0


@pytest.mark.parametrize('n_branch', [1, 3])
def test_lookup_draft_tree_merges_the_most_recent_matches(ops, n_branch):
  rng = np.random.default_rng(n_branch)
  B, ld, k, n, g = 4, 200, 4, 12, (1, 3)
  lens = [150, 60, 1, 199]
  hist = torch.tensor(rng.integers(0, 3, (B, ld))).cuda()
  add = torch.tensor(rng.integers(0, 3, (B, 2))).cuda()
  n_add = [2, 1, 0, 2]  # the last sequence's append does not fit
  h1, l1, h2, l2 = hist.clone(), i32(lens), hist.clone(), i32(lens)
  st = torch.zeros(1, dtype=I32, device='cuda')
  t = ops.lookup_draft_tree(h1, l1, add, i32(n_add), n=n, k=k, n_branch=n_branch, ngram=g, status=st)
  d = ops.lookup_draft(h2, l2, add, i32(n_add), k=k, ngram=g)
  assert st.item() == 1 and torch.equal(h1, h2) and torch.equal(l1, l2) and torch.equal(t.match_len, d.match_len)
  assert t.n_new[3].item() == 0
  for b in range(3):
    L, row, m = l1[b].item(), h1[b].tolist(), t.match_len[b].item()
    ends = [e for e in range(L - 1, 0, -1) if m and e >= m and row[e - m:e] == row[L - m:L]][:n_branch]
    tok, par = [row[L - 1]], [-1]
    for e in ends:  # the plain merge
      at = 0
      for i in range(k):
        x = row[e + i % (L - e)]
        kid = next((j for j in range(at + 1, len(tok)) if par[j] == at and tok[j] == x), None)
        if kid is None:
          if len(tok) == n:
            break
          tok.append(x)
          par.append(at)
          kid = len(tok) - 1
        at = kid
    assert t.n_new[b].item() == len(tok) and t.tokens[b, :len(tok)].tolist() == tok and t.parent[b].tolist() == par + [-1] * (n - len(par)), b
    if n_branch == 1 and d.n_prop[b].item():
      assert t.tokens[b, 1:k + 1].tolist() == d.draft_tokens[b].tolist() and t.parent[b, :k + 1].tolist() == list(range(-1, k)), b


@pytest.mark.parametrize('fused', [False, True])
def test_extend_tree_logits_are_extend_s_on_every_root_to_node_chain(model, mdl, fused):
  m, T0, n = model, 16, 6
  tok = mdl['tokens']
  parent = [-1, 0, 0, 1, 1, 3]
  tree = torch.stack([tok[b, [T0, T0 + 1, 40, T0 + 2, 41, 42]] for b in range(2)]).cuda()
  with torch.no_grad():
    cache, _ = m.prefill(tok[:, :T0].cuda(), max_len=32)
    lg = m.extend_tree(tree, i32([parent] * 2), cache, logits=True, fused=fused)
    assert cache.lens.tolist() == [T0, T0] and tuple(lg.shape) == (2, n, 256)
    worst = 0.0
    for r in range(n):
      chain, p = [r], parent[r]
      while p >= 0:
        chain, p = [p] + chain, parent[p]
      want = m.extend(tree[:, chain].contiguous(), cache, logits=True, fused=fused)
      cache.set_lens(i32([T0, T0]))
      worst = max(worst, relmax(lg[:, r].float().cpu(), want.float().cpu()))
    # commit a non-identity path (rows 0, 1, 4) and decode one more token: the chain 0 -> 1 -> 4 extended, then the same step
    nxt = tok[:, 43].cuda()
    m.extend(tree[:, [0, 1, 4]].contiguous(), cache, fused=fused)
    want = m.decode_step(nxt, cache, logits=True, fused=fused).float().cpu()
    cache.set_lens(i32([T0, T0]))
    m.extend_tree(tree, i32([parent] * 2), cache, fused=fused)
    cache.commit_tree(i32([[0, 1, 4, -1, -1, -1]] * 2), i32([2, 2]))
    assert cache.lens.tolist() == [T0 + 3] * 2
    worst = max(worst, relmax(m.decode_step(nxt, cache, logits=True, fused=fused).float().cpu(), want))
    cache.check()
  assert worst < 2e-2  # tests/test_extend_gpu.py's BOUND for teacher-forced logits


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('n_branch', [1, 3])
def test_generate_lookup_tree_meets_generate_s_criteria(model, mdl, n_branch, fused):
  m, N, prompt = model, TL.N, mdl['tokens'][:, :TL.T0].cuda()
  with torch.no_grad():
    toks, lps, stats = m.generate_lookup_tree(prompt, N, n_draft=TL.K, n_branch=n_branch, return_logprobs=True, return_stats=True, fused=fused)
    TL._against_the_full_forward(m, prompt, toks, lps)
    assert (stats['accepted'] <= stats['drafted']).all() and (stats['nodes'] >= stats['drafted']).all() and 1 <= stats['rounds'] <= N - 1
    eos = int(toks[0, 5].item())
    te, le = m.generate_lookup_tree(prompt, N, n_draft=TL.K, n_branch=n_branch, eos_id=eos, return_logprobs=True, fused=fused)
    for b in range(2):
      hit = (toks[b] == eos).nonzero()
      k = int(hit[0]) + 1 if len(hit) else N
      assert torch.equal(te[b, :k], toks[b, :k]) and torch.equal(le[b, :k].view(I32), lps[b, :k].view(I32)) and (te[b, k:] == eos).all() and (le[b, k:] == 0).all(), b


def test_a_prompt_with_two_continuations_drafts_a_branched_trie(model):
  """Where the first generated token is p or q, round 0 finds it twice with different continuations: both are drafted at n_branch 3."""
  cand = torch.tensor([[t, 1, 2, 3, (t + 128) % 256, 4, 5, 6, t, 7, 8, 9, (t + 128) % 256, 10, 11, 12] for t in range(13, 128)]).cuda()
  with torch.no_grad():
    first = model.generate(cand, 1)[:, 0]
    hit = ((first == cand[:, 0]) | (first == cand[:, 4])).nonzero()[:2, 0]
    assert len(hit), 'no candidate prompt contains its own first generated token'
    for nb, want in ((1, TL.K), (3, 2 * TL.K)):
      toks, stats = model.generate_lookup_tree(cand[hit].contiguous(), 2, n_draft=TL.K, n_branch=nb, return_stats=True)
      assert stats['rounds'] == 1 and stats['drafted'].tolist() == [want] * len(hit) and torch.equal(toks[:, 0], first[hit]), (nb, stats)
