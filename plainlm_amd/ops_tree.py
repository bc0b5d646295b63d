"""The ops wrappers of tree verification for lookup decoding: ``ops.tree_plan`` (parents -> depths and ancestor
masks), ``ops.kv_append_rope_tree`` (store a tree row at its chunk row, rotate it at its depth), ``ops.attn_extend_tree`` (a node attends
the prefix and its ancestors), ``ops.tree_accept`` (the longest path the target's greedy predictions follow), ``ops.kv_tree_commit`` (keep
that path's cache rows), ``ops.lookup_draft_tree`` (a trie of n-gram continuations) and ``ops.extend_layer_tree`` (a whole layer over tree
rows from one library call).

Operands: B sequences of n <= TREE_MAX_ROWS rows; row b*n + r of every [B*n, ...] tensor is chunk row r of sequence b.  parent, depth and
anc are int32 [B, n] (anc holds the library's uint32 bit for bit); n_new int32 [B] or None.  bf16 caches only: an FP8 cache is refused.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract - the operand validator (``ops._need``), the launch
bracket (``ops._Launch``), the workspace arena of the current stream, ``_lib.check`` around the one library call - and, like every wrapper
there, launch hand-written gfx950 kernels with no torch fallback.  They live in a module of their own for ops_decode.py's reason."""

import collections
import ctypes as C

import torch

from . import _lib
from . import ops as O
from . import ops_decode as D

TREE_MAX_ROWS = 32    # rows of a tree chunk: one 32x32 MFMA tile of chunk keys by queries, one bit of anc per row
TREE_MAX_BRANCH = 8   # matches plm_lookup_draft_tree_i64 merges

TreePlan = collections.namedtuple('TreePlan', ['depth', 'anc'])
TreeAccept = collections.namedtuple('TreeAccept', ['n_accept', 'path', 'tokens', 'next_token', 'logprob'])
LookupTree = collections.namedtuple('LookupTree', ['tokens', 'parent', 'n_new', 'match_len'])


def _need_rows(name, t, dtype, what, B, n):
  """t: a ``dtype`` [B, n] per-row operand (contiguous, on the GPU)."""
  try:
    O._need(t, dtype, what, 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  if tuple(t.shape) != (B, n):
    raise ValueError(f'{name}: {what} {tuple(t.shape)} is not [{B}, {n}]')
  return t


def _need_seq(name, t, what, B):
  """t: None or an int32 [B] per-sequence operand."""
  if t is None:
    return None
  try:
    O._need(t, torch.int32, what, 1)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  if t.shape[0] != B:
    raise ValueError(f'{name}: {what} {tuple(t.shape)} does not fit the batch of {B}')
  return t


def _need_n(name, n):
  if not 1 <= n <= TREE_MAX_ROWS:
    raise ValueError(f'{name}: {n} rows per sequence; a tree chunk takes 1 to {TREE_MAX_ROWS}')


def _refuse_fp8(name, kv):
  if isinstance(kv, torch.Tensor) and kv.dtype == torch.uint8:
    raise TypeError(f'{name}: an FP8 cache is not served by the tree kernels (bf16 caches only)')


def tree_plan(parent, n_new=None, status=None):
  """parent int32 [B, n] (parent[b, 0] = -1, 0 <= parent[b, r] < r, or -1 for another root), n_new int32 [B] | None -> the named tuple
  (depth int32 [B, n], anc int32 [B, n]: bit j of anc[b, r] is set iff j == r or row j is an ancestor of row r).  Rows at and beyond
  n_new[b] get depth 0 and anc 0.  A real row with a parent outside [-1, r) refuses its sequence: depth -1 and anc 0 in all its rows - the
  append then stores nothing for it - and status[0] = 1 (int32 [1], zeroed by the caller; made here when absent).  One launch."""
  name = 'tree_plan'
  try:
    O._need(parent, torch.int32, 'parent', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  B, n = parent.shape
  _need_n(name, n)
  _need_seq(name, n_new, 'n_new', B)
  _need_seq(name, status, 'status', 1)
  status = torch.zeros((1,), dtype=torch.int32, device=parent.device) if status is None else status
  depth, anc = torch.empty_like(parent), torch.empty_like(parent)
  _lib.check(_lib.load().plm_tree_plan(O._p(parent), O._p(n_new), O._p(depth), O._p(anc), O._p(status), B, n, O._stream()), 'plm_tree_plan')
  return TreePlan(depth, anc)


def kv_append_rope_tree(qkv, lens0, depth, rope_cos, rope_sin, kv, nh, n_new=None, q_out=None, status=None):
  """ops.kv_append_rope_rows for tree rows: row r < n_new[b] of sequence b is stored in kv[b, lens0[b] + r] as ever but rotated at position
  lens0[b] + depth[b, r] (depth int32 [B, n], tree_plan's; clamped to [0, r]; None: at its row, kv_append_rope_rows's bits).  The
  refusals are kv_append_rope_rows's on lens0 + n_new, and a sequence tree_plan refused (depth[b, 0] < 0) stores nothing either.
  Returns (q_out bf16 [B*n, nh*hd], status)."""
  name = 'kv_append_rope_tree'
  _refuse_fp8(name, kv)
  B, n, hd = O._cached_operands(name, qkv, 3, kv, nh, lens0, 'lens0', True, n_new=n_new, rope=(rope_cos, rope_sin))
  _need_n(name, n)
  if depth is not None:
    _need_rows(name, depth, torch.int32, 'depth', B, n)
  q_out, status = O._append_outputs(name, qkv, B * n, nh * hd, q_out, status)
  _lib.check(_lib.load().plm_kv_append_rope_tree(O._p(qkv), qkv.stride(0), O._p(lens0), O._p(n_new), O._p(depth), O._p(rope_cos), O._p(rope_sin),
                                                 rope_cos.shape[0], O._p(q_out), O._p(kv), kv.stride(1), O._p(status), B, n, kv.shape[1], nh, hd,
                                                 O._stream()), 'plm_kv_append_rope_tree')
  return q_out, status


def attn_extend_tree_workspace_bytes(B, n, nh, hd, Tmax, splits=0):
  """Workspace bytes of attn_extend_tree at this shape and splits argument; a shape the library refuses raises."""
  nbytes = O._ws_bytes('plm_attn_extend_tree_workspace_bytes', B, n, nh, hd, Tmax, int(splits))
  if nbytes == 0:
    raise ValueError(f'attn_extend_tree: unsupported shape B={B} n={n} nh={nh} hd={hd} Tmax={Tmax} or splits={splits} (n <= {TREE_MAX_ROWS}; '
                     'splits 0 = automatic, 1..64)')
  return nbytes


def attn_extend_tree(q, kv, lens0, anc, nh, n_new=None, splits=0, want_lse=False):
  """Attention of a chunk of tree rows: q bf16 [B*n, nh*hd] (kv_append_rope_tree's q_out), kv with the chunk appended, lens0 int32 [B]
  the lengths BEFORE the chunk, anc int32 [B, n] (tree_plan's).  Row r < n_new[b] attends keys 0 .. lens0[b]-1 and the chunk keys
  lens0[b] + j with bit j of anc[b, r] set: its ancestors and itself.  Rows past n_new[b] give out = 0 and lse = +inf.  Three launches
  (the shared-prefix kernel over the prefix, one wave per (sequence, head) over the chunk, the combine), bit-reproducible.  splits: 0
  automatic | 1..64 forced, of the prefix.  Returns out bf16 [B*n, nh*hd], or (out, lse fp32 [B*n, nh], base 2) with want_lse."""
  name = 'attn_extend_tree'
  _refuse_fp8(name, kv)
  B, n, hd = O._cached_operands(name, q, 1, kv, nh, lens0, 'lens0', True, n_new=n_new)
  _need_n(name, n)
  _need_rows(name, anc, torch.int32, 'anc', B, n)
  Tmax = kv.shape[1]
  nbytes = attn_extend_tree_workspace_bytes(B, n, nh, hd, Tmax, splits)
  stream = O._stream()
  ws = O._workspace(q.device, nbytes, stream)
  out = torch.empty((B * n, nh * hd), dtype=O.BF16, device=q.device)
  lse = torch.empty((B * n, nh), dtype=O.F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_extend_tree(O._p(q), O._p(kv), kv.stride(1), O._p(lens0), O._p(n_new), O._p(anc), O._p(out), O._p(lse), B, n, Tmax,
                                              nh, hd, int(splits), O._p(ws), nbytes, stream), 'plm_attn_extend_tree')
  return (out, lse) if want_lse else out


def tree_accept(tok, parent, pred, logp, n_new=None, tokens_out=None):
  """Greedy acceptance over a tree: tok int64 [B, n] the rows' tokens, parent int32 [B, n], pred int64 [B, n] / logp fp32 [B, n] the
  target's greedy prediction after every row and its log-probability.  From row 0, descend to the smallest-index real child whose token
  is the current row's prediction, until there is none.  Returns the named tuple (n_accept int32 [B], path int32 [B, n] - the row at
  every accepted depth, -1 beyond -, tokens int64 [B, n-1] - the accepted tokens in path order, 0 beyond: what commit_round takes as its
  draft -, next_token int64 [B], logprob fp32 [B, n] - of the accepted tokens, then of next_token, 0 beyond).  tokens_out: an int64
  [B, n-1] buffer to write ``tokens`` into.  One launch, nothing is read back."""
  name = 'tree_accept'
  try:
    O._need(tok, torch.int64, 'tok', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  B, n = tok.shape
  _need_n(name, n)
  _need_rows(name, parent, torch.int32, 'parent', B, n)
  _need_rows(name, pred, torch.int64, 'pred', B, n)
  _need_rows(name, logp, O.F32, 'logp', B, n)
  _need_seq(name, n_new, 'n_new', B)
  dev = tok.device
  acc = torch.empty((B, n - 1), dtype=torch.int64, device=dev) if tokens_out is None else _need_rows(name, tokens_out, torch.int64, 'tokens_out', B, n - 1)
  n_accept = torch.empty((B,), dtype=torch.int32, device=dev)
  path = torch.empty((B, n), dtype=torch.int32, device=dev)
  next_tok = torch.empty((B,), dtype=torch.int64, device=dev)
  lp = torch.empty((B, n), dtype=O.F32, device=dev)
  _lib.check(_lib.load().plm_tree_accept_greedy(O._p(tok), O._p(parent), O._p(n_new), O._p(pred), O._p(logp), O._p(n_accept), O._p(path),
                                                O._p(acc) if n > 1 else None, O._p(next_tok), O._p(lp), B, n, O._stream()), 'plm_tree_accept_greedy')
  return TreeAccept(n_accept, path, acc, next_tok, lp)


def kv_tree_commit(kvs, lens0, path, n_accept, nh):
  """Keep the accepted path: in every cache of ``kvs`` (a list of bf16 [B, Tmax, 2*nh*hd] caches of one shape and stride, one per layer)
  row lens0[b] + path[b, d] is copied to row lens0[b] + d for d = 1 .. n_accept[b] (tree_accept's path and n_accept).  One launch for all
  layers; every other byte of the caches stays as it is.  The caller then moves the lengths by n_accept + 1."""
  name = 'kv_tree_commit'
  if not isinstance(kvs, (list, tuple)) or len(kvs) < 1:
    raise TypeError(f'{name}: kvs must be a non-empty list of caches')
  for kv in kvs:
    _refuse_fp8(name, kv)
  kv0 = kvs[0]
  if kv0.dim() != 3 or kv0.shape[2] % (2 * nh) != 0:
    raise ValueError(f'{name}: kv {tuple(kv0.shape)} does not fit nh={nh}')
  hd = kv0.shape[2] // (2 * nh)
  try:
    for kv in kvs:
      O._need_kv(kv, nh, hd, 'kv')
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  if any(kv.shape != kv0.shape or kv.stride() != kv0.stride() for kv in kvs):
    raise ValueError(f'{name}: the layers\' caches differ in shape or stride')
  B, Tmax = kv0.shape[:2]
  try:
    O._need(path, torch.int32, 'path', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  n = path.shape[1]
  _need_n(name, n)
  _need_rows(name, path, torch.int32, 'path', B, n)
  _need_seq(name, lens0, 'lens0', B)
  _need_seq(name, n_accept, 'n_accept', B)
  if lens0 is None or n_accept is None:
    raise TypeError(f'{name}: lens0 and n_accept are required')
  table = (C.c_void_p * len(kvs))(*[kv.data_ptr() for kv in kvs])
  _lib.check(_lib.load().plm_kv_tree_commit(table, len(kvs), kv0.stride(1), O._p(lens0), O._p(path), O._p(n_accept), B, n, Tmax, nh, hd, O._stream()),
             'plm_kv_tree_commit')


def lookup_draft_tree(hist, lens, add_tok=None, n_add=None, n=16, k=8, n_branch=3, ngram=(1, 4), status=None):
  """ops.lookup_draft proposing a trie: the same history handling and match rule, but the up to n_branch most recent occurrences of the
  longest match are kept and their continuations, k tokens each, are merged into at most n rows (row 0: the sequence's newest token;
  equal tokens under one parent share a row; rows in creation order, the most recent match first).  Returns the named tuple (tokens int64
  [B, n], parent int32 [B, n] - -1 in row 0 and in unused rows -, n_new int32 [B] = rows used: 1 without a match, 0 for a refused sequence,
  match_len int32 [B]).  With n_branch = 1 and n > k, rows 1 .. k are ops.lookup_draft's proposal.  One launch, nothing is read back."""
  name = 'lookup_draft_tree'
  O._need(hist, torch.int64, f'{name}.hist', 2)
  B, ld = hist.shape
  g_min, g_max = ngram
  for t, dtype, shape, what in ((lens, torch.int32, (B,), 'lens'), (add_tok, torch.int64, None, 'add_tok'), (n_add, torch.int32, (B,), 'n_add'),
                                (status, torch.int32, (1,), 'status')):
    if t is not None:
      O._need(t, dtype, f'{name}.{what}')
      if shape is not None and tuple(t.shape) != shape:
        raise ValueError(f'{name}: {what} {tuple(t.shape)} is not {shape} (hist {tuple(hist.shape)})')
  if add_tok is None and n_add is not None:
    raise ValueError(f'{name}: n_add without add_tok')
  if add_tok is not None and (add_tok.dim() != 2 or add_tok.shape[0] != B):
    raise ValueError(f'{name}: add_tok {tuple(add_tok.shape)} is not [B, n] for hist {tuple(hist.shape)}')
  _need_n(name, int(n))
  if not 1 <= int(n_branch) <= TREE_MAX_BRANCH:
    raise ValueError(f'{name}: n_branch must be in [1, {TREE_MAX_BRANCH}], got {n_branch}')
  dev = hist.device
  status = torch.zeros((1,), dtype=torch.int32, device=dev) if status is None else status
  tok = torch.empty((B, int(n)), dtype=torch.int64, device=dev)
  parent = torch.empty((B, int(n)), dtype=torch.int32, device=dev)
  n_new = torch.empty((B,), dtype=torch.int32, device=dev)
  match_len = torch.empty((B,), dtype=torch.int32, device=dev)
  _lib.check(_lib.load().plm_lookup_draft_tree_i64(O._p(hist), ld, O._p(lens), O._p(add_tok), 0 if add_tok is None else add_tok.shape[1], O._p(n_add),
                                                   O._p(tok), O._p(parent), O._p(n_new), O._p(match_len), O._p(status), B, int(n), int(k),
                                                   int(n_branch), int(g_min), int(g_max), O._stream()), 'plm_lookup_draft_tree_i64')
  return LookupTree(tok, parent, n_new, match_len)


def extend_layer_tree(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, n_new, depth, anc, rope_cos, rope_sin, kv, nh, kind, status,
                      splits=0):
  """ops.extend_layer over tree rows from one library call (seven launches): the qkv stage under kv_append_rope_tree's contract (depth),
  attn_extend_tree (anc), decode_gemm_residual with w_out, decode_norm_fc1_act, decode_gemm_residual with w_fc2.  x fp32 [B*n, d]
  (B = kv.shape[0], B*n <= FUSED_EXTEND_MAX_ROWS) is updated in place and returned; n_new may be None."""
  name = 'extend_layer_tree'
  _refuse_fp8(name, kv)
  M, d = D._decode_operands(name, x, (attn_norm_w, mlp_norm_w), (w_qkv, w_out, w_fc1, w_fc2))
  k = D._decode_mlp_kind(name, kind)
  hidden = w_fc2.shape[1]
  if d % nh != 0 or tuple(w_qkv.shape) != (3 * d, d) or tuple(w_out.shape) != (d, d) or w_fc2.shape[0] != d or \
     tuple(w_fc1.shape) != ((2 if kind == 'glu' else 1) * hidden, d):
    raise ValueError(f'{name}: the weights {tuple(w_qkv.shape)}, {tuple(w_out.shape)}, {tuple(w_fc1.shape)}, {tuple(w_fc2.shape)} do not fit '
                     f'x {tuple(x.shape)}, nh={nh}, kind {kind!r}')
  hd = d // nh
  B, n = D._row_operands(name, M, hd, kv, {'lens0': lens0, 'n_new': n_new}, rope_cos, rope_sin, nh, None)
  _need_rows(name, depth, torch.int32, 'depth', B, n)
  _need_rows(name, anc, torch.int32, 'anc', B, n)
  _need_seq(name, status, 'status', 1)
  Tmax = kv.shape[1]
  nbytes = O._ws_bytes('plm_extend_layer_tree_workspace_bytes', B, n, nh, hd, hidden, Tmax, int(splits))
  if nbytes == 0:
    raise ValueError(f'{name}: unsupported shape B={B} n={n} nh={nh} hd={hd} hidden={hidden} Tmax={Tmax} or splits={splits}')
  stream = O._stream()
  ws = O._workspace(x.device, nbytes, stream)
  with O._Launch('hbm:decode_fused', 2.0 * (w_qkv.numel() + w_out.numel() + w_fc1.numel() + w_fc2.numel())):
    _lib.check(_lib.load().plm_extend_layer_tree_bf16(
        O._p(x), O._p(attn_norm_w), O._p(mlp_norm_w), float(eps), O._p(w_qkv), O._p(w_out), O._p(w_fc1), O._p(w_fc2), O._p(lens0), O._p(n_new),
        O._p(depth), O._p(anc), O._p(rope_cos), O._p(rope_sin), rope_cos.shape[0], O._p(kv), kv.stride(1), O._p(status), B, n, Tmax, nh, hd, hidden, k,
        int(splits), O._p(ws), nbytes, stream), 'plm_extend_layer_tree_bf16')
  return x
