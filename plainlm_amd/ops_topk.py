"""The ops wrappers of the top-k head: ``ops.head_topk`` (the k most likely columns of every row of
bf16(y w^T) with their log-probabilities, the row's log-sum-exp and a target's rank, without the [M, V] logits) and
``ops.head_topk_chunk_rows``.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract - the operand validator (``ops._need``), the launch
bracket (``ops._Launch``), the workspace arena of the current stream, ``_lib.check`` around the one library call - and, like every wrapper
there, launch hand-written gfx950 kernels with no torch fallback.  They live in a module of their own for ops_decode.py's reason."""

import collections

import torch

from . import _lib
from . import ops as O

HeadTopKOut = collections.namedtuple('HeadTopKOut', ['tok', 'logp', 'lse', 'rank'])
HEAD_TOPK_MAX = 64  # head_topk.hip: one wave sorts a row's candidates


def head_topk_chunk_rows():
  """Rows of logits plm_head_topk_bf16 holds at a time (the library's PLM_HT_CHUNK, or the PLM_HT_CHUNK switch of an A/B run)."""
  return int(_lib.load().plm_head_topk_chunk_rows())


def head_topk(y, w, k, targets=None, want_lse=False):
  """Top-k head: per row of l = bf16(y[M,K] @ w[V,K]^T) - gemm_nt's logits, bit for bit, held a chunk of rows at a time (DESIGN.md
  section 25) - tok int64[M, k], the k largest columns (value descending, equal values by column ascending), and logp fp32[M, k] =
  l[tok] - lse; with ``targets`` rank int32[M], the 0-based place of the target in that order over the whole row (-1: target outside
  [0, V); V: its logit is not finite); want_lse: lse fp32[M].  Non-finite logits are absent: a row with fewer than k finite ones pads tok
  with -1 and logp with -inf.  1 <= k <= min(64, V).  Returns the named tuple (tok, logp, lse, rank), None for what was not asked for.
  No gradient."""
  if not isinstance(k, int) or not 1 <= k <= HEAD_TOPK_MAX:
    raise ValueError(f'head_topk: k={k!r} must be an int in [1, {HEAD_TOPK_MAX}]')
  try:
    O._need(y, O.BF16, 'y', strided=True)
    O._need(w, O.BF16, 'w', strided=True)
    if targets is not None:
      O._need(targets, torch.int64, 'targets', 1)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'head_topk.{e}') from None
  M, K = y.shape
  V = w.shape[0]
  if w.shape[1] != K or k > V or (targets is not None and targets.shape[0] != M):
    raise ValueError(f'head_topk: y {tuple(y.shape)}, w {tuple(w.shape)}, targets {None if targets is None else tuple(targets.shape)}, k={k} do not fit')
  launch = O._Launch('gemm_nt', 2.0 * M * V * K)
  nbytes = O._ws_bytes('plm_head_topk_workspace_bytes', M, V, K, k)
  stream = O._stream()
  ws = O._workspace(y.device, max(nbytes, 16), stream)
  tok = torch.empty((M, k), dtype=torch.int64, device=y.device)
  logp = torch.empty((M, k), dtype=O.F32, device=y.device)
  lse = torch.empty((M,), dtype=O.F32, device=y.device) if want_lse else None
  rank = torch.empty((M,), dtype=torch.int32, device=y.device) if targets is not None else None
  with launch:
    _lib.check(_lib.load().plm_head_topk_bf16(O._p(y), y.stride(0), O._p(w), w.stride(0), O._p(targets), k, O._p(tok), O._p(logp), O._p(lse), O._p(rank),
                                              M, V, K, O._p(ws), nbytes, stream), 'plm_head_topk_bf16')
  return HeadTopKOut(tok, logp, lse, rank)
