"""CPU reference of the prediction head (include/plainlm_hip.h plm_head_predict_bf16): what the GPU tests
compare against, and a plain fp32 restatement of the kernel's tile-wise arithmetic that shows how much of the tests' bound the
arithmetic itself uses.

Definitions, per row of bf16 logits l[V]:
  pred     the first index of the maximum (the lowest column among equal values), written out explicitly below - torch.argmax
           does not promise which of several equal maxima it returns;
  logp     max(l) - lse, the log-probability of pred (<= 0);
  entropy  lse - sum_i softmax(l)_i l_i, nats; a -inf logit has probability 0 and contributes 0.
"""

import torch

F64 = torch.float64
NOCOL = 0x7fffffff


def first_argmax(L):
  """int64 [M]: the lowest column that holds the row's maximum (NaN-free rows)."""
  L = L.float()
  V = L.shape[-1]
  mx = L.max(dim=-1, keepdim=True).values
  cols = torch.arange(V, dtype=torch.int64, device=L.device).expand_as(L)
  return torch.where(L == mx, cols, torch.full_like(cols, V)).min(dim=-1).values


def tied_rows(L):
  """bool [M]: rows whose maximum occurs in more than one column."""
  L = L.float()
  return (L == L.max(dim=-1, keepdim=True).values).sum(-1) > 1


def predict_reference(L):
  """bf16 (or any) logits [M, V] -> dict of fp64 'logp', 'entropy', 'lse' and int64 'pred', on the device of L."""
  x = L.double()
  lse = torch.logsumexp(x, -1)
  p = torch.exp(x - lse[:, None])
  px = torch.where(p > 0, p * x, torch.zeros_like(x))  # 0 * -inf is 0 here
  return {'pred': first_argmax(x), 'logp': x.max(-1).values - lse, 'entropy': lse - px.sum(-1), 'lse': lse}


def _combine(a, b):
  """Two (m, s, u, idx) records, each a tuple of fp32 / int64 [M] tensors: the kernel's rule, with its two guards (an empty record
  (-inf, 0, 0, none) gives way to the other side; without them 0 * -inf and -inf - -inf make NaN)."""
  ma, sa, ua, ia = a
  mb, sb, ub, ib = b
  m = torch.maximum(ma, mb)
  ea, eb = torch.exp(ma - m), torch.exp(mb - m)
  za, zb = ma == float('-inf'), mb == float('-inf')
  zero = torch.zeros_like(m)
  s = torch.where(za, zero, sa * ea) + torch.where(zb, zero, sb * eb)
  u = torch.where(za, zero, ea * (ua + sa * (ma - m))) + torch.where(zb, zero, eb * (ub + sb * (mb - m)))
  idx = torch.where(mb > ma, ib, torch.where(mb == ma, torch.minimum(ia, ib), ia))
  return m, s, u, idx


def tilewise_fp32(L, tile=128):
  """The kernel's arithmetic restated in plain fp32 on the CPU: one (max, sum-exp, u, first column) record per row and `tile` columns,
  combined left to right.  Returns fp32 'logp', 'entropy', 'lse' and int64 'pred'."""
  x = L.float().cpu()
  M, V = x.shape
  rec = (torch.full((M,), float('-inf')), torch.zeros(M), torch.zeros(M), torch.full((M,), NOCOL, dtype=torch.int64))
  for c0 in range(0, V, tile):
    xt = x[:, c0:c0 + tile]
    m = xt.max(-1).values
    d = xt - m[:, None]
    p = torch.exp(d)
    u = torch.where(p > 0, p * d, torch.zeros_like(d)).sum(-1)  # a -inf logit contributes 0, not 0 * -inf
    idx = torch.where(m == float('-inf'), torch.full((M,), NOCOL, dtype=torch.int64), c0 + first_argmax(xt))
    rec = _combine(rec, (m, torch.where(m == float('-inf'), torch.zeros(M), p.sum(-1)), u, idx))
  m, s, u, idx = rec
  ls = torch.log(s)
  return {'pred': idx, 'logp': -ls, 'entropy': ls - u / s, 'lse': m + ls}
