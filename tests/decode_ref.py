"""References for the decode attention kernel (plm_attn_decode): a fp64 softmax of one query row over its keys, and a numpy
restatement of what the kernel does instead - split the keys into S contiguous ranges, keep a base-2 partial (m, l, acc) per range,
combine the partials in split order - with the kernel's partition rule and its two non-finite hazards (an empty range, no key at all)."""

import math

import numpy as np

LOG2E = 1.4426950408889634


def attn_row(q, k, v):
  """q [hd], k / v [L, hd] -> (out [hd], lse2): softmax(q k^T / sqrt(hd)) v in fp64 and the base-2 log-sum-exp of the scaled scores.
  L == 0: out = 0 and lse2 = +inf (the kernels' rule for a row with no key)."""
  q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
  if k.shape[0] == 0:
    return np.zeros(q.shape[0]), math.inf
  s = k @ q / math.sqrt(q.shape[0])
  m = s.max()
  p = np.exp(s - m)
  return (p @ v) / p.sum(), (m + math.log(p.sum())) * LOG2E


def split_ranges(L, S):
  """The kernel's partition of keys 0 .. L-1 into S contiguous ranges of ceil(L / S) keys; trailing ranges may be empty."""
  chunk = -(-L // S)
  out = []
  for s in range(S):
    k0 = min(s * chunk, L)
    out.append((k0, min(k0 + chunk, L)))
  return out


def partial(q, k, v):
  """(m, l, acc) of one key range in log2 units: m = max score, l = sum 2^(s - m), acc = sum 2^(s - m) v.  Empty: (-inf, 0, 0)."""
  q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
  if k.shape[0] == 0:
    return -math.inf, 0.0, np.zeros(q.shape[0])
  s = (k @ q) * (LOG2E / math.sqrt(q.shape[0]))
  m = s.max()
  p = np.exp2(s - m)
  return m, p.sum(), p @ v


def combine(parts, hd):
  """The combine kernel's rule: partials with m = -inf carry no weight and are skipped (their 2^(m - M) would be 2^(-inf - -inf) = NaN
  when every partial is empty); no partial at all gives out = 0, lse2 = +inf."""
  M = max(m for m, _, _ in parts)
  if M == -math.inf:
    return np.zeros(hd), math.inf
  l, acc = 0.0, np.zeros(hd)
  for m, li, ai in parts:
    if m == -math.inf:
      continue
    w = np.exp2(m - M)
    l += li * w
    acc = acc + ai * w
  return acc / l, M + math.log2(l)


def split_and_combine(q, k, v, S):
  q = np.asarray(q, dtype=np.float64)
  parts = [partial(q, k[a:b], v[a:b]) for a, b in split_ranges(len(k), S)]
  return combine(parts, q.shape[0])
