"""References for the cache-extension attention kernel (plm_attn_extend): the staircase mask of a chunk of n query rows appended at
offset lens0 (row r < c sees key j iff j <= lens0 + r; rows r >= c see nothing), the unsplit masked softmax of every chunk row in fp64,
and a numpy restatement of what the kernel does instead - cut the sequence's keys 0 .. lens0 + c - 1 into S contiguous ranges with
plm_attn_decode's rule (tests/decode_ref.py), keep a base-2 partial (m, l, acc) per (row, range) under the mask, combine the partials of
a row in split order skipping the empty ones."""

import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_ref as R  # noqa: E402


def n_keys(lens0, c, Tmax=None):
  """Keys the sequence holds once the chunk is appended: lens0 + c, at most Tmax."""
  L = lens0 + c
  return L if Tmax is None else min(L, Tmax)


def staircase(lens0, c, n, L):
  """bool [n, L]: row r may see key j.  Rows r >= c are all False."""
  r = np.arange(n)[:, None]
  j = np.arange(L)[None, :]
  return (j <= lens0 + r) & (r < c)


def chunk_attention(q, k, v, lens0, c):
  """q [n, hd], k / v [>= lens0 + c, hd] -> (out [n, hd], lse2 [n]): the masked softmax of every chunk row in fp64, unsplit.  Rows r >= c:
  out = 0, lse2 = +inf.  Keys at and beyond lens0 + c are never touched (they may hold NaN)."""
  q = np.asarray(q, dtype=np.float64)
  n, hd = q.shape
  out, lse = np.zeros((n, hd)), np.full(n, math.inf)
  for r in range(min(c, n)):
    out[r], lse[r] = R.attn_row(q[r], k[:lens0 + r + 1], v[:lens0 + r + 1])
  return out, lse


def split_and_combine(q, k, v, lens0, c, S):
  """The kernel's route: S ranges over keys 0 .. lens0 + c - 1, one partial per (row, range) under the staircase, the combine of
  tests/decode_ref.py per row (m = -inf partials skipped; no partial at all: out = 0, lse2 = +inf)."""
  q = np.asarray(q, dtype=np.float64)
  n, hd = q.shape
  L = n_keys(lens0, min(c, n))
  mask = staircase(lens0, c, n, L)
  ranges = R.split_ranges(L, S)
  out, lse = np.zeros((n, hd)), np.full(n, math.inf)
  for r in range(n):
    parts = []
    for a, b in ranges:
      sel = np.arange(a, b)[mask[r, a:b]]
      parts.append(R.partial(q[r], np.asarray(k)[sel], np.asarray(v)[sel]))
    out[r], lse[r] = R.combine(parts, hd)
  return out, lse
