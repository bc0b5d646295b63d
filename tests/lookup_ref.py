"""Draft-free speculative decoding (include/plainlm_hip.h) restated in numpy: the n-gram lookup draft of
plm_lookup_draft_i64 in integers, and the one-hot acceptance rule of plm_spec_verify_lookup_bf16 in fp64 on top of tests/sample_ref.py
and tests/spec_ref.py (a row's distribution is the sampler's: ``spec_ref.Dist``).

  draft     m(e) = the number of consecutive t = 1, 2, .. with hist[e - t] == hist[L - t], up to min(g_max, e), for every end e in
            [1, L - 1]; the winner has the largest m >= g_min and, among those, the largest e; the proposal is hist[e + (i mod (L - e))]
  alpha     p(x); 0 when x is outside [0, V) or outside the kept set
  accept    rows r = 0 .. n_prop - 1 while u[r] < alpha_r
  residual  p with column x set to 0, C its running sum in ascending column order, R = C[-1] = 1 - p(x); the draw is the sampler's: the
            lowest i with C_i > u_res * R; R = 0 falls back to the target sampler's own token of that row
  bonus     all n_prop accepted: the target sampler's token of row n_prop
  logp      as spec_ref states it"""

import numpy as np

import sample_ref as R


# ---- the draft ---------------------------------------------------------------------------------------------------------------------------
def match_len(h, L, e, g_max):
  m = 0
  while m < min(g_max, e) and h[e - 1 - m] == h[L - 1 - m]:
    m += 1
  return m


def draft(h, L, k, g_min, g_max):
  """One sequence: h the history (at least L entries).  Returns (tokens int64 [k], n_prop, match length)."""
  best = (0, 0)
  for e in range(1, L):
    m = match_len(h, L, e, g_max)
    if m >= g_min:
      best = max(best, (m, e))
  m, e = best
  if m == 0:
    return np.zeros(k, dtype=np.int64), 0, 0
  return np.array([h[e + i % (L - e)] for i in range(k)], dtype=np.int64), k, m


def draft_brute(h, L, k, g_min, g_max):
  """The same in other words: the longest suffix of h[:L] (g_max .. g_min tokens) that occurs earlier, at its most recent occurrence;
  the proposal is what followed, continued periodically through the proposal itself."""
  h = list(h[:L])
  for g in range(min(g_max, L - 1), g_min - 1, -1):
    suffix = h[L - g:]
    starts = [s for s in range(L - g) if h[s:s + g] == suffix]   # an earlier occurrence ends at s + g <= L - 1
    if starts:
      e = starts[-1] + g
      ext = list(h)
      for i in range(k):                                          # the overlapped copy, one token at a time
        ext.append(ext[e + i])
      return np.array(ext[L:], dtype=np.int64), k, g
  return np.zeros(k, dtype=np.int64), 0, 0


def lookup(hist, lens, add_tok, n_add, k, ngram):
  """The whole launch.  hist int64 [B, ld], lens int32 [B]; add_tok int64 [B, ld_add] or None, n_add int32 [B] or None.  Returns a dict
  of new arrays: hist, lens, draft [B, k], n_prop [B], match_len [B], status (0 or 1)."""
  hist, lens = np.array(hist, dtype=np.int64), np.array(lens, dtype=np.int32)
  B, ld = hist.shape
  out = dict(hist=hist, lens=lens, draft=np.zeros((B, k), dtype=np.int64), n_prop=np.zeros(B, dtype=np.int32),
             match_len=np.zeros(B, dtype=np.int32), status=0)
  for b in range(B):
    c = 0
    if add_tok is not None:
      c = add_tok.shape[1] if n_add is None else int(np.clip(n_add[b], 0, add_tok.shape[1]))
    L0 = int(lens[b])
    if L0 < 0 or L0 + c > ld:
      out['status'] = 1
      continue
    if c:
      hist[b, L0:L0 + c] = add_tok[b, :c]
    lens[b] = L0 + c
    out['draft'][b], out['n_prop'][b], out['match_len'][b] = draft(hist[b], L0 + c, k, *ngram)
  return out


# ---- one-hot acceptance --------------------------------------------------------------------------------------------------------------------
def alpha(P, x):
  return float(P.prob[x]) if 0 <= x < P.V else 0.0


def residual(P, x):
  """(r [V], C [V]): p with column x removed, and its running sum."""
  r = P.prob.copy()
  if 0 <= x < P.V:
    r[x] = 0.0
  return r, np.cumsum(r)


def draw(C, u):
  """The lowest i with C_i > u * R, or None when R = 0."""
  if C[-1] <= 0:
    return None
  hit = np.flatnonzero(C > float(R.clamp_u(u)) * C[-1])
  return int(hit[0]) if hit.size else None


def verify(P, tok, n_prop, p_tok, u_acc, u_res):
  """One sequence.  P: k + 1 ``spec_ref.Dist`` of the chunk rows, tok [k] the proposal, n_prop in [0, k] (clamped), p_tok [k + 1] the
  target sampler's own tokens, u_acc [k], u_res scalar.  Returns (n_accept, next_tok, logp [k + 1])."""
  k = len(tok)
  n_prop = int(np.clip(n_prop, 0, k))
  ua = R.clamp_u(u_acc)
  n, logp = 0, np.zeros(k + 1)
  while n < n_prop and ua[n] < alpha(P[n], int(tok[n])):
    logp[n] = P[n].logp[int(tok[n])]
    n += 1
  nxt = int(p_tok[n])
  if n < n_prop:
    i = draw(residual(P[n], int(tok[n]))[1], u_res)
    nxt = nxt if i is None else i
  logp[n] = P[n].logp[nxt]
  return n, nxt, logp


def first_token_distribution(P0, x):
  """The distribution of the first token of a round whose proposal is x, in closed form: x with probability p(x), else the residual."""
  a = alpha(P0, x)
  r, C = residual(P0, x)
  out = np.zeros(P0.V)
  if 0 <= x < P0.V:
    out[x] = a
  if C[-1] > 0:
    out += (1.0 - a) * r / C[-1]
  return out
