"""The speculative-sampling acceptance rule of DESIGN.md section 15 (include/plainlm_hip.h, plm_spec_verify_bf16) restated in fp64 numpy,
on top of tests/sample_ref.py's definitions: a row's distribution is the sampler's - weight exp((x - x_max) / tau) on the kept set
{i : x_i finite and x_i >= cutoff}, 0 outside it - and u is clamped as the sampler clamps it.

  alpha     min(1, p(x) / q(x)); 0 when x is outside [0, V) or p(x) = 0; 1 when q(x) = 0 < p(x)
  accept    rows r = 0, 1, .. while u[r] < alpha_r
  residual  r_i = max(0, p_i - q_i) at the first rejected row, C its running sum in ascending column order, R = C[-1]; the draw is the
            sampler's: the lowest i with C_i > u_res * R; R = 0 falls back to the target sampler's own token of that row
  bonus     all k accepted: the target sampler's token of row k
  logp      log softmax over every finite logit of the target row, at temperature 1, of the token emitted there; 0 beyond n_accept"""

import numpy as np

import sample_ref as R


class Dist:
  """One row's warped distribution.  x float64 [V] (NaN and infinities allowed), cutoff: the kept set's lowest logit (NaN keeps nothing)."""

  def __init__(self, x, tau, cutoff):
    x = np.asarray(x, dtype=np.float64)
    self.V = x.shape[0]
    valid = np.isfinite(x)
    with np.errstate(invalid='ignore'):
      self.keep = valid & (x >= cutoff)
    self.xmax = x[valid].max() if valid.any() else -np.inf
    with np.errstate(invalid='ignore', over='ignore'):
      self.lnw = np.where(self.keep, (x - self.xmax) / float(tau), -np.inf)  # ln of the weight: -|d / tau|
    self.w = np.exp(self.lnw)
    self.Z = self.w.sum()
    self.prob = self.w / self.Z if self.Z > 0 else np.zeros_like(self.w)
    if valid.any():
      d = np.where(valid, x - self.xmax, -np.inf)
      self.logp = np.where(valid, d - np.log(np.exp(d).sum()), np.nan)
    else:
      self.logp = np.full(self.V, np.nan)


def alpha(P, Q, x):
  if not 0 <= x < P.V or P.prob[x] == 0:
    return 0.0
  if Q.prob[x] == 0:
    return 1.0
  return min(1.0, P.prob[x] / Q.prob[x])


def residual(P, Q):
  """(r [V], C [V]): max(0, p - q) and its running sum."""
  r = np.maximum(0.0, P.prob - Q.prob)
  return r, np.cumsum(r)


def draw(C, u):
  """The lowest i with C_i > u * R, or None when R = 0."""
  if C[-1] <= 0:
    return None
  hit = np.flatnonzero(C > float(R.clamp_u(u)) * C[-1])
  return int(hit[0]) if hit.size else None


def verify(P, Q, tok, p_tok, u_acc, u_res):
  """One sequence.  P: k + 1 Dist of the target's chunk rows, Q: k Dist of the draft's steps, tok [k] the drafted tokens, p_tok [k + 1]
  the target sampler's own tokens, u_acc [k], u_res scalar.  Returns (n_accept, next_tok, logp [k + 1])."""
  k = len(Q)
  ua = R.clamp_u(u_acc)
  n, logp = 0, np.zeros(k + 1)
  while n < k and ua[n] < alpha(P[n], Q[n], int(tok[n])):
    logp[n] = P[n].logp[int(tok[n])]
    n += 1
  nxt = int(p_tok[n])
  if n < k:
    i = draw(residual(P[n], Q[n])[1], u_res)
    nxt = nxt if i is None else i
  logp[n] = P[n].logp[nxt]
  return n, nxt, logp


def first_token_distribution(P0, Q0):
  """The distribution of the first token a round emits, in closed form: x is drafted with q(x) and accepted with alpha(x); otherwise the
  residual is drawn.  The rule is exact when this equals p."""
  V = P0.V
  a = np.array([alpha(P0, Q0, x) for x in range(V)])
  r, C = residual(P0, Q0)
  reject = 1.0 - (Q0.prob * a).sum()
  res = r / C[-1] if C[-1] > 0 else np.zeros(V)  # R = 0 only when p = q, where nothing is ever rejected
  return Q0.prob * a + reject * res
