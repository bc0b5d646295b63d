"""The sampling rule of DESIGN.md section 13 (include/plainlm_hip.h) restated in fp64 numpy, for whole batches at once.

  temperature  w_i = exp((x_i - x_max) / tau); a NaN or infinite logit has weight 0, is never kept and never chosen
  top-k        by value: every i with x_i >= v_k, v_k the k-th largest value (all ties with it stay); k = 0 or k >= V is off
  top-p        by value class: t* = the largest value present among the top-k survivors with mass(t*) >= top_p, where mass(t) is the
               survivors' softmax mass at x >= t; every survivor with x_i >= t* stays
  draw         over the kept columns in ascending index order: the lowest kept i with C_i > u * Z (C the running sum of w, Z its end);
               if rounding leaves none, the last kept i with w_i > 0; u is clamped: NaN or negative -> 0, >= 1 -> the float below 1

`Rows(x)` sorts once (the expensive part, independent of tau / top_k / top_p); `keep_set` and `draw` are cheap per configuration."""

import numpy as np

U_MAX = float(np.nextafter(np.float32(1.0), np.float32(0.0)))  # the largest float below 1


class Rows:
  """x float64 [B, V]: the values of bf16 logits (NaN and infinities allowed).  Never modified."""

  def __init__(self, x):
    x = np.asarray(x, dtype=np.float64)
    self.x, (self.B, self.V) = x, x.shape
    self.valid = np.isfinite(x)
    xs = np.where(self.valid, x, -np.inf)
    self.order = np.argsort(-xs, axis=1, kind='stable')  # descending by value; non-finite entries last
    self.sx = np.take_along_axis(xs, self.order, 1)
    self.nvalid = self.valid.sum(1)
    self.xmax = self.sx[:, 0].copy()                     # -inf for a row without a finite logit
    self.class_end = np.ones(x.shape, dtype=bool)        # sorted position j is the last of its value class
    self.class_end[:, :-1] = self.sx[:, :-1] != self.sx[:, 1:]
    with np.errstate(invalid='ignore', divide='ignore'):
      self.d = np.where(self.valid, x - self.xmax[:, None], -np.inf)  # x - x_max, -inf where the weight is 0
      self.logp = np.where(self.valid, self.d - np.log(np.exp(self.d).sum(1))[:, None], np.nan)  # log softmax(x) at temperature 1

  def weights(self, tau):
    return np.exp(self.d / float(tau))

  def topk_value(self, top_k):
    """v_k per row (the lowest finite value when top-k is off or the row has fewer finite logits; +inf for a row with none)."""
    k = self.nvalid if not 0 < top_k < self.V else np.minimum(top_k, self.nvalid)
    vk = self.sx[np.arange(self.B), np.maximum(k, 1) - 1]
    return np.where(self.nvalid > 0, vk, np.inf)

  def keep_set(self, tau, top_k, top_p, w=None):
    """dict: keep bool [B, V], n_kept [B], cutoff [B] (NaN for an empty set), surv (the top-k survivors), w, vk."""
    w = self.weights(tau) if w is None else w
    vk = self.topk_value(top_k)
    surv = self.valid & (self.x >= vk[:, None])
    t = vk
    if top_p < 1:
      nsurv = surv.sum(1)
      sw = np.take_along_axis(w, self.order, 1)
      pos = np.arange(self.V)[None, :]
      sw = np.where(pos < nsurv[:, None], sw, 0.0)       # survivors are a prefix of the descending order
      cum = np.cumsum(sw, axis=1)
      zk = cum[:, -1:]
      with np.errstate(invalid='ignore', divide='ignore'):
        cand = self.class_end & (pos < nsurv[:, None]) & (cum >= top_p * zk)
      j = np.argmax(cand, axis=1)                        # the first class, from the top, that reaches top_p
      t = np.where(nsurv > 0, self.sx[np.arange(self.B), j], np.inf)
    keep = surv & (self.x >= t[:, None])
    n = keep.sum(1)
    return dict(keep=keep, n_kept=n, cutoff=np.where(n > 0, t, np.nan), surv=surv, w=w, vk=vk)

  def running(self, keep, w):
    """C [B, V]: running sum of the kept weights in index order (C[:, -1] = Z)."""
    return np.cumsum(np.where(keep, w, 0.0), axis=1)


def clamp_u(u):
  u = np.asarray(u, dtype=np.float64)
  u = np.where(u >= 0, u, 0.0)  # NaN and negative values
  return np.where(u < 1, u, U_MAX)


def draw(keep, w, C, u):
  """tok [B]: the lowest kept i with C_i > u * Z, else the last kept i with w_i > 0, else 0."""
  uz = clamp_u(u) * C[:, -1]
  hit = keep & (C > uz[:, None])
  tok = np.argmax(hit, axis=1)
  pos = keep & (w > 0)
  last = pos.shape[1] - 1 - np.argmax(pos[:, ::-1], axis=1)
  return np.where(hit.any(1), tok, np.where(pos.any(1), last, 0))


def sample(x, u, tau=1.0, top_k=0, top_p=1.0):
  """The whole rule: dict of keep_set plus tok [B], logp [B] (NaN for a row without a finite logit), C."""
  r = Rows(x)
  ks = r.keep_set(tau, top_k, top_p)
  C = r.running(ks['keep'], ks['w'])
  tok = draw(ks['keep'], ks['w'], C, u)
  ks.update(tok=tok, logp=r.logp[np.arange(r.B), tok], C=C)
  return ks
