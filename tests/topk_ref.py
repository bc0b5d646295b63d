"""The CPU contract of the top-k head, in fp64 on the logits it is handed.  Non-finite logits are absent: lse is
the log-sum-exp of the finite entries (-inf for a row without one); the order is value descending, then index ascending (+0 == -0) over
the finite entries; tok holds its first k indices, -1 beyond them, logp = x[tok] - lse, -inf beyond them; rank is the target's 0-based
place in that order (-1 for a target outside [0, V), V for a target whose logit is not finite)."""
import torch


def topk_reference(logits, k, targets=None):
  """logits [M, V] (any float dtype) -> dict(tok int64 [M, k], logp fp64 [M, k], lse fp64 [M], rank int32 [M] or None)."""
  x = logits.detach().cpu().double()
  M, V = x.shape
  fin = torch.isfinite(x)
  low = torch.where(fin, x, torch.full_like(x, float('-inf')))
  lse = torch.logsumexp(low, dim=1)  # -inf for a row without a finite entry
  val, idx = torch.sort(low, dim=1, descending=True, stable=True)  # equal values keep index order; the absent entries go last
  n_fin = fin.sum(1, keepdim=True)
  keep = torch.arange(k)[None, :] < n_fin
  tok = torch.where(keep, idx[:, :k], torch.full((M, k), -1, dtype=torch.int64))
  logp = torch.where(keep, val[:, :k] - lse[:, None], torch.full((M, k), float('-inf'), dtype=torch.float64))
  rank = None
  if targets is not None:
    t = targets.detach().cpu()
    ok = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1)
    place = torch.argsort(idx, dim=1).gather(1, tc[:, None])[:, 0]  # where the sort put the target's column
    rank = torch.where(ok, torch.where(fin.gather(1, tc[:, None])[:, 0], place, torch.full_like(place, V)), torch.full_like(place, -1)).to(torch.int32)
  return dict(tok=tok, logp=logp, lse=lse, rank=rank)


def kth_place_ties(logits, k):
  """bool [M]: rows whose k-th and (k+1)-th largest finite logits are equal - the k-th place is decided by the index rule."""
  x = logits.detach().cpu().double()
  val = torch.sort(torch.where(torch.isfinite(x), x, torch.full_like(x, float('-inf'))), dim=1, descending=True).values
  return (val[:, k - 1] == val[:, k]) & torch.isfinite(val[:, k]) if x.shape[1] > k else torch.zeros(x.shape[0], dtype=torch.bool)
