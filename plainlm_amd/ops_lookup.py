"""The ops wrappers of draft-free speculative decoding: ``ops.lookup_draft`` and ``ops.spec_verify_lookup``.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract - the same operand validator (``ops._need``), the
same pointer and stream plumbing, ``_lib.check`` around the one library call - and, like every wrapper there, launch hand-written gfx950
kernels with no torch fallback.  They live in a module of their own because tests/test_ops_trace_host.py holds every function defined in
ops.py to a trace recorded on an earlier commit, which a new wrapper cannot have; tests/test_lookup_host.py records theirs against the
same fakes."""

import collections

import torch

from . import _lib
from . import ops as O

LookupDraft = collections.namedtuple('LookupDraft', ['draft_tokens', 'n_prop', 'match_len'])


def lookup_draft(hist, lens, add_tok=None, n_add=None, k=8, ngram=(1, 4), status=None):
  """Prompt-lookup drafting (include/plainlm_hip.h states the rule): hist int64 [B, ld] and lens int32 [B] are every
  sequence's token history and its length, both updated in place.  add_tok int64 [B, ld_add] / n_add int32 [B] (None: all ld_add) are
  appended first; then sequence b proposes the k tokens that followed the most recent, longest (g_min .. g_max tokens, ``ngram``) earlier
  occurrence of its last tokens.  A sequence whose append does not fit ld stores nothing and sets status[0] = 1 (int32 [1], zeroed by the
  caller; made here when absent - read it from the ``status`` the caller passed).  One launch, integers only, nothing is read back.  Returns the
  named tuple (draft_tokens int64 [B, k], n_prop int32 [B] = k or 0, match_len int32 [B]); a row without a proposal is zeros."""
  O._need(hist, torch.int64, 'lookup_draft.hist', 2)
  B, ld = hist.shape
  g_min, g_max = ngram
  for t, dtype, shape, name in ((lens, torch.int32, (B,), 'lens'), (add_tok, torch.int64, None, 'add_tok'), (n_add, torch.int32, (B,), 'n_add'),
                                (status, torch.int32, (1,), 'status')):
    if t is not None:
      O._need(t, dtype, f'lookup_draft.{name}')
      if shape is not None and tuple(t.shape) != shape:
        raise ValueError(f'lookup_draft: {name} {tuple(t.shape)} is not {shape} (hist {tuple(hist.shape)})')
  if add_tok is None and n_add is not None:
    raise ValueError('lookup_draft: n_add without add_tok')
  if add_tok is not None and (add_tok.dim() != 2 or add_tok.shape[0] != B):
    raise ValueError(f'lookup_draft: add_tok {tuple(add_tok.shape)} is not [B, n] for hist {tuple(hist.shape)}')
  dev = hist.device
  status = torch.zeros((1,), dtype=torch.int32, device=dev) if status is None else status
  draft = torch.empty((B, int(k)), dtype=torch.int64, device=dev)
  n_prop = torch.empty((B,), dtype=torch.int32, device=dev)
  match_len = torch.empty((B,), dtype=torch.int32, device=dev)
  _lib.check(_lib.load().plm_lookup_draft_i64(O._p(hist), ld, O._p(lens), O._p(add_tok), 0 if add_tok is None else add_tok.shape[1], O._p(n_add),
                                              O._p(draft), O._p(n_prop), O._p(match_len), O._p(status), B, int(k), int(g_min), int(g_max), O._stream()),
             'plm_lookup_draft_i64')
  return LookupDraft(draft, n_prop, match_len)


def spec_verify_lookup(target_logits, draft_tokens, n_prop, target_cutoff, target_tokens, u_accept, u_resid, temperature=1.0):
  """The acceptance rule of ``spec_verify`` for a deterministic draft (include/plainlm_hip.h states the rule): the
  draft is one-hot on the proposed token, so a row is accepted with probability p(x) and a rejected one draws from p with x removed - in
  the sampler's integers, without a quotient.  target_logits bf16 [B*(k+1), V], row b*(k+1) + r, unit inner stride and any row stride >= V;
  draft_tokens int64 [B, k] and n_prop int32 [B] (rows at and beyond n_prop[b] hold no proposal and are never loaded): ops.lookup_draft's;
  target_cutoff fp32 [B*(k+1)] and target_tokens int64 [B*(k+1)]: ops.sample_logits(..., want_stats=True) on those rows at this temperature;
  u_accept fp32 [k, B], u_resid fp32 [B].  Two launches, bit-reproducible, nothing is read back.  Returns ops.SpecVerify (n_accept int32 [B] <=
  n_prop, next_token int64 [B], logprob fp32 [B, k+1], 0 beyond entry n_accept)."""
  O._need(draft_tokens, torch.int64, 'spec_verify_lookup.draft_tokens', 2)
  B, k = draft_tokens.shape
  ldp = O._logits_rows(target_logits, B * (k + 1), 'spec_verify_lookup.target_logits')
  V = target_logits.shape[1]
  for t, dtype, n, name in ((n_prop, torch.int32, B, 'n_prop'), (target_cutoff, O.F32, B * (k + 1), 'target_cutoff'),
                            (target_tokens, torch.int64, B * (k + 1), 'target_tokens'), (u_accept, O.F32, k * B, 'u_accept'),
                            (u_resid, O.F32, B, 'u_resid')):
    O._need(t, dtype, f'spec_verify_lookup.{name}')
    if t.numel() != n:
      raise ValueError(f'spec_verify_lookup: {name} {tuple(t.shape)} does not hold {n} elements (B={B}, k={k})')
  dev = target_logits.device
  n_accept = torch.empty((B,), dtype=torch.int32, device=dev)
  next_tok = torch.empty((B,), dtype=torch.int64, device=dev)
  logp = torch.empty((B, k + 1), dtype=O.F32, device=dev)
  _lib.check(_lib.load().plm_spec_verify_lookup_bf16(O._p(target_logits), ldp, O._p(draft_tokens), O._p(n_prop), O._p(target_cutoff), O._p(target_tokens),
                                                     O._p(u_accept), O._p(u_resid), float(temperature), O._p(n_accept), O._p(next_tok), O._p(logp), B, k, V,
                                                     O._stream()), 'plm_spec_verify_lookup_bf16')
  return O.SpecVerify(n_accept, next_tok, logp)
