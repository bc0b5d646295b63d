"""KV-cached generation (DESIGN.md sections 12 and 14): the cache, and the host logic of ``Transformer.prefill / decode_step / extend /
generate`` (``extend``: a chunk of tokens per sequence on top of a live cache).

Everything that can be stated without a GPU lives here as plain functions over tensors on any device - the length checks, the choice of
the row a padded prompt is continued from, the token loop with its EOS freezing - so that tests/test_decode_host.py runs them on the CPU
with a fake step function.  The kernels are reached through two ops per cached step from transformer.py: ops.kv_append_rope /
ops.attn_decode for one token per sequence, ops.kv_append_rope_rows / ops.attn_extend for a chunk.  On-device
sampling adds the argument rules (check_sampling), the one draw of uniforms per call (draw_uniforms) and the
per-step pick (sampling_pick over ops.sample_logits).  Speculative decoding adds the host logic of
``Transformer.generate_speculative``: its refusals (check_speculative), greedy acceptance (greedy_accept), the bookkeeping of a round
(commit_round), the round loop over callables (speculative_loop) and the one draw of all its uniforms (speculative_uniforms).
"""

import math

import torch

from . import ops

FINISH_CHECK_EVERY = 16  # generate: the one device-to-host read of the loop (have all sequences emitted eos_id?) at most this often


class KVCache:
  """Per-layer ``kv`` bf16 [B, Tmax, 2*dim] (row (b, j): the k | v columns of token j's rotated qkv row), ``lens`` int32 [B] on the
  device, and the status flag of the append kernel (checked by ``check``).  It owns no workspace: ops.attn_decode / ops.attn_extend take
  theirs from the workspace arena of the current stream."""

  def __init__(self, n_layers, B, Tmax, n_heads, head_dim, device):
    dim = n_heads * head_dim
    self.B, self.Tmax, self.n_heads, self.head_dim = B, Tmax, n_heads, head_dim
    self.kv = [torch.empty((B, Tmax, 2 * dim), dtype=torch.bfloat16, device=device) for _ in range(n_layers)]  # rows >= lens are never read
    # [pos | lens] = [lens - 1 | lens] during a decode step: one in-place add per step moves both, every layer reads the same pair
    self._pl = torch.zeros((2, B), dtype=torch.int32, device=device)
    self._pl[0] -= 1
    self.status = torch.zeros((1,), dtype=torch.int32, device=device)

  @property
  def lens(self):
    return self._pl[1]

  @property
  def pos(self):
    """Position of the token appended by the current decode step (lens - 1)."""
    return self._pl[0]

  def set_lens(self, lens):
    self._pl[1].copy_(lens)
    self._pl[0].copy_(lens - 1)

  def advance(self):
    self._pl += 1

  def advance_by(self, n_new):
    """Move [pos | lens] by n_new - an int32 [B] device tensor, or an int - with one in-place add (Transformer.extend, after its chunk)."""
    self._pl += n_new

  def check(self):
    """Raises if a decode step tried to append past the cache (or past the RoPE table); reads the device flag, so it waits for the GPU."""
    if int(self.status.item()) != 0:
      raise RuntimeError(f'KVCache: a decode step appended at a position outside [0, {self.Tmax}): that token was not stored '
                         '(prefill with a larger max_len)')


def chunk_lens(token_lens, B, n, device):
  """token_lens of Transformer.extend as (what advance_by takes, the int32 [B] device tensor the kernels take or None for "n
  everywhere").  None: every sequence appends all n tokens.  Host integers (a sequence of B ints in [0, n], or a CPU tensor) are checked
  here and copied to the device; an int32 [B] device tensor is never read back: it is clamped to [0, n] on the device (as the kernels
  clamp it), so that the lengths move by what was appended and the gather of the last rows stays inside the chunk."""
  if token_lens is None:
    return int(n), None
  if isinstance(token_lens, torch.Tensor) and token_lens.device.type != 'cpu':
    if token_lens.dtype != torch.int32 or tuple(token_lens.shape) != (B,):
      raise TypeError(f'extend: a device token_lens must be an int32 [{B}] tensor, got {token_lens.dtype} {tuple(token_lens.shape)}')
    t = token_lens.clamp(0, int(n))
    return t, t
  vals = token_lens.tolist() if isinstance(token_lens, torch.Tensor) else list(token_lens)
  vals = [int(v) for v in vals]
  if len(vals) != B:
    raise ValueError(f'extend: {len(vals)} token_lens for a batch of {B}')
  if any(v < 0 or v > n for v in vals):
    raise ValueError(f'extend: every token_lens must be in [0, {n}] (the token tensor\'s width), got {vals}')
  t = torch.tensor(vals, dtype=torch.int32).to(device)
  return t, t


def pad4(n):
  return (int(n) + 3) // 4 * 4


def prompt_lens_list(prompt_lens, B, T):
  """prompt_lens (None | a sequence of ints | an integer tensor on the host) as a list of B ints in [1, T]."""
  if prompt_lens is None:
    return [int(T)] * B
  if isinstance(prompt_lens, torch.Tensor):
    if prompt_lens.is_cuda:
      raise TypeError('prompt_lens: pass host integers (a list, a tuple or a CPU tensor): they size the cache before anything is launched')
    prompt_lens = prompt_lens.tolist()
  lens = [int(v) for v in prompt_lens]
  if len(lens) != B:
    raise ValueError(f'prompt_lens: {len(lens)} lengths for a batch of {B}')
  if any(v < 1 or v > T for v in lens):
    raise ValueError(f'prompt_lens: every length must be in [1, {T}] (the prompt tensor\'s width), got {lens}')
  return lens


def check_lengths(T, max_new_tokens, seq_len):
  """The refusals of generate that need no GPU; returns the cache length (the padded prompt must fit it too)."""
  if int(max_new_tokens) < 1:
    raise ValueError(f'generate: max_new_tokens must be at least 1, got {max_new_tokens}')
  if T < 1:
    raise ValueError('generate: empty prompt')
  if T + int(max_new_tokens) > seq_len:
    raise ValueError(f'generate: prompt length {T} + max_new_tokens {max_new_tokens} exceeds cfg.seq_len {seq_len}')
  return max(pad4(T), T + int(max_new_tokens))


def last_rows(y, B, T, lens):
  """Rows lens[b] - 1 of every sequence of y [B*T, d] -> [B, d]: what a right-padded prompt is continued from (NOT the padded last row)."""
  idx = torch.arange(B, device=y.device) * T + (lens.to(device=y.device, dtype=torch.int64) - 1)
  return y.index_select(0, idx)


def generate_loop(first, step, max_new_tokens, eos_id=None, all_done=None, check_every=FINISH_CHECK_EVERY):
  """The token loop.  ``first`` = (tokens int64 [B], logprob fp32 [B]) from the prefill; ``step(tokens) -> (tokens, logprob)`` is one
  decode step.  Returns (tokens [B, N], logprobs [B, N]).  After a sequence has emitted eos_id its later tokens are eos_id with
  log-probability 0 (its steps still run: the batch stays rectangular).  Nothing is read back per token; ``all_done(done)`` - the one
  device-to-host read - runs at most once every ``check_every`` steps and ends the loop early."""
  tok, lp = first
  toks, lps = [tok], [lp]
  done = (tok == eos_id) if eos_id is not None else None
  if all_done is None:
    all_done = lambda d: bool(d.all())  # noqa: E731
  for i in range(1, int(max_new_tokens)):
    if done is not None and i % check_every == 0 and all_done(done):
      rest = int(max_new_tokens) - i
      toks += [torch.full_like(tok, eos_id)] * rest
      lps += [torch.zeros_like(lp)] * rest
      break
    tok, lp = step(tok)
    if done is not None:
      tok = torch.where(done, torch.full_like(tok, eos_id), tok)
      lp = torch.where(done, torch.zeros_like(lp), lp)
      done = done | (tok == eos_id)
    toks.append(tok)
    lps.append(lp)
  return torch.stack(toks, dim=1), torch.stack(lps, dim=1)


def sampled(sample, logits):
  """(tokens int64 [B], log p(tokens) fp32 [B]) from the caller's sampler on fp32 logits [B, V]."""
  lf = logits.float()
  tok = sample(lf)
  if not isinstance(tok, torch.Tensor) or tok.dtype != torch.int64 or tuple(tok.shape) != (lf.shape[0],):
    raise TypeError('generate: sample(logits fp32 [B, V]) must return an int64 [B] tensor')
  tok = tok.to(lf.device)
  return tok, torch.log_softmax(lf, dim=-1).gather(1, tok[:, None])[:, 0]


def check_sampling(temperature=None, top_k=None, top_p=None, sample=None, seed=None):
  """The sampling arguments of generate, normalised: None when the call is greedy or goes through the caller's ``sample``, else
  (temperature, top_k, top_p) for ops.sample_logits.  top_k None is 0 (off), top_p None is 1 (off); temperature None or 0 with neither
  filter is greedy, temperature None with a filter is 1.  Refused with ValueError: ``sample`` together with any of the other four, a
  negative or non-finite temperature, temperature 0 together with a filter (that is greedy: say so by leaving the filters out), top_k < 0,
  top_p outside (0, 1]."""
  if sample is not None:
    given = [n for n, v in (('temperature', temperature), ('top_k', top_k), ('top_p', top_p), ('seed', seed)) if v is not None]
    if given:
      raise ValueError(f'generate: sample= is the caller\'s own sampler; it cannot be combined with {", ".join(given)}')
    return None
  k = 0 if top_k is None else int(top_k)
  p = 1.0 if top_p is None else float(top_p)
  if k < 0:
    raise ValueError(f'generate: top_k must be >= 0 (0 or None = off), got {top_k}')
  if not (0.0 < p <= 1.0):
    raise ValueError(f'generate: top_p must be in (0, 1] (1 or None = off), got {top_p}')
  t = None if temperature is None else float(temperature)
  if t is not None and (not math.isfinite(t) or t < 0.0):
    raise ValueError(f'generate: temperature must be finite and >= 0, got {temperature}')
  filtered = k > 0 or p < 1.0
  if t is None or t == 0.0:
    if not filtered:
      return None  # greedy: the fused prediction head, no logits
    if t is not None:
      raise ValueError('generate: temperature 0 is greedy decoding, which top_k / top_p cannot change: leave them out, or give a positive temperature')
    t = 1.0
  return t, k, p


def draw_uniforms(max_new_tokens, B, device, seed=None):
  """u fp32 [max_new_tokens, B] on ``device``, drawn once per generate call: step n uses row n.  ``seed`` seeds a torch.Generator of
  that device (the same seed gives the same bits); None draws from torch's default generator."""
  gen = None
  if seed is not None:
    gen = torch.Generator(device=device)
    gen.manual_seed(int(seed))
  return torch.rand((int(max_new_tokens), int(B)), generator=gen, dtype=torch.float32, device=device)


def sampling_pick(u, temperature, top_k, top_p, sampler=None):
  """pick(logits bf16 [B, V]) -> (tokens, logprob) for generate_loop: its n-th call samples with row n of u, through ops.sample_logits
  (``sampler`` stands in for it in the host tests)."""
  sampler = ops.sample_logits if sampler is None else sampler
  n = [0]

  def pick(logits):
    r = sampler(logits, u[n[0]], temperature, top_k, top_p)
    n[0] += 1
    return r[0], r[1]
  return pick


# ---- speculative decoding ---------------------------------------------------------------------------------------
MAX_DRAFT = 31  # a chunk of n_draft + 1 <= 32 rows is one wave's queries in attn_extend_kernel; plm_spec_verify_bf16 holds the same limit


def check_speculative(T, max_new_tokens, n_draft, cfg, draft_cfg, device=None, draft_device=None, temperature=None, top_k=None, top_p=None,
                      seed=None, sample=None):
  """The refusals of generate_speculative that need no GPU.  cfg / draft_cfg: the two models' ModelConfig.  Returns (cache rows per
  sequence - the same for both models -, check_sampling's normalised (temperature, top_k, top_p) or None for greedy).  A round may write
  n_draft + 1 rows past the last token a sequence keeps, hence the longer cache."""
  if sample is not None:
    raise ValueError('generate_speculative: sample= callables are not supported (the acceptance rule needs both models\' distributions on the '
                     'device): use temperature / top_k / top_p, or generate()')
  if isinstance(n_draft, bool) or not isinstance(n_draft, int):
    raise TypeError(f'generate_speculative: n_draft must be an int, got {type(n_draft).__name__}')
  if n_draft < 1 or n_draft > MAX_DRAFT:
    raise ValueError(f'generate_speculative: n_draft must be in [1, {MAX_DRAFT}], got {n_draft}')
  if draft_cfg.vocab_size != cfg.vocab_size:
    raise ValueError(f'generate_speculative: the draft\'s vocab_size {draft_cfg.vocab_size} is not the target\'s {cfg.vocab_size}')
  if device is not None and draft_device is not None and torch.device(device) != torch.device(draft_device):
    raise ValueError(f'generate_speculative: the draft is on {draft_device}, the target on {device}')
  if int(max_new_tokens) < 1:
    raise ValueError(f'generate_speculative: max_new_tokens must be at least 1, got {max_new_tokens}')
  if T < 1:
    raise ValueError('generate_speculative: empty prompt')
  need = T + int(max_new_tokens) + n_draft + 1
  for who, c in (('the target', cfg), ('the draft', draft_cfg)):
    if need > c.seq_len:
      raise ValueError(f'generate_speculative: prompt length {T} + max_new_tokens {max_new_tokens} + n_draft {n_draft} + 1 exceeds '
                       f'{who}\'s cfg.seq_len {c.seq_len}')
  return need, check_sampling(temperature, top_k, top_p, None, seed)


def greedy_accept(draft_tok, target_pred):
  """Greedy acceptance: draft_tok int64 [B, k], target_pred int64 [B, k + 1] (row r: the target's prediction after the round's first r + 1
  tokens).  Returns (n_accept int32 [B] = the number of leading draft tokens the target predicts too, next_token int64 [B] = the target's
  prediction at the first mismatch, or at row k).  Integer ops only, any device."""
  k = draft_tok.shape[1]
  n = (draft_tok == target_pred[:, :k]).to(torch.int32).cumprod(dim=1).sum(dim=1)
  return n.to(torch.int32), target_pred.gather(1, n.to(torch.int64)[:, None])[:, 0]


def commit_round(out_tok, out_lp, count, done, draft_tok, n_accept, next_tok, logp, eos_id=None):
  """The bookkeeping of one round, plain tensor ops on any device.  out_tok int64 [B, N] / out_lp fp32 [B, N] are updated in place;
  count int [B] (tokens emitted so far) and done bool [B] are not.  The round offers sequence b the tokens draft_tok[b, :n_accept[b]]
  followed by next_tok[b], with log-probabilities logp[b, :n_accept[b] + 1]; a live sequence takes them at columns count[b] .., cut at N
  and after the first eos_id, a finished one takes nothing.  A sequence that has emitted eos_id holds eos_id with log-probability 0 from
  there on, as generate_loop leaves it.  Returns (count, done, moved): the new counts and flags, and moved int32 [B] = the number of tokens
  each sequence took - how far its caches move."""
  B, N = out_tok.shape
  k = draft_tok.shape[1]
  dev = out_tok.device
  j = torch.arange(k + 1, device=dev)[None, :]
  na = n_accept.to(torch.int64)[:, None]
  cand = torch.where(j < na, torch.nn.functional.pad(draft_tok, (0, 1)), next_tok[:, None])
  m = torch.minimum(na[:, 0] + 1, N - count.to(torch.int64))
  m = torch.where(done, torch.zeros_like(m), m)
  if eos_id is not None:  # cut after the first eos_id among the tokens taken
    is_eos = (cand == eos_id) & (j < m[:, None])
    hit = is_eos.any(dim=1)
    m = torch.where(hit, is_eos.to(torch.int32).argmax(dim=1) + 1, m)
  pos = torch.arange(N, device=dev)[None, :] - count.to(torch.int64)[:, None]  # column n of the outputs is round entry pos[b, n]
  take = (pos >= 0) & (pos < m[:, None])
  src = pos.clamp(0, k)
  out_tok.copy_(torch.where(take, cand.gather(1, src), out_tok))
  out_lp.copy_(torch.where(take, logp.gather(1, src), out_lp))
  new_count = count + m.to(count.dtype)
  new_done = done | (new_count >= N)
  if eos_id is not None:
    new_done = new_done | hit
    tail = new_done[:, None] & (pos >= m[:, None])  # nothing for a sequence that filled up: it has no column left
    out_tok.masked_fill_(tail, eos_id)
    out_lp.masked_fill_(tail, 0.0)
  return new_count, new_done, m.to(torch.int32)


def speculative_loop(first, draft_round, target_round, accept, max_new_tokens, n_draft, eos_id=None, advance=None, all_done=None):
  """The round loop of speculative decoding over callables (tests/test_spec_host.py runs it on the CPU with fake models).
    first                                       (tokens int64 [B], logprob fp32 [B]) of the target's prefill
    draft_round(last, carry_tok, carry, live)   -> (draft_tok int64 [B, k], whatever accept needs of the draft).  last [B]: every
                                                sequence's newest token; carry bool [B]: the draft has not seen carry_tok [B] yet (the
                                                last draft token of a round that accepted all k), which then precedes ``last``
    target_round(last, draft_tok, live)         -> whatever accept needs of the target's k + 1 chunk rows
    accept(draft_tok, draft_out, target_out)    -> (n_accept [B], next_token [B], logprob [B, k + 1])
    advance(moved, live)                        moves the caches: moved int32 [B] from commit_round (0 for a finished sequence); a live
                                                sequence's draft cache keeps min(moved, k) of the round's rows
  Returns (tokens [B, N], logprobs [B, N], stats) with stats = dict(rounds, drafted int64 [B], accepted int64 [B]) over the rounds a
  sequence was live in.  A round emits at least one token per live sequence, so there are at most N - 1 rounds.  ``all_done(done)`` - the
  one device-to-host read, one int32 per round - ends the loop."""
  tok, lp = first
  N, k = int(max_new_tokens), int(n_draft)
  B, dev = tok.shape[0], tok.device
  out_tok = torch.zeros((B, N), dtype=torch.int64, device=dev)
  out_lp = torch.zeros((B, N), dtype=torch.float32, device=dev)
  out_tok[:, 0] = tok
  out_lp[:, 0] = lp
  count = torch.ones((B,), dtype=torch.int32, device=dev)
  done = torch.full((B,), N <= 1, dtype=torch.bool, device=dev)
  if eos_id is not None:
    done = done | (tok == eos_id)
    out_tok[:, 1:] = torch.where(done[:, None], torch.full_like(out_tok[:, 1:], eos_id), out_tok[:, 1:])
  if all_done is None:
    all_done = lambda d: bool(d.all())  # noqa: E731
  last, carry_tok = tok, tok
  carry = torch.zeros((B,), dtype=torch.bool, device=dev)
  drafted = torch.zeros((B,), dtype=torch.int64, device=dev)
  accepted = torch.zeros((B,), dtype=torch.int64, device=dev)
  rounds = 0
  while rounds < N - 1 and not all_done(done):
    live = ~done
    draft_tok, draft_out = draft_round(last, carry_tok, carry, live)
    n_accept, next_tok, logp = accept(draft_tok, draft_out, target_round(last, draft_tok, live))
    count, done, moved = commit_round(out_tok, out_lp, count, done, draft_tok, n_accept, next_tok, logp, eos_id)
    if advance is not None:
      advance(moved, live)
    carry = live & (moved == k + 1)
    carry_tok = draft_tok[:, k - 1]
    last = torch.where(live, next_tok, last)
    drafted += live.to(torch.int64) * k
    accepted += torch.where(live, n_accept.to(torch.int64), torch.zeros_like(accepted))
    rounds += 1
  return out_tok, out_lp, dict(rounds=rounds, drafted=drafted, accepted=accepted)


def uniforms_per_round(k):
  """Uniforms a round uses per sequence: k draft draws, k + 1 draws of the target's sampler, k acceptance tests, one residual draw."""
  return 3 * k + 2


def speculative_uniforms(max_new_tokens, n_draft, B, device, seed=None):
  """All uniforms of one generate_speculative call, drawn once through draw_uniforms: fp32 [1 + (N - 1) * (3k + 2), B].  Row 0 draws the
  first token; round i owns the next 3k + 2 rows (``round_uniforms``).  Every entry is used at most once, so the four roles are
  independent of one another."""
  return draw_uniforms(1 + (int(max_new_tokens) - 1) * uniforms_per_round(int(n_draft)), B, device, seed)


def round_uniforms(u, i, n_draft):
  """Round i's rows of ``speculative_uniforms``: (draft draws [k, B], target sampler's [k + 1, B], acceptance [k, B], residual [B])."""
  k = int(n_draft)
  r = u[1 + i * uniforms_per_round(k):1 + (i + 1) * uniforms_per_round(k)]
  return r[:k], r[k:2 * k + 1], r[2 * k + 1:3 * k + 1], r[3 * k + 1]
