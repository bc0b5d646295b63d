"""KV-cached generation (DESIGN.md sections 12 and 14): the cache, and the host logic of ``Transformer.prefill / decode_step / extend /
generate`` (``extend``: a chunk of tokens per sequence on top of a live cache).

Everything that can be stated without a GPU lives here as plain functions over tensors on any device - the length checks, the choice of
the row a padded prompt is continued from, the token loop with its EOS freezing - so that tests/test_decode_host.py runs them on the CPU
with a fake step function.  The kernels are reached through two ops per cached step from transformer.py: ops.kv_append_rope /
ops.attn_decode for one token per sequence, ops.kv_append_rope_rows / ops.attn_extend for a chunk.  On-device
sampling adds the argument rules (check_sampling), the one draw of uniforms per call (draw_uniforms) and the
per-step pick (sampling_pick over ops.sample_logits).
"""

import math

import torch

from . import ops

FINISH_CHECK_EVERY = 16  # generate: the one device-to-host read of the loop (have all sequences emitted eos_id?) at most this often


class KVCache:
  """Per-layer ``kv`` bf16 [B, Tmax, 2*dim] (row (b, j): the k | v columns of token j's rotated qkv row), ``lens`` int32 [B] on the
  device, the attention workspaces (shared by all layers), and the status flag of the append kernel (checked by ``check``)."""

  def __init__(self, n_layers, B, Tmax, n_heads, head_dim, device):
    dim = n_heads * head_dim
    self.B, self.Tmax, self.n_heads, self.head_dim = B, Tmax, n_heads, head_dim
    self.kv = [torch.empty((B, Tmax, 2 * dim), dtype=torch.bfloat16, device=device) for _ in range(n_layers)]  # rows >= lens are never read
    # [pos | lens] = [lens - 1 | lens] during a decode step: one in-place add per step moves both, every layer reads the same pair
    self._pl = torch.zeros((2, B), dtype=torch.int32, device=device)
    self._pl[0] -= 1
    self.status = torch.zeros((1,), dtype=torch.int32, device=device)
    # (workspace, bytes) pairs at the automatic split count: key 0 is ops.attn_decode's, made here; key n >= 1 ops.attn_extend's for
    # chunks of n rows, made at the first extend of that width
    self._ws = {0: ops.attn_decode_workspace(B, n_heads, head_dim, Tmax, 0, device)}

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

  @property
  def workspace(self):
    """The (workspace, bytes) pair of ops.attn_decode."""
    return self._ws[0]

  def extend_workspace(self, n):
    """The (workspace, bytes) pair of ops.attn_extend for chunks of n rows: allocated at the first chunk of that width and kept."""
    ws = self._ws.get(n)
    if ws is None:
      ws = self._ws[n] = ops.attn_extend_workspace(self.B, n, self.n_heads, self.head_dim, self.Tmax, 0, self.status.device)
    return ws

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
