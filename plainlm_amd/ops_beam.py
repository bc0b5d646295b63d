"""The ops wrappers of beam search on the shared-prefix cache: ``ops.attn_decode_beam`` (the G beams of a prompt
attend the prompt's prefix cache, then the suffix rows an ancestor table names - no cache row is ever copied), ``ops.decode_layer_beam`` (a
whole decode layer with that attention from one library call), ``ops.beam_select`` (the 2G best continuations per prompt, in a defined
order), ``ops.beam_advance`` (one step of the bookkeeping on ``BeamBuffers``) and ``ops.beam_finalize`` (the best hypotheses).

Operands as ops_shared.py's: P prompts, G <= BEAM_MAX beams each, row i = p*G + g.  anc uint8 [P*G, Ts_max]: anc[p*G+g][j] is the suffix
slot (0 .. G-1) of prompt p whose row j holds the j-th generated token of beam g's history.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract, as ops_shared.py states it."""

import torch

from . import _lib
from . import ops as O
from . import ops_shared as S

BEAM_MAX = 32  # beams per prompt: the N of one 32x32 MFMA tile in plm_attn_decode_beam, BEAM_MAX in csrc/beam.hip


def _need_anc(name, anc, M, Ts):
  try:
    O._need(anc, torch.uint8, 'anc', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  if tuple(anc.shape) != (M, Ts):
    raise ValueError(f'{name}: anc {tuple(anc.shape)} is not the uint8 [{M}, {Ts}] ancestor table of the suffix cache')


def _need_beams(name, G):
  if not 1 <= G <= BEAM_MAX:
    raise ValueError(f'{name}: {G} beams per prompt unsupported (1 .. {BEAM_MAX}: one MFMA tile of queries)')


def attn_decode_beam(q, kv_p, lens_p, kv_s, lens_s, anc, nh, splits_p=0, splits_s=0, want_lse=False):
  """Attention of one rotated query row per beam: q bf16 [P*G, nh*hd]; beam g of prompt p attends keys 0 .. lens_p[p]-1 of kv_p[p], then,
  for j < lens_s[p*G], row j of kv_s[p*G + anc[p*G+g][j]] (an entry >= G names no slot; rows and table entries at and beyond lens_s are
  never read; lens_s = 0 gives the prefix-only result).  G <= BEAM_MAX.  Returns out bf16 [P*G, nh*hd], or (out, lse fp32 [P*G, nh], base
  2) with want_lse."""
  name = 'attn_decode_beam'
  try:
    O._need(q, O.BF16, 'q', 2)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  if q.shape[1] % nh != 0:
    raise ValueError(f'{name}: q {tuple(q.shape)} does not fit nh={nh}')
  hd = q.shape[1] // nh
  P, G = S._shared_operands(name, tuple(q.shape), kv_p, lens_p, kv_s, lens_s, nh, hd)
  _need_beams(name, G)
  Tp, Ts = kv_p.shape[1], kv_s.shape[1]
  _need_anc(name, anc, P * G, Ts)
  nbytes = O._ws_bytes('plm_attn_decode_beam_workspace_bytes', P, G, nh, hd, Tp, Ts, int(splits_p), int(splits_s))
  if nbytes == 0:
    raise ValueError(f'{name}: unsupported shape P={P} G={G} nh={nh} hd={hd} Tp_max={Tp} Ts_max={Ts} or splits_p={splits_p} / splits_s={splits_s} '
                     '(0 = automatic, 1..64)')
  stream = O._stream()
  ws = O._workspace(q.device, nbytes, stream)
  out = torch.empty((P * G, nh * hd), dtype=O.BF16, device=q.device)
  lse = torch.empty((P * G, nh), dtype=O.F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_decode_beam(O._p(q), O._p(kv_p), kv_p.stride(1), O._p(lens_p), O._p(kv_s), kv_s.stride(1), O._p(lens_s), O._p(anc),
                                              O._p(out), O._p(lse), P, G, Tp, Ts, nh, hd, int(splits_p), int(splits_s), O._p(ws), nbytes, stream),
             'plm_attn_decode_beam')
  return (out, lse) if want_lse else out


def decode_layer_beam(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, row, lens_s, rot0, lens_p, anc, rope_cos, rope_sin, kv_p, kv_s, nh,
                      kind, status, splits_p=0, splits_s=0):
  """ops.decode_layer_shared with attn_decode_beam as its attention stage (anc as above), P*G <= FUSED_DECODE_MAX_ROWS: one library call,
  seven launches.  x fp32 [P*G, d] is updated in place and returned."""
  name = 'decode_layer_beam'
  if kv_p.dim() == 3 and kv_s.dim() == 3 and kv_p.shape[0] >= 1 and kv_s.shape[0] % kv_p.shape[0] == 0:
    _need_beams(name, kv_s.shape[0] // kv_p.shape[0])
    _need_anc(name, anc, kv_s.shape[0], kv_s.shape[1])
  return S._layer_two_caches(name, 'plm_decode_layer_beam', x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, row, lens_s, rot0, lens_p,
                             (anc,), rope_cos, rope_sin, kv_p, kv_s, nh, kind, status, splits_p, splits_s)


class BeamBuffers:
  """The device state of one beam search over P prompts, G beams, at most N new tokens - what ops.beam_advance / ops.beam_finalize move:
  the ping-pong pair of ancestor tables (``anc`` is the current one: what the next decode step attends), ``score`` fp32 [P*G], ``tokens``
  int64 [P*G] (the tokens the next step takes), ``parent`` int32 [P*G], the histories int32 [P, N, G], the finished pool and ``done``
  int32 [P].  ``steps``: selections made so far."""

  def __init__(self, P, G, N, device):
    _need_beams('BeamBuffers', G)
    if P < 1 or N < 1:
      raise ValueError(f'BeamBuffers: need P >= 1 and N >= 1, got P={P} N={N}')
    self.P, self.G, self.N, self.steps = int(P), int(G), int(N), 0
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
    self._anc = z((2, P * G, N), torch.uint8)
    self.score, self.tokens, self.parent = z((P * G,), O.F32), z((P * G,), torch.int64), z((P * G,), torch.int32)
    self.score0 = z((P,), O.F32)  # the prompts' scores before the first selection
    self.tok_hist, self.par_hist = z((P, N, G), torch.int32), z((P, N, G), torch.int32)
    self.pool_f, self.pool_i, self.pool_n = z((P, G, 2), O.F32), z((P, G, 3), torch.int32), z((P,), torch.int32)
    self.done = z((P,), torch.int32)

  @property
  def anc(self):
    return self._anc[self.steps & 1]


def beam_select(logits, score, G, rows_per_prompt):
  """The 2G best (score[g] + log_softmax(logits[g])[v], g, v) per prompt, sorted by score descending, then beam ascending, then token
  ascending.  logits bf16 [P*rows_per_prompt, V] (unit inner stride, row stride >= V), score fp32 [P*rows_per_prompt]; rows_per_prompt is
  1 for the first step and G afterwards.  The log-softmax is built from ops.sample_logits's integer weights, so equal inputs give equal
  bits; NaN and infinite logits are never candidates, a beam with a non-finite score has none.  Returns (cand_score fp32, cand_beam int32,
  cand_tok int32), each [P, 2G]; missing candidates are (-inf, -1, -1) at the end."""
  name = 'beam_select'
  O._need(logits, O.BF16, f'{name}.logits', strided=True)
  O._need(score, O.F32, f'{name}.score', 1)
  rows, V = logits.shape
  _need_beams(name, G)
  if not 1 <= rows_per_prompt <= G or rows < 1 or rows % rows_per_prompt != 0 or score.shape[0] != rows or (rows > 1 and logits.stride(0) < V):
    raise ValueError(f'{name}: logits {tuple(logits.shape)} / score {tuple(score.shape)} are not P * rows_per_prompt={rows_per_prompt} rows '
                     f'(1 <= rows_per_prompt <= G={G}, row stride >= V)')
  if V < 2 * G:
    raise ValueError(f'{name}: a vocabulary of {V} is too small for {G} beams (V >= 2 * num_beams)')
  P = rows // rows_per_prompt
  nbytes = O._ws_bytes('plm_beam_select_workspace_bytes', rows, G)
  stream = O._stream()
  ws = O._workspace(logits.device, nbytes, stream)
  cs = torch.empty((P, 2 * G), dtype=O.F32, device=logits.device)
  cb, ct = torch.empty((P, 2 * G), dtype=torch.int32, device=logits.device), torch.empty((P, 2 * G), dtype=torch.int32, device=logits.device)
  _lib.check(_lib.load().plm_beam_select_bf16(O._p(logits), logits.stride(0) if rows > 1 else V, O._p(score), O._p(cs), O._p(cb), O._p(ct), P,
                                              int(rows_per_prompt), G, V, O._p(ws), nbytes, stream), 'plm_beam_select_bf16')
  return cs, cb, ct


def beam_advance(buf, cand, eos_id=None, length_penalty=1.0, early_stopping=False):
  """Step ``buf.steps`` of the search on BeamBuffers ``buf`` from ``cand`` = beam_select's triple: EOS candidates of rank < G enter the
  finished pool (length steps + 1), the others fill the next G live beams; writes buf.tokens / score / parent, row ``steps`` of the
  histories, the other ancestor table (which becomes ``buf.anc``) and buf.done.  Returns buf.tokens."""
  name = 'beam_advance'
  cs, cb, ct = cand
  for t, dt, nm in ((cs, O.F32, 'cand_score'), (cb, torch.int32, 'cand_beam'), (ct, torch.int32, 'cand_tok')):
    O._need(t, dt, f'{name}.{nm}', 2)
    if tuple(t.shape) != (buf.P, 2 * buf.G):
      raise ValueError(f'{name}: {nm} {tuple(t.shape)} is not [{buf.P}, {2 * buf.G}]')
  t = buf.steps
  if t >= buf.N:
    raise ValueError(f'{name}: all {buf.N} steps of these BeamBuffers are taken')
  _lib.check(_lib.load().plm_beam_advance(O._p(cs), O._p(cb), O._p(ct), O._p(buf._anc[t & 1]), O._p(buf._anc[(t + 1) & 1]), O._p(buf.tokens),
                                          O._p(buf.score), O._p(buf.parent), O._p(buf.tok_hist), O._p(buf.par_hist), O._p(buf.pool_f), O._p(buf.pool_i),
                                          O._p(buf.pool_n), O._p(buf.done), buf.P, buf.G, buf.N, t, -1 if eos_id is None else int(eos_id),
                                          float(length_penalty), int(bool(early_stopping)), O._stream()), 'plm_beam_advance')
  buf.steps = t + 1
  return buf.tokens


def beam_finalize(buf, num_return=1, length_penalty=1.0, eos_id=None, pad_id=0):
  """The best num_return <= G hypotheses per prompt after buf.steps steps, best first: (tokens int64 [P, R, N] padded with pad_id, lengths
  int32 [P, R], scores fp32 [P, R] = score / length ** length_penalty).  The live beams of a prompt that is not done enter at length
  buf.steps.  Changes no state."""
  name = 'beam_finalize'
  R = int(num_return)
  if not 1 <= R <= buf.G:
    raise ValueError(f'{name}: num_return must be in [1, num_beams={buf.G}], got {num_return}')
  if buf.steps < 1:
    raise ValueError(f'{name}: no step was taken')
  dev = buf.score.device
  tokens = torch.empty((buf.P, R, buf.N), dtype=torch.int64, device=dev)
  lengths, scores = torch.empty((buf.P, R), dtype=torch.int32, device=dev), torch.empty((buf.P, R), dtype=O.F32, device=dev)
  _lib.check(_lib.load().plm_beam_finalize(O._p(buf.score), O._p(buf.tok_hist), O._p(buf.par_hist), O._p(buf.pool_f), O._p(buf.pool_i),
                                           O._p(buf.pool_n), O._p(buf.done), O._p(tokens), O._p(lengths), O._p(scores), buf.P, buf.G, buf.N, buf.steps, R,
                                           -1 if eos_id is None else int(eos_id), int(pad_id), float(length_penalty), O._stream()),
             'plm_beam_finalize')
  return tokens, lengths, scores
