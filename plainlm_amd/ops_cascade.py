"""The ops wrappers of cascade attention over shared-prefix pages: sequences of one GROUP start with the same
whole pages - the same page ids at the start of their table rows - and a ragged step reads those keys once per 32 query rows of all
the group's members, not once per sequence.  ``ops.cascade_plan`` (pure host) turns per-slot row counts, shared keys and group ids into
``ragged_plan``'s words plus the group tiles; ``ops.attn_ragged_paged_cascade`` is ops.attn_ragged_paged over them (a prefix launch, the
ragged launch over the keys from key_lo on, one combine), ``ops.ragged_layer_paged_wide_cascade`` the wide fused layer with that stage.

The plan's words, int32 on the device: key_lo [B] (the shared keys of sequence b, a multiple of 64, 0: none), tile_rows [NTg, 32]
(the packed rows of a group tile, -1: a padding column), tile_seq [NTg] (the member whose table row names the tile's pages), tile_keys
[NTg].  A row of a sequence with key_lo > 0 always takes the prefix launch, alone in its group or not, so its bits depend on its own
sequence's rows, lens0[b], j and key_lo[b] alone.

They are part of ``plainlm_amd.ops`` (which re-exports them) and stand on its contract, like ops_ragged.py; no torch fallback."""

import torch

from . import _lib
from . import ops as O
from . import ops_decode as D
from . import ops_paged as PG
from . import ops_ragged as RG
from . import ops_wide as W


def cascade_plan(counts, key_lo, group):
  """Per-slot row counts, shared keys (host ints, multiples of ops.KV_PAGE_ROWS; 0: the slot shares nothing) and group ids (any
  hashable; read only where key_lo > 0) -> ragged_plan(counts)'s (cu_rows, row_seq, last_row, NT) followed by (key_lo int32 [B],
  tile_rows int32 [NTg, 32], tile_seq int32 [NTg], tile_keys int32 [NTg], NTg, Pcap), on the CPU.  The rows of a group's members, in
  packed order, fill its tiles 32 at a time; the first member with rows is the representative.  Pcap is the longest shared prefix with
  rows in the step.  A step in which no sharing slot has a row gets one tile without columns (NTg = 1, Pcap = one page)."""
  cu, row_seq, last_row, NT = RG.ragged_plan(counts)
  key_lo = [int(k) for k in key_lo]
  if len(key_lo) != len(counts) or len(group) != len(counts) or any(k < 0 or k % PG.KV_PAGE_ROWS for k in key_lo):
    raise ValueError(f'cascade_plan: need one key_lo (a multiple of {PG.KV_PAGE_ROWS}, none negative) and one group per count, got {key_lo}')
  rows, keys, seq = {}, {}, {}
  for b, c in enumerate(counts):
    if key_lo[b] and int(c):
      g = group[b]
      if keys.setdefault(g, key_lo[b]) != key_lo[b]:
        raise ValueError(f'cascade_plan: group {g!r} has members with {keys[g]} and {key_lo[b]} shared keys')
      seq.setdefault(g, b)
      rows.setdefault(g, []).extend(range(int(cu[b]), int(cu[b + 1])))
  tile_rows, tile_seq, tile_keys = [], [], []
  for g, rs in rows.items():
    for i in range(0, len(rs), RG.RAGGED_TILE_ROWS):
      part = rs[i:i + RG.RAGGED_TILE_ROWS]
      tile_rows.append(part + [-1] * (RG.RAGGED_TILE_ROWS - len(part)))
      tile_seq.append(seq[g])
      tile_keys.append(keys[g])
  if not tile_rows:
    tile_rows, tile_seq, tile_keys = [[-1] * RG.RAGGED_TILE_ROWS], [-1], [0]
  i32 = lambda v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
  return (cu, row_seq, last_row, NT, i32(key_lo), i32(tile_rows), i32(tile_seq), i32(tile_keys), len(tile_seq),
          max(tile_keys + [PG.KV_PAGE_ROWS]))


def _plan_operands(name, R, B, max_pages, key_lo, tile_rows, tile_seq, tile_keys, NTg, Pcap):
  """The checks of the plan's words; returns (NTg, Pcap) as ints."""
  try:
    O._need(key_lo, torch.int32, 'key_lo', 1)
    O._need(tile_rows, torch.int32, 'tile_rows', 2)
    O._need(tile_seq, torch.int32, 'tile_seq', 1)
    O._need(tile_keys, torch.int32, 'tile_keys', 1)
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  NTg, Pcap = int(NTg), int(Pcap)
  if not 1 <= NTg <= R:
    raise ValueError(f'{name}: NTg={NTg} group tiles outside [1, R = {R}] (cascade_plan counts them)')
  if key_lo.shape[0] != B or tuple(tile_rows.shape) != (NTg, RG.RAGGED_TILE_ROWS) or tile_seq.shape[0] != NTg or tile_keys.shape[0] != NTg:
    raise ValueError(f'{name}: key_lo {tuple(key_lo.shape)} (B = {B}), tile_rows {tuple(tile_rows.shape)}, tile_seq {tuple(tile_seq.shape)}, '
                     f'tile_keys {tuple(tile_keys.shape)} do not fit NTg={NTg}')
  if Pcap < PG.KV_PAGE_ROWS or Pcap % PG.KV_PAGE_ROWS or Pcap > max_pages * PG.KV_PAGE_ROWS:
    raise ValueError(f'{name}: Pcap={Pcap} is no positive multiple of {PG.KV_PAGE_ROWS} within the table\'s {max_pages * PG.KV_PAGE_ROWS} keys')
  return NTg, Pcap


def attn_ragged_paged_cascade(q, pool, table, lens0, key_lo, cu_rows, row_seq, tile_rows, tile_seq, tile_keys, nh, NT, NTg, Pcap, Lcap=None,
                              want_lse=False):
  """ops.attn_ragged_paged where sequences share their first key_lo[b] keys as whole pages: row j of sequence b attends keys
  0 .. lens0[b] + j, the first key_lo[b] of them through its group tile (cascade_plan's words), the rest through its own tile.  The
  table rows of a group's members name the same pages below key_lo.  A padding row, and a row of a sharing sequence that no tile
  lists, give out = 0 and lse = +inf.  Lcap and Pcap size the grids, never the bits.  Returns out bf16 [R, nh*hd], or (out, lse fp32
  [R, nh], base 2) with want_lse."""
  name = 'attn_ragged_paged_cascade'
  R, B, hd, max_pages, n_pages = RG._ragged_operands(name, q, 1, pool, table, nh, lens0, cu_rows, row_seq)
  NT = RG._tiles(name, NT, R)
  NTg, Pcap = _plan_operands(name, R, B, max_pages, key_lo, tile_rows, tile_seq, tile_keys, NTg, Pcap)
  Lcap = PG._lcap(name, Lcap, max_pages)
  nbytes = O._ws_bytes('plm_attn_ragged_paged_cascade_workspace_bytes', R, nh, hd, Lcap, NTg, Pcap)
  if nbytes == 0:
    raise ValueError(f'{name}: unsupported shape R={R} nh={nh} hd={hd} Lcap={Lcap} Pcap={Pcap} (at most 64 chunks of {PG.KV_PAGED_CHUNK} keys)')
  stream = O._stream()
  ws = O._workspace(q.device, nbytes, stream)
  out = torch.empty((R, nh * hd), dtype=O.BF16, device=q.device)
  lse = torch.empty((R, nh), dtype=O.F32, device=q.device) if want_lse else None
  _lib.check(_lib.load().plm_attn_ragged_paged_cascade(O._p(q), O._p(pool), pool.stride(1), O._p(table), O._p(lens0), O._p(key_lo), O._p(cu_rows),
                                                       O._p(row_seq), O._p(tile_rows), O._p(tile_seq), O._p(tile_keys), O._p(out), O._p(lse), R, B,
                                                       NT, NTg, Lcap, Pcap, max_pages, n_pages, nh, hd, O._p(ws), nbytes, stream),
             'plm_attn_ragged_paged_cascade')
  return (out, lse) if want_lse else out


def ragged_layer_paged_wide_cascade(x, attn_norm_w, mlp_norm_w, eps, w_qkv, w_out, w_fc1, w_fc2, lens0, key_lo, cu_rows, row_seq, tile_rows,
                                    tile_seq, tile_keys, rope_cos, rope_sin, pool, table, nh, kind, status, NT, NTg, Pcap, Lcap=None):
  """ops.ragged_layer_paged_wide with attn_ragged_paged_cascade as its attention stage, one library call: x fp32 [R, d]
  (R <= FUSED_WIDE_MAX_ROWS packed rows) is updated in place and returned."""
  name = 'ragged_layer_paged_wide_cascade'
  R, d, hd, B, max_pages, n_pages = W._wide_ragged_operands(name, x, (attn_norm_w, mlp_norm_w), (w_qkv, w_out, w_fc1, w_fc2), pool, table, lens0,
                                                            cu_rows, row_seq, rope_cos, rope_sin, nh)
  k = D._decode_mlp_kind(name, kind)
  hidden = w_fc2.shape[1]
  if tuple(w_out.shape) != (d, d) or w_fc2.shape[0] != d or tuple(w_fc1.shape) != ((2 if kind == 'glu' else 1) * hidden, d):
    raise ValueError(f'{name}: the weights {tuple(w_out.shape)}, {tuple(w_fc1.shape)}, {tuple(w_fc2.shape)} do not fit x {tuple(x.shape)}, '
                     f'kind {kind!r}')
  try:
    O._need(status, torch.int32, 'status')
  except (RuntimeError, TypeError, ValueError) as e:
    raise type(e)(f'{name}.{e}') from None
  NT = RG._tiles(name, NT, R)
  NTg, Pcap = _plan_operands(name, R, B, max_pages, key_lo, tile_rows, tile_seq, tile_keys, NTg, Pcap)
  Lcap = PG._lcap(name, Lcap, max_pages)
  nbytes = O._ws_bytes('plm_ragged_layer_paged_wide_cascade_workspace_bytes', R, nh, hd, hidden, Lcap, NTg, Pcap)
  if nbytes == 0:
    raise ValueError(f'{name}: unsupported shape R={R} nh={nh} hd={hd} hidden={hidden} Lcap={Lcap} Pcap={Pcap}')
  stream = O._stream()
  ws = O._workspace(x.device, nbytes, stream)
  with O._Launch('hbm:layer_wide', 2.0 * (w_qkv.numel() + w_out.numel() + w_fc1.numel() + w_fc2.numel())):
    _lib.check(_lib.load().plm_ragged_layer_paged_wide_cascade_bf16(
        O._p(x), O._p(attn_norm_w), O._p(mlp_norm_w), float(eps), O._p(w_qkv), O._p(w_out), O._p(w_fc1), O._p(w_fc2), O._p(lens0), O._p(key_lo),
        O._p(cu_rows), O._p(row_seq), O._p(tile_rows), O._p(tile_seq), O._p(tile_keys), O._p(rope_cos), O._p(rope_sin), rope_cos.shape[0],
        O._p(pool), pool.stride(1), O._p(table), O._p(status), R, B, NT, NTg, Lcap, Pcap, max_pages, n_pages, nh, hd, hidden, k, O._p(ws), nbytes,
        stream), 'plm_ragged_layer_paged_wide_cascade_bf16')
  return x
