"""Shared-prefix pages on a real MI355X: plm_attn_ragged_paged_cascade against the fp64 attention reference under
oracle/parity.py's bounds, with ops.attn_ragged_paged on the same aliased table as the control, and its bit properties (group size,
packing order, page placement, Lcap); the wide cascade layer against its parts' bits; step_ragged on a cache admitted with admit_prefix
and serve_shared against the full forward."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity as PB  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_decode_gpu as TD  # noqa: E402
from test_decode_gpu import P, biteq, bits, mdl, ops  # noqa: E402,F401
from test_paged_gpu import BF16, NH, PG, _model, _scrambled_pool, i32, paginate  # noqa: E402

# (own keys before the step, rows, shared keys, group): the first own token; a page edge; two own tiles, causal inside; an own range that
# crosses a chunk edge at a key_lo offset; no prefix; an idle slot.  Group b has 41 rows: two group tiles, the second of two sequences
SEQS = ((0, 1, 64, 'a'), (63, 1, 64, 'a'), (0, 40, 576, 'b'), (500, 1, 576, 'b'), (100, 3, 0, None), (10, 0, 0, None))
L0 = [own + klo for own, _, klo, _ in SEQS]
REP = [[g for _, _, _, g in SEQS].index(g) for _, _, _, g in SEQS]  # the first member of every sequence's group (itself without one)
_case = {}


def cascade_case(ops, hd):
  """test_ragged_gpu.ragged_case's construction; a group's members hold their representative's first key_lo k | v rows."""
  if hd not in _case:
    B, T, d = len(SEQS), 1088, NH * hd
    qkv = torch.randn(B, T, 3 * d, generator=torch.Generator().manual_seed(T * NH + hd)).to(BF16)
    for b, (_, _, klo, _) in enumerate(SEQS):
      qkv[b, :klo, d:] = qkv[REP[b], :klo, d:]
    cos, sin = (t.cuda() for t in O.rope_table(hd, T))
    q3 = ops.rope_qk_(qkv.view(B * T, 3 * d).cuda(), cos, sin, B, T, NH).view(B, T, 3 * d)
    ref = PB.reference(q3.reshape(B * T, 3 * d).cpu(), torch.zeros(B * T, d), B, T, NH, hd)
    cut = lambda t: torch.cat([t[b, :, a:a + SEQS[b][1]].transpose(0, 1) for b, a in enumerate(L0)]).unsqueeze(2)  # noqa: E731
    _case[hd] = dict(kv=q3[:, :, d:].contiguous(), q=[q3[b, a:a + SEQS[b][1], :d] for b, a in enumerate(L0)], out=cut(ref['out']), lse=cut(ref['lse']))
  return _case[hd]


def paginate_shared(kv, seed, spare=3):
  """paginate, then every member's first key_lo / 64 table entries name its representative's pages; its own copies turn to NaN."""
  pool, table = paginate(kv, [a + c for a, (_, c, _, _) in zip(L0, SEQS)], seed, spare)
  for b, (_, _, klo, _) in enumerate(SEQS):
    if REP[b] != b:
      pool[table[b, :klo // PG].long()] = float('nan')
      table[b, :klo // PG] = table[REP[b], :klo // PG]
  return pool, table


def attend(ops, c, order, pool, table, Lcap=None, alone=False, plain=False):
  """The sequences ``order`` packed in that order, then one padding row; returns ({b: (out rows, lse rows)}, the padding row's)."""
  counts = [SEQS[b][1] for b in order]
  group = [(b if alone else SEQS[b][3]) for b in order]
  cu, row_seq, _, NT, key_lo, tile_rows, tile_seq, tile_keys, NTg, Pcap = ops.cascade_plan(counts, [SEQS[b][2] for b in order], group)
  q = torch.cat([c['q'][b] for b in order] + [torch.full_like(c['q'][0][:1], float('nan'))]).contiguous()
  row_seq = torch.cat([row_seq, torch.tensor([-1], dtype=torch.int32)]).cuda()
  tb, l0 = table[list(order)].contiguous(), i32([L0[b] for b in order])
  if plain:
    out, lse = ops.attn_ragged_paged(q, pool, tb, l0, cu.cuda(), row_seq, NH, NT, Lcap=Lcap, want_lse=True)
  else:
    out, lse = ops.attn_ragged_paged_cascade(q, pool, tb, l0, key_lo.cuda(), cu.cuda(), row_seq, tile_rows.cuda(), tile_seq.cuda(), tile_keys.cuda(),
                                             NH, NT, NTg, Pcap, Lcap=Lcap, want_lse=True)
  return {b: (out[cu[i]:cu[i + 1]], lse[cu[i]:cu[i + 1]]) for i, b in enumerate(order)}, (out[-1], lse[-1])


@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_cascade_vs_fp64_and_its_bit_properties(ops, hd):
  c, B = cascade_case(ops, hd), len(SEQS)
  pool, table = paginate_shared(c['kv'], 1)
  before = pool.clone()
  got, (pad_o, pad_l) = attend(ops, c, range(B), pool, table)
  assert (bits(pad_o) == 0).all() and bool((pad_l == float('inf')).all())  # the padding row: out = 0, lse = +inf
  assert PB.BOUNDS['row']['out'] == 1.5e-2 and PB.BOUNDS['proj']['out'] == 3e-3 and PB.BOUNDS['proj_slice']['out'] == 3e-3 and PB.BOUNDS['lse'] == 1e-4
  for name, res in (('cascade', got), ('control: attn_ragged_paged on the aliased table', attend(ops, c, range(B), pool, table, plain=True)[0])):
    out, lse = torch.cat([res[b][0] for b in range(B)]), torch.cat([res[b][1] for b in range(B)])
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    got_o, got_l = out.double().cpu().view(-1, NH, 1, hd), lse.double().cpu().view(-1, NH, 1)
    m = {'row_out': PB.row_local(got_o, c['out'])}
    m['proj_out'], m['proj_slice_out'] = PB.projection(got_o, c['out'])
    m['lse'] = (got_l - c['lse']).abs().max().item()
    print(f'parity {name} hd={hd}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
    assert not PB.violations(m), (name, PB.violations(m))
  assert biteq(pool, before)  # the pool is unchanged by the calls
  same = lambda other: all(biteq(other[b][0], got[b][0]) and torch.equal(other[b][1], got[b][1]) for b in other)  # noqa: E731
  assert same(attend(ops, c, range(B), pool, table, alone=True)[0])  # every sequence the only member of its group
  pool2, table2 = paginate_shared(c['kv'], 2, spare=5)  # another page placement
  assert not torch.equal(table, table2) and same(attend(ops, c, range(B), pool2, table2)[0])
  assert same(attend(ops, c, range(B - 1, -1, -1), pool, table)[0])  # packed in reverse order: other tiles, other columns
  for b in range(B):  # every sequence alone in the step, at the least Lcap its length needs
    if SEQS[b][1]:
      assert same(attend(ops, c, [b], pool, table, -(-(L0[b] + SEQS[b][1]) // PG) * PG)[0]), b


def test_wide_cascade_layer_is_its_parts_bits(ops):
  hd, Tmax, hidden, eps = 64, 192, 256, 1e-6
  lens0, counts, key_lo = (64, 70, 5, 0), (40, 1, 30, 0), [64, 64, 0, 0]  # R = 71: two 64-row tiles of the wide stages
  B, R, d = len(counts), sum(counts), NH * hd
  g = torch.Generator().manual_seed(R)
  rnd = lambda *s, dt=BF16, k=0.1: (k * torch.randn(*s, generator=g)).to(dt).cuda()  # noqa: E731
  x = rnd(R, d, dt=torch.float32, k=1.0)
  an, mn = 1 + rnd(d, dt=torch.float32), 1 + rnd(d, dt=torch.float32)
  w_qkv, w_out, w_fc1, w_fc2 = rnd(3 * d, d), rnd(d, d), rnd(2 * hidden, d), rnd(d, hidden)
  cos, sin = (t.cuda() for t in O.rope_table(hd, Tmax))
  pool0, table = paginate(rnd(B, Tmax, 2 * d, k=1.0), [a + c for a, c in zip(lens0, counts)], 81)
  table[1, 0] = table[0, 0]  # sequences 0 and 1 share their first page
  cu, row_seq, _, NT, kl, tr, ts, tk, NTg, Pcap = ops.cascade_plan(counts, key_lo, 'aa--')
  l0, cu, rs, plan = i32(lens0), cu.cuda(), row_seq.cuda(), (tr.cuda(), ts.cuda(), tk.cuda())
  xs, pool = x.clone(), pool0.clone()
  q, status = ops.ragged_norm_qkv_append_paged_wide(xs, an, eps, w_qkv, l0, cu, rs, cos, sin, pool, table, NH)
  att = ops.attn_ragged_paged_cascade(q, pool, table, l0, kl.cuda(), cu, rs, *plan, NH, NT, NTg, Pcap)
  ops.wide_gemm_residual(xs, att, w_out)
  ops.wide_gemm_residual(xs, ops.wide_norm_fc1_act(xs, mn, eps, w_fc1, 'glu'), w_fc2)
  xl, pl = x.clone(), pool0.clone()
  ops.ragged_layer_paged_wide_cascade(xl, an, mn, eps, w_qkv, w_out, w_fc1, w_fc2, l0, kl.cuda(), cu, rs, *plan, cos, sin, pl, table, NH, 'glu',
                                      status, NT, NTg, Pcap)
  assert (NTg, Pcap) == (2, 64) and torch.isfinite(xl).all() and biteq(xl, xs) and biteq(pl, pool) and not biteq(xl, x) and int(status.item()) == 0


def _full(m, seq):
  return m(torch.nn.functional.pad(seq, (0, -seq.numel() % 4)).view(1, -1), None).float()[0]


@pytest.mark.parametrize('fused', [False, 'wide'])
def test_step_ragged_on_a_shared_prefix_vs_the_full_forward(P, mdl, fused):
  """Slots 0 and 1 stand on one prefix page and feed its rest and their own tokens in chunks, slot 2 has no prefix; then all decode."""
  m, tok = _model(P, mdl, seq_len=192), mdl['tokens'].reshape(-1).cuda()
  pool = _scrambled_pool(m, 9, 11)
  with torch.no_grad():
    prefix = m.prefill_prefix(tok[:70], pool)
    assert prefix.n_tokens == 64 and prefix.rest.numel() == 6 and pool.n_free == 8
    cache = m.new_cache_paged(3, pool, 192)
    cache.admit_prefix(0, prefix)
    cache.admit_prefix(1, prefix)
    cache.admit(2)
    seqs = [torch.cat([tok[:70], tok[70:121]]), torch.cat([tok[:70], tok[20:23]]), tok[80:121]]  # (the golden file holds 128 tokens)
    fed, rows = [64, 64, 0], [[], [], []]
    for counts in ((40, 9, 33), (16, 0, 8), (0, 0, 0)):
      counts = [c or min(1, s.numel() - f) for c, s, f in zip(counts, seqs, fed)]  # a slot without a chunk decodes while it has tokens
      x = torch.cat([s[f:f + c] for s, f, c in zip(seqs, fed, counts)])
      for b, part in enumerate(m.step_ragged(x, counts, cache, logits=True, all_rows=True, fused=fused).split(counts)):
        rows[b].append(part)
        fed[b] += counts[b]
    cache.check()
    assert cache.lens.tolist() == fed == [121, 73, 41] and cache.key_lo == [64, 64, 0]
    for b in range(3):
      start = 64 if b < 2 else 0
      e = TD.relmax(torch.cat(rows[b]).float(), _full(m, seqs[b])[start:fed[b]])
      print(f'step_ragged on a shared prefix fused={fused}: slot {b}: rows {start}..{fed[b]}, relmax {e:.2e}')
      assert e < 2e-2, (b, e)
    for b in range(3):
      cache.release(b)
    prefix.release()
    assert pool.n_free == 9


@pytest.mark.parametrize('fused', [False, 'wide'])
def test_serve_shared_against_the_full_forward(P, mdl, fused):
  m, tok = _model(P, mdl, seq_len=192), mdl['tokens'].reshape(-1).cuda()
  plen, budget = (5, 30, 17, 9), [70, 12, 40, 8]
  prompts, o = [], 64
  for n in plen:
    prompts.append(tok[o:o + n])
    o += n
  with torch.no_grad():
    for n_prefix, n_pages in ((70, 5), (20, 4)):  # one shared page and six rest tokens; a prefix shorter than a page shares nothing
      pool = _scrambled_pool(m, n_pages, 8)
      outs = m.serve_shared(tok[:n_prefix], prompts, budget, max_batch=2, pool=pool, fused=fused, prefill_chunk=16)
      assert pool.n_free == n_pages and [t.numel() for t in outs] == budget  # every page is back in the pool
      for i, (p, t) in enumerate(zip(prompts, outs)):
        full, at = _full(m, torch.cat([tok[:n_prefix], p, t])), n_prefix + p.numel() - 1  # row at + j predicts generated token j
        eps = 2e-2 * full.abs().max().item()
        rows = full[at:at + t.numel()]
        gap = (rows.max(dim=-1).values - rows.gather(1, t[:, None])[:, 0]).max().item()
        print(f'serve_shared prefix={n_prefix} fused={fused}: sequence {i}: worst (row max - chosen logit) {gap:.3e} against 4 eps = {4 * eps:.3e}')
        assert gap <= 4 * eps, i  # every generated position, none excluded
