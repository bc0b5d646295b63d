"""Ragged steps on a real MI355X: plm_attn_ragged_paged against the fp64 attention reference under oracle/parity.py's
bounds and its bit properties (page placement, packing order, batch, Lcap), the packed append against the rows kernel's bits, the fused
stage and layer against their parts' bits, the model teacher-forced through step_ragged against the golden logits, and
serve(prefill_chunk=...) against the full forward."""

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

# (lens0, count): the first token, a page edge, a chunk edge, an idle slot, a prompt from nothing (three tiles, causal inside), a chunk
# edge inside a chunk, a second tile holding one row
SEQS = ((0, 1), (63, 1), (512, 1), (10, 0), (0, 70), (500, 40), (1030, 33))
_case = {}


def ragged_case(ops, hd):
  """test_paged_gpu.decode_case's construction: packed row (b, j) is row lens0[b] + j of the causal fp64 reference."""
  if hd not in _case:
    B, T, d = len(SEQS), 2 * ops.KV_PAGED_CHUNK + 64, NH * hd
    qkv = torch.randn(B * T, 3 * d, generator=torch.Generator().manual_seed(T * NH + hd)).to(BF16)
    cos, sin = (t.cuda() for t in O.rope_table(hd, T))
    q3 = ops.rope_qk_(qkv.cuda(), cos, sin, B, T, NH).view(B, T, 3 * d)
    ref = PB.reference(q3.reshape(B * T, 3 * d).cpu(), torch.zeros(B * T, d), B, T, NH, hd)
    _case[hd] = dict(kv=q3[:, :, d:].contiguous(), q=[q3[b, a:a + c, :d] for b, (a, c) in enumerate(SEQS)],
                     out=torch.cat([ref['out'][b, :, a:a + c].transpose(0, 1) for b, (a, c) in enumerate(SEQS)]).unsqueeze(2),
                     lse=torch.cat([ref['lse'][b, :, a:a + c].transpose(0, 1) for b, (a, c) in enumerate(SEQS)]).unsqueeze(2))
  return _case[hd]


def attend(ops, c, order, pool, table, Lcap=None):
  """The sequences ``order`` packed in that order, then one padding row; returns ({b: (out rows, lse rows)}, the padding row's)."""
  counts = [SEQS[b][1] for b in order]
  cu, row_seq, _, NT = ops.ragged_plan(counts)
  q = torch.cat([c['q'][b] for b in order] + [torch.full_like(c['q'][0][:1], float('nan'))])
  row_seq = torch.cat([row_seq, torch.tensor([-1], dtype=torch.int32)])
  out, lse = ops.attn_ragged_paged(q.contiguous(), pool, table[list(order)].contiguous(), i32([SEQS[b][0] for b in order]), cu.cuda(), row_seq.cuda(),
                                   NH, NT, Lcap=Lcap, want_lse=True)
  return {b: (out[cu[i]:cu[i + 1]], lse[cu[i]:cu[i + 1]]) for i, b in enumerate(order)}, (out[-1], lse[-1])


@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_ragged_paged_vs_fp64_and_its_bit_properties(ops, hd):
  c, B, held = ragged_case(ops, hd), len(SEQS), [a + n for a, n in SEQS]
  pool, table = paginate(c['kv'], held, 1)
  before = pool.clone()
  got, (pad_o, pad_l) = attend(ops, c, range(B), pool, table)
  out, lse = torch.cat([got[b][0] for b in range(B)]), torch.cat([got[b][1] for b in range(B)])
  assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
  assert (bits(pad_o) == 0).all() and bool((pad_l == float('inf')).all())  # the padding row: out = 0, lse = +inf
  got_o, got_l = out.double().cpu().view(-1, NH, 1, hd), lse.double().cpu().view(-1, NH, 1)
  m = {'row_out': PB.row_local(got_o, c['out'])}
  m['proj_out'], m['proj_slice_out'] = PB.projection(got_o, c['out'])
  m['lse'] = (got_l - c['lse']).abs().max().item()
  print(f'parity ragged paged hd={hd}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  assert PB.BOUNDS['row']['out'] == 1.5e-2 and PB.BOUNDS['proj']['out'] == 3e-3 and PB.BOUNDS['proj_slice']['out'] == 3e-3 and PB.BOUNDS['lse'] == 1e-4
  assert not PB.violations(m), PB.violations(m)
  assert biteq(pool, before)  # the pool is unchanged by the call
  same = lambda other: all(biteq(other[b][0], got[b][0]) and torch.equal(other[b][1], got[b][1]) for b in other)  # noqa: E731
  pool2, table2 = paginate(c['kv'], held, 2, spare=5)  # another page placement
  assert not torch.equal(table, table2) and same(attend(ops, c, range(B), pool2, table2)[0])
  assert same(attend(ops, c, range(B - 1, -1, -1), pool, table)[0])  # packed in reverse order
  for b in range(B):  # every sequence alone, at the table's width and at the least its length needs
    if SEQS[b][1]:
      for Lcap in (None, -(-held[b] // PG) * PG):
        assert same(attend(ops, c, [b], pool, table, Lcap)[0]), (b, Lcap)


@pytest.mark.parametrize('hd', [32, 64, 128])
def test_packed_append_is_the_rows_append(ops, hd):
  B, n, Tmax, d = 5, 7, 192, NH * hd
  g = torch.Generator().manual_seed(hd)
  qkv = torch.randn(B * n, 3 * d, generator=g).to(BF16).cuda()
  cos, sin = (t.cuda() for t in O.rope_table(hd, Tmax))
  old = torch.randn(B, Tmax, 2 * d, generator=g).to(BF16).cuda()
  lens0, counts = (60, 0, 125, 64, 190), (7, 3, 0, 6, 7)  # across a page edge, a first row, nothing, a missing page, past max_pages
  pool0, table = paginate(old, [min(a + c, Tmax) for a, c in zip(lens0, counts)], 3)
  table[3, 1] = -1
  rows_pool, pool = pool0.clone(), pool0.clone()
  q_rows, _ = ops.kv_paged_append_rope_rows(qkv, i32(lens0), cos, sin, rows_pool, table, NH, n_new=i32(counts))
  cu, row_seq, _, _ = ops.ragged_plan(counts)
  take = torch.tensor([b * n + j for b, c in enumerate(counts) for j in range(c)]).cuda()
  q, status = ops.kv_paged_append_rope_packed(qkv[take], i32(lens0), cu.cuda(), row_seq.cuda(), cos, sin, pool, table, NH)
  assert int(status.item()) == 1 and biteq(pool, rows_pool) and biteq(q, q_rows[take])
  assert int((bits(pool) != bits(pool0)).any(-1).sum()) == 10  # sequences 0 and 1 stored their rows, every other pool byte is as it was
  assert (bits(q[10:]) == 0).all() and bits(q[:10]).any()  # the refused sequences' q rows are zeros


@pytest.mark.parametrize('counts', [(4, 1, 0, 2), (20, 1, 0, 11)])  # R = 7 and R = 32: both bodies of the skinny-M kernel
def test_fused_ragged_stage_and_layer_are_their_parts_bits(ops, counts):
  hd, B, Tmax, hidden, eps, R = 64, len(counts), 192, 256, 1e-6, sum(counts)
  d = NH * hd
  g = torch.Generator().manual_seed(R)
  rnd = lambda *s, dt=BF16, k=0.1: (k * torch.randn(*s, generator=g)).to(dt).cuda()  # noqa: E731
  x = rnd(R, d, dt=torch.float32, k=1.0)
  an, mn = 1 + rnd(d, dt=torch.float32), 1 + rnd(d, dt=torch.float32)
  w_qkv, w_out, w_fc1, w_fc2 = rnd(3 * d, d), rnd(d, d), rnd(2 * hidden, d), rnd(d, hidden)
  cos, sin = (t.cuda() for t in O.rope_table(hd, Tmax))
  lens0 = (60, 5, 130, 0)  # across a page edge, inside a page, idle, a prompt from nothing
  pool0, table = paginate(rnd(B, Tmax, 2 * d, k=1.0), [a + c for a, c in zip(lens0, counts)], 10 + R)
  cu, row_seq, _, NT = ops.ragged_plan(counts)
  l0, cu_d, rs = i32(lens0), cu.cuda(), row_seq.cuda()
  # the stage: every sequence's rows through ops.extend_norm_qkv_append_paged, at its positions
  want, pool = pool0.clone(), pool0.clone()
  q_want = torch.cat([ops.extend_norm_qkv_append_paged(x[cu[b]:cu[b + 1]], an, eps, w_qkv, l0[b:b + 1], cos, sin, want, table[b:b + 1].contiguous(),
                                                       NH)[0] for b in range(B) if counts[b]])
  q, status = ops.ragged_norm_qkv_append_paged(x, an, eps, w_qkv, l0, cu_d, rs, cos, sin, pool, table, NH)
  assert int(status.item()) == 0 and biteq(q, q_want) and biteq(pool, want)
  # the layer: its five stages, one ops call each
  xs = x.clone()
  ops.decode_gemm_residual(xs, ops.attn_ragged_paged(q, pool, table, l0, cu_d, rs, NH, NT), w_out)
  ops.decode_gemm_residual(xs, ops.decode_norm_fc1_act(xs, mn, eps, w_fc1, 'glu'), w_fc2)
  xl, pl = x.clone(), pool0.clone()
  ops.ragged_layer_paged(xl, an, mn, eps, w_qkv, w_out, w_fc1, w_fc2, l0, cu_d, rs, cos, sin, pl, table, NH, 'glu', status, NT)
  assert torch.isfinite(xl).all() and biteq(xl, xs) and biteq(pl, pool) and not biteq(xl, x) and int(status.item()) == 0


@pytest.mark.parametrize('fused', [False, True])
def test_step_ragged_logits_vs_golden(P, mdl, fused):
  """Slot 0 takes sequence 0 in chunks of 5, slot 1 decodes sequence 1 one row a step, slot 2 joins at step 3 with one chunk of sequence
  0 - 33 rows, or 26 with fused=True: the step then holds 5 + 1 + 26 = 32 rows, the most a fused step takes - and decodes on."""
  m, tok, T = _model(P, mdl), mdl['tokens'], 64
  cache = m.new_cache_paged(3, _scrambled_pool(m, 5, 7), T)
  cache.admit(0)
  cache.admit(1)
  src, fed, rows = (0, 1, 0), [0, 0, 0], [[], [], []]
  for step in range(13):
    if step == 3:
      cache.admit(2)
    counts = [min(5, T - fed[0]), 1, 0 if step < 3 else ((26 if fused else 33) if step == 3 else 1)]
    x = torch.cat([tok[src[b], fed[b]:fed[b] + c] for b, c in enumerate(counts)]).cuda()
    lg = m.step_ragged(x, counts, cache, logits=True, all_rows=True, fused=fused)
    for b, part in enumerate(lg.split(counts)):
      rows[b].append(part)
      fed[b] += counts[b]
  cache.check()
  assert cache.lens.tolist() == fed == [64, 13, (26 if fused else 33) + 9]
  for b in range(3):
    e = TD.relmax(torch.cat(rows[b]).float(), mdl['logits'][src[b], :fed[b]])
    print(f'step_ragged fused={fused}: slot {b}: {fed[b]} rows, relmax {e:.2e}')
    assert e < 2e-2, (b, e)
  last = m.step_ragged(tok[1, 13:14].cuda(), [0, 1, 0], cache, logits=True, fused=fused)  # the last rows alone: [B, V], slot 1's is real
  assert tuple(last.shape) == (3, 256) and TD.relmax(last[1].float(), mdl['logits'][1, 13]) < 2e-2


@pytest.mark.parametrize('fused', [False, True])
def test_serve_with_chunked_prefill_against_the_full_forward(P, mdl, fused):
  m, C = _model(P, mdl, seq_len=192), 8 if fused else 16
  tok = mdl['tokens'].reshape(-1)
  plen, budget = (5, 60, 17, 33, 9), [70, 12, 40, 8, 20]  # test_serve_continuous_batching_against_the_full_forward's prompts, budgets and pools
  prompts, o = [], 0
  for n in plen:
    prompts.append(tok[o:o + n].cuda())
    o += n
  with torch.no_grad():
    free_run = m.serve(prompts, budget, max_batch=2, pool=_scrambled_pool(m, 3, 8), fused=fused, prefill_chunk=C)
    assert [t.numel() for t in free_run] == budget
    eos = int(free_run[2][10])  # sequence 2 ends through eos_id, at the latest at its 11th token
    pool = _scrambled_pool(m, 3, 9)
    outs = m.serve(prompts, budget, max_batch=2, pool=pool, eos_id=eos, fused=fused, prefill_chunk=C)
    assert pool.n_free == 3
    again = m.serve(prompts, budget, max_batch=2, pool=pool, eos_id=eos, fused=fused, prefill_chunk=C)
    assert outs[2].numel() <= 11 and int(outs[2][-1]) == eos
    for i, (p, t, t2) in enumerate(zip(prompts, outs, again)):
      assert torch.equal(t, t2) and 1 <= t.numel() <= budget[i], i
      assert t.numel() == budget[i] or int(t[-1]) == eos, i
      assert eos not in t[:-1].tolist(), i
      seq = torch.cat([p, t])
      full = m(torch.nn.functional.pad(seq, (0, -seq.numel() % 4)).view(1, -1), None).float()[0]
      eps = 2e-2 * full.abs().max().item()
      rows = full[p.numel() - 1:p.numel() - 1 + t.numel()]  # row len(prompt) - 1 + j predicts generated token j
      gap = (rows.max(dim=-1).values - rows.gather(1, t[:, None])[:, 0]).max().item()
      print(f'serve prefill_chunk={C} fused={fused}: sequence {i}: {t.numel()} tokens, worst (row max - chosen logit) {gap:.3e} against 4 eps = {4 * eps:.3e}')
      assert gap <= 4 * eps, i  # every generated position, none excluded
