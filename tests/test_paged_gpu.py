"""The paged KV cache on a real MI355X: plm_attn_decode_paged and plm_attn_extend_paged against the fp64 attention
reference under oracle/parity.py's bounds and their bit properties (page placement, batch, Lcap), the paged append and store against the
contiguous kernels' bits, the model teacher-forced on a paged cache against the golden logits, and serve against the full forward."""

import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity as PB  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_decode_gpu as TD  # noqa: E402
import test_extend_gpu as TE  # noqa: E402
from test_decode_gpu import P, biteq, bits, mdl, ops  # noqa: E402,F401

BF16, NH, PG = torch.bfloat16, 3, 64
i32 = lambda v: torch.tensor(v, dtype=torch.int32).cuda()  # noqa: E731


def paginate(kv, lens, seed, spare=3):
  """kv [B, T, w] and the rows each sequence holds -> (pool, table): the pages at a random permutation of a pool with spare pages;
  every unreferenced page, and the rows past lens in each last page, hold NaN."""
  B, T, w = kv.shape
  need = [-(-n // PG) for n in lens]
  perm = torch.randperm(sum(need) + spare, generator=torch.Generator().manual_seed(seed)).tolist()
  pool = torch.full((len(perm), PG, w), float('nan'), dtype=BF16, device='cuda')
  table = torch.full((B, -(-T // PG)), -1, dtype=torch.int32)
  for b in range(B):
    for i in range(need[b]):
      table[b, i] = p = perm.pop()
      rows = kv[b, i * PG:min((i + 1) * PG, lens[b])]
      pool[p, :rows.shape[0]] = rows
  return pool, table.cuda()


# ---- 1, 2: plm_attn_decode_paged --------------------------------------------------------------------------------------------------------
_case = {}


def decode_case(ops, hd):
  """test_decode_gpu.decode_case's construction at the lengths that cross a page edge, a chunk edge and an odd tail."""
  if hd not in _case:
    C = ops.KV_PAGED_CHUNK
    lens = (1, 63, 64, 65, C, C + 1, 2 * C + 13)
    B, T, d = len(lens), 2 * C + 16, NH * hd  # T: a multiple of 4, the RoPE pass's granularity
    g = torch.Generator().manual_seed(T * NH + hd)
    qkv = torch.randn(B * T, 3 * d, generator=g).to(BF16)
    cos, sin = (t.cuda() for t in O.rope_table(hd, T))
    qrot = ops.rope_qk_(qkv.cuda(), cos, sin, B, T, NH)
    ref = PB.reference(qrot.cpu(), torch.zeros(B * T, d), B, T, NH, hd)
    rows, ar = torch.tensor(lens) - 1, torch.arange(B)
    q3 = qrot.view(B, T, 3 * d)
    _case[hd] = dict(kv=q3[:, :, d:].contiguous(), q=q3[ar.cuda(), rows.cuda(), :d].contiguous(), lens=lens, B=B,
                     out=ref['out'][ar, :, rows, :].unsqueeze(2), lse=ref['lse'][ar, :, rows].unsqueeze(2))
  return _case[hd]


@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_decode_paged_vs_fp64_and_its_bit_properties(ops, hd):
  c = decode_case(ops, hd)
  B, lens = c['B'], i32(c['lens'])
  pool, table = paginate(c['kv'], c['lens'], 1)
  before = pool.clone()
  out, lse = ops.attn_decode_paged(c['q'], pool, table, lens, NH, want_lse=True)
  assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
  got_o, got_l = out.double().cpu().view(B, NH, 1, hd), lse.double().cpu().view(B, NH, 1)
  m = {'row_out': PB.row_local(got_o, c['out'])}
  m['proj_out'], m['proj_slice_out'] = PB.projection(got_o, c['out'])
  m['lse'] = (got_l - c['lse']).abs().max().item()
  print(f'parity decode paged hd={hd}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  assert PB.BOUNDS['row']['out'] == 1.5e-2 and PB.BOUNDS['proj']['out'] == 3e-3 and PB.BOUNDS['proj_slice']['out'] == 3e-3 and PB.BOUNDS['lse'] == 1e-4
  assert not PB.violations(m), PB.violations(m)
  assert biteq(pool, before)  # the pool is unchanged by the call
  # another page placement: the same bits
  pool2, table2 = paginate(c['kv'], c['lens'], 2, spare=5)
  assert not torch.equal(table, table2[:, :table.shape[1]])
  out2, lse2 = ops.attn_decode_paged(c['q'], pool2, table2, lens, NH, want_lse=True)
  assert biteq(out, out2) and torch.equal(lse, lse2)
  # every sequence alone, with its own table row, at the whole table's Lcap and at the least its length needs: the bits it has in the batch
  for b in range(B):
    for Lcap in (None, -(-c['lens'][b] // PG) * PG):
      o1, l1 = ops.attn_decode_paged(c['q'][b:b + 1], pool, table[b:b + 1].contiguous(), lens[b:b + 1], NH, Lcap=Lcap, want_lse=True)
      assert biteq(o1, out[b:b + 1]) and torch.equal(l1, lse[b:b + 1]), (b, Lcap)


# ---- 3: plm_kv_paged_append_rope_rows, plm_kv_paged_store_rows --------------------------------------------------------------------------
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_paged_append_is_the_contiguous_append_at_the_pages_address(ops, hd):
  B, n, Tmax, d = 5, 7, 192, NH * hd
  g = torch.Generator().manual_seed(hd)
  qkv = torch.randn(B * n, 3 * d, generator=g).to(BF16).cuda()
  cos, sin = (t.cuda() for t in O.rope_table(hd, Tmax))
  old = torch.randn(B, Tmax, 2 * d, generator=g).to(BF16).cuda()
  lens0, n_new = (60, 0, 125, 64, 190), (7, 3, 0, 6, 7)  # across a page edge, a first row, nothing, a page's first row, past max_pages
  pool, table = paginate(old, [min(a + c, Tmax) for a, c in zip(lens0, n_new)], 3)
  table[3, 1] = -1  # a page sequence 3 needs is missing
  kv = old.clone()
  q_want, _ = ops.kv_append_rope_rows(qkv, i32(lens0), cos, sin, kv, NH, n_new=i32(n_new))
  want = pool.clone()
  for b in (0, 1):  # the sequences that are served: their new rows, at their pages
    for t in range(lens0[b], lens0[b] + n_new[b]):
      want[table[b, t // PG], t % PG] = kv[b, t]
  q, status = ops.kv_paged_append_rope_rows(qkv, i32(lens0), cos, sin, pool, table, NH, n_new=i32(n_new))
  assert int(status.item()) == 1 and biteq(pool, want)  # sequences 3 and 4 stored nothing: every other pool byte is as it was
  q, q_want = q.view(B, n, d), q_want.view(B, n, d)
  assert biteq(q[:3], q_want[:3]) and (bits(q[3:]) == 0).all()
  # served alone, nothing is refused
  _, status = ops.kv_paged_append_rope_rows(qkv[:3 * n], i32(lens0[:3]), cos, sin, pool, table[:3].contiguous(), NH, n_new=i32(n_new[:3]))
  assert int(status.item()) == 0 and biteq(pool, want)


@pytest.mark.parametrize('hd', [32, 128])
def test_paged_store_rows_is_the_contiguous_prefill_image(ops, hd):
  B, T, d = 3, 132, NH * hd
  qkv = torch.randn(B, T, 3 * d, generator=torch.Generator().manual_seed(hd)).to(BF16).cuda()
  rows, lens = qkv[:, :, d:], (132, 64, 5)  # a strided view, as prefill passes it; pad rows past lens have no page
  want, table = paginate(rows, lens, 4)
  pool = torch.full_like(want, float('nan'))
  status = ops.kv_paged_store_rows(rows, i32(lens), pool, table, NH)
  assert int(status.item()) == 0 and biteq(pool, want)
  gathered = pool[table.clamp(min=0).long()].reshape(B, -1, 2 * d)
  for b, n in enumerate(lens):
    assert biteq(gathered[b, :n], rows[b, :n])


# ---- 4: plm_attn_extend_paged -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('splits', [1, 3, 0])
@pytest.mark.parametrize('n', [1, 5, 33])
@pytest.mark.parametrize('hd', [64, 128])
def test_attn_extend_paged_vs_fp64_reference(ops, hd, n, splits):
  c = TE.extend_case(ops, hd)
  lens0 = (63, 64, 10, 128 - n, 130)  # on both sides of a page edge; sequence 3's chunk ends on one
  n_new = (n, min(n, 2), 0, n, max(n - 1, 1))
  q = TE.chunk_q(c, n, lens0, n_new, float('nan'))
  held = [a + b for a, b in zip(lens0, n_new)]
  pool, table = paginate(c['kv'], held, 5)
  out, lse = ops.attn_extend_paged(q, pool, table, i32(lens0), NH, n_new=i32(n_new), splits=splits, want_lse=True)
  want_o, want_l, valid = TE.chunk_ref(c, n, lens0, n_new, hd)
  TE.check_vs_fp64(f'extend paged hd={hd} n={n} splits={splits}', out, lse, want_o, want_l, valid, n, hd)
  pool2, table2 = paginate(c['kv'], held, 6, spare=1)
  out2, lse2 = ops.attn_extend_paged(q, pool2, table2, i32(lens0), NH, n_new=i32(n_new), splits=splits, want_lse=True)
  assert biteq(out, out2) and torch.equal(lse, lse2)  # page placement does not reach the bits


# ---- 5: the fused stage and layers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 4])
def test_fused_paged_stage_and_layers_are_their_parts_bits(ops, n):
  hd, B, Tmax, hidden, eps = 64, 3, 192, 256, 1e-6
  d = NH * hd
  g = torch.Generator().manual_seed(n)
  rnd = lambda *s, dt=BF16, k=0.1: (k * torch.randn(*s, generator=g)).to(dt).cuda()  # noqa: E731
  x = rnd(B * n, d, dt=torch.float32, k=1.0)
  an, mn = 1 + rnd(d, dt=torch.float32), 1 + rnd(d, dt=torch.float32)
  w_qkv, w_out, w_fc1, w_fc2 = rnd(3 * d, d), rnd(d, d), rnd(2 * hidden, d), rnd(d, hidden)
  cos, sin = (t.cuda() for t in O.rope_table(hd, Tmax))
  old = rnd(B, Tmax, 2 * d, k=1.0)
  lens0, n_new = (62 if n > 1 else 64, 5, 130), (n, 1, 0)  # across a page edge (n = 1: a page's first row), a ragged chunk, nothing
  held = [a + c for a, c in zip(lens0, n_new)]
  pool0, table = paginate(old, held, 10 + n)
  l0, nn = i32(lens0), i32(n_new)
  # the stage: ops.extend_norm_qkv_append's q and rows, at the pages' addresses
  kv = old.clone()
  q_want, _ = ops.extend_norm_qkv_append(x, an, eps, w_qkv, l0, cos, sin, kv, NH, n_new=nn)
  want = pool0.clone()
  for b in range(B):
    for t in range(lens0[b], held[b]):
      want[table[b, t // PG], t % PG] = kv[b, t]
  pool = pool0.clone()
  q, status = ops.extend_norm_qkv_append_paged(x, an, eps, w_qkv, l0, cos, sin, pool, table, NH, n_new=nn)
  assert int(status.item()) == 0 and biteq(q, q_want) and biteq(pool, want)

  def by_stages(attend):  # the layer's five stages, one ops call each
    xs, ps = x.clone(), pool0.clone()
    qs, _ = ops.extend_norm_qkv_append_paged(xs, an, eps, w_qkv, l0, cos, sin, ps, table, NH, n_new=nn)
    ops.decode_gemm_residual(xs, attend(qs, ps), w_out)
    ops.decode_gemm_residual(xs, ops.decode_norm_fc1_act(xs, mn, eps, w_fc1, 'glu'), w_fc2)
    return xs, ps

  W = (an, mn, eps, w_qkv, w_out, w_fc1, w_fc2)
  xs, ps = by_stages(lambda qs, ps: ops.attn_extend_paged(qs, ps, table, l0, NH, n_new=nn))
  xl, pl = x.clone(), pool0.clone()
  ops.extend_layer_paged(xl, *W, l0, nn, cos, sin, pl, table, NH, 'glu', status)
  assert torch.isfinite(xl).all() and biteq(xl, xs) and biteq(pl, ps) and not biteq(xl, x)
  if n == 1:  # the decode layer: pos = lens0, live = n_new, lens = pos + live
    lens = i32(held)
    xs, ps = by_stages(lambda qs, ps: ops.attn_decode_paged(qs, ps, table, lens, NH))
    xl, pl = x.clone(), pool0.clone()
    ops.decode_layer_paged(xl, *W, l0, lens, cos, sin, pl, table, NH, 'glu', status, live=nn)
    assert torch.isfinite(xl).all() and biteq(xl, xs) and biteq(pl, ps) and int(status.item()) == 0


# ---- 6, 7: the model ----------------------------------------------------------------------------------------------------------------------
def _model(P, mdl, seq_len=64):
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=seq_len, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  m.load_state_dict(TD._weights(mdl))
  return m.cuda()


def _scrambled_pool(m, n_pages, seed):
  pool = m.new_page_pool(n_pages)
  for t in pool.kv:
    t.fill_(float('nan'))
  ids = pool.alloc(n_pages)
  pool.free([ids[i] for i in torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed)).tolist()])
  return pool


@pytest.mark.parametrize('fused', [False, True])
def test_cached_logits_on_a_paged_cache_vs_golden(P, mdl, fused):
  m, tok, lens, T0, T = _model(P, mdl), mdl['tokens'], (16, 9), 16, 64
  pool = _scrambled_pool(m, 5, 7)
  x = tok[:, :T0].clone()
  for b, n in enumerate(lens):
    x[b, n:] = 7  # padding: must not matter, and must not need a page
  cache, first = m.prefill_paged(x.cuda(), pool, lens, logits=True)
  assert pool.n_free == 3
  rows = [first]
  for i in range(T - max(lens)):
    rows.append(m.decode_step(torch.stack([tok[b, lens[b] + i] for b in range(2)]).cuda(), cache, logits=True, fused=fused))
  cache.check()
  logits = torch.stack(rows, dim=1)
  assert cache.lens.tolist() == [n + T - max(lens) for n in lens]
  for b, n in enumerate(lens):
    e = TD.relmax(logits[b].float(), mdl['logits'][b, n - 1:n + 48])
    print(f'paged cache, ragged prompts, fused={fused}: sequence {b}: relmax {e:.2e}')
    assert e < 2e-2, (b, e)
  # a chunk through extend on a fresh paged cache: the same bound
  cache2 = m.new_cache_paged(2, pool, 64)
  cache2.set_lens([0, 0])
  Tc = 16 if fused else 24  # fused: B * n <= ops.FUSED_EXTEND_MAX_ROWS chunk rows
  lg = m.extend(tok[:, :Tc].cuda(), cache2, logits=True, all_rows=True, fused=fused)
  cache2.check()
  assert TD.relmax(lg.float(), mdl['logits'][:, :Tc]) < 2e-2


@pytest.mark.parametrize('fused', [False, True])
def test_serve_continuous_batching_against_the_full_forward(P, mdl, fused):
  m = _model(P, mdl, seq_len=192)
  tok = mdl['tokens'].reshape(-1)
  plen, budget = (5, 60, 17, 33, 9), [70, 12, 40, 8, 20]  # sequences 0 and 1 cross a page edge while decoding
  prompts, o = [], 0
  for n in plen:
    prompts.append(tok[o:o + n].cuda())
    o += n
  with torch.no_grad():
    free_run = m.serve(prompts, budget, max_batch=2, pool=_scrambled_pool(m, 3, 8), fused=fused)
    assert [t.numel() for t in free_run] == budget
    eos = int(free_run[2][10])  # sequence 2 ends through eos_id, at the latest at its 11th token
    pool = _scrambled_pool(m, 3, 9)  # 2 slots, 3 pages, 7 pages' worth of sequences: pages are reused after a release
    outs = m.serve(prompts, budget, max_batch=2, pool=pool, eos_id=eos, fused=fused)
    assert pool.n_free == 3
    again = m.serve(prompts, budget, max_batch=2, pool=pool, eos_id=eos, fused=fused)
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
      print(f'serve fused={fused}: sequence {i}: {t.numel()} tokens, worst (row max - chosen logit) {gap:.3e} against 4 eps = {4 * eps:.3e}')
      assert gap <= 4 * eps, i  # every generated position, none excluded
