"""KV-cached generation on a real MI355X: plm_kv_append_rope against the stand-alone RoPE pass (bit equality), plm_attn_decode against
the fp64 attention reference under oracle/parity.py's bounds and its bit-equality properties (empty length, stale cache tail,
determinism, independence of the rest of the batch), the cached model teacher-forced against the golden logits, and generate."""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cpu_ref as O  # noqa: E402
from oracle import parity as PB  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BF16 = torch.bfloat16


@pytest.fixture(scope='module')
def P():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  import plainlm_amd
  return plainlm_amd


@pytest.fixture(scope='module')
def ops(P):
  from plainlm_amd import ops as _ops
  return _ops


def bits(t):
  return t.contiguous().view(torch.int16)


def biteq(a, b):
  return torch.equal(bits(a), bits(b))


# ---- plm_kv_append_rope ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hd', [32, 64, 128])
@pytest.mark.parametrize('nh', [1, 3])
def test_kv_append_rope_is_rope_qk_at_the_given_positions(ops, nh, hd):
  B, Tmax, d = 5, 40, nh * hd
  g = torch.Generator().manual_seed(100 * nh + hd)
  qkv = torch.randn(B, 3 * d, generator=g).to(BF16).cuda()
  cos, sin = (t.cuda() for t in O.rope_table(hd, Tmax))
  sentinel_kv = torch.randn(B, Tmax, 2 * d, generator=g).to(BF16).cuda()
  sentinel_q = torch.randn(B, d, generator=g).to(BF16).cuda()
  for positions, skipped in (((0, 1, 17, 38, 39), None), ((39, 0, Tmax, 17, 1), 2), ((3, -1, 5, 7, 9), 1)):
    pos = torch.tensor(positions, dtype=torch.int32).cuda()
    kv, q_out = sentinel_kv.clone(), sentinel_q.clone()
    q, status = ops.kv_append_rope(qkv, pos, cos, sin, kv, nh, q_out=q_out)
    assert q.data_ptr() == q_out.data_ptr()
    # the yardstick: the same values at the same positions of a [B, Tmax] layout through the stand-alone RoPE pass
    full = torch.zeros(B, Tmax, 3 * d, dtype=BF16, device='cuda')
    for b, t in enumerate(positions):
      if b != skipped:
        full[b, t] = qkv[b]
    rot = ops.rope_qk_(full.view(B * Tmax, 3 * d), cos, sin, B, Tmax, nh).view(B, Tmax, 3 * d)
    want_kv = sentinel_kv.clone()
    for b, t in enumerate(positions):
      if b == skipped:
        assert biteq(q[b], sentinel_q[b])  # untouched
        continue
      assert biteq(q[b], rot[b, t, :d]), (b, t)
      assert biteq(kv[b, t, :d], rot[b, t, d:2 * d]), (b, t)
      assert biteq(kv[b, t, d:], qkv[b, 2 * d:]), (b, t)  # v: a bit copy
      assert not biteq(q[b], qkv[b, :d]) or t == 0  # position 0 is the identity rotation
      want_kv[b, t] = kv[b, t]
    assert biteq(kv, want_kv)  # no other cache row changed, the skipped sequence's rows included
    assert int(status.item()) == (0 if skipped is None else 1)


# ---- plm_attn_decode ------------------------------------------------------------------------------------------------------------------
B_, NH, T_ = 5, 3, 200
LENS = (1, 2, 13, 129, 200)
_case = {}


def decode_case(ops, hd):
  """Rotated qkv for [B, T], drawn as test_attention_fwd_bwd draws it, its fp64 reference (computed once per head dim, never modified)
  and the decode operands cut from it: the cache = the k | v columns, q = row lens[b] - 1 of every sequence."""
  if hd not in _case:
    d = NH * hd
    g = torch.Generator().manual_seed(T_ * NH + hd)
    qkv = torch.randn(B_ * T_, 3 * d, generator=g).to(BF16)
    cos, sin = (t.cuda() for t in O.rope_table(hd, T_))
    qrot = ops.rope_qk_(qkv.cuda(), cos, sin, B_, T_, NH)
    ref = PB.reference(qrot.cpu(), torch.zeros(B_ * T_, d), B_, T_, NH, hd)
    rows = torch.tensor(LENS) - 1
    ar = torch.arange(B_)
    q3 = qrot.view(B_, T_, 3 * d)
    _case[hd] = dict(kv=q3[:, :, d:].contiguous(), q=q3[ar.cuda(), rows.cuda(), :d].contiguous(),
                     lens=torch.tensor(LENS, dtype=torch.int32).cuda(),
                     out=ref['out'][ar, :, rows, :].unsqueeze(2), lse=ref['lse'][ar, :, rows].unsqueeze(2))  # [B, nh, 1, hd], [B, nh, 1]
  return _case[hd]


@pytest.mark.parametrize('splits', [1, 2, 7, 64, 0])
@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_decode_vs_fp64_reference(ops, hd, splits):
  c = decode_case(ops, hd)
  out, lse = ops.attn_decode(c['q'], c['kv'], c['lens'], NH, splits=splits, want_lse=True)
  assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()  # with 64 splits most ranges of the short sequences are empty
  got_o = out.double().cpu().view(B_, NH, 1, hd)
  got_l = lse.double().cpu().view(B_, NH, 1)
  m = {'row_out': PB.row_local(got_o, c['out'])}
  m['proj_out'], m['proj_slice_out'] = PB.projection(got_o, c['out'])
  m['lse'] = (got_l - c['lse']).abs().max().item()
  print(f'parity decode hd={hd} splits={splits}: ' + ' '.join(f'{k}={v:.2e}' for k, v in m.items()))
  assert PB.BOUNDS['row']['out'] == 1.5e-2 and PB.BOUNDS['proj']['out'] == 3e-3 and PB.BOUNDS['proj_slice']['out'] == 3e-3 and PB.BOUNDS['lse'] == 1e-4
  bad = PB.violations(m)
  assert not bad, bad
  # lse NULL: the same out
  assert biteq(ops.attn_decode(c['q'], c['kv'], c['lens'], NH, splits=splits), out)


@pytest.mark.parametrize('hd', [32, 64, 128])
def test_attn_decode_bit_equalities(ops, hd):
  c = decode_case(ops, hd)
  q, kv, lens = c['q'], c['kv'], c['lens']
  d = NH * hd
  for splits in (1, 2, 7, 64, 0):
    out, lse = ops.attn_decode(q, kv, lens, NH, splits=splits, want_lse=True)
    # determinism
    out2, lse2 = ops.attn_decode(q, kv, lens, NH, splits=splits, want_lse=True)
    assert biteq(out, out2) and torch.equal(lse, lse2), splits
    # empty length: out = 0, lse = +inf - for one sequence of the batch, the others unchanged, and for all of them
    l0 = lens.clone()
    l0[3] = 0
    o0, s0 = ops.attn_decode(q, kv, l0, NH, splits=splits, want_lse=True)
    assert (bits(o0[3]) == 0).all() and (s0[3] == float('inf')).all(), splits
    keep = [0, 1, 2, 4]
    assert biteq(o0[keep], out[keep]) and torch.equal(s0[keep], lse[keep]), splits
    oz, sz = ops.attn_decode(q, kv, torch.zeros_like(lens), NH, splits=splits, want_lse=True)
    assert (bits(oz) == 0).all() and (sz == float('inf')).all(), splits
    on, sn = ops.attn_decode(q, kv, torch.full_like(lens, -5), NH, splits=splits, want_lse=True)  # clamped to 0
    assert (bits(on) == 0).all() and (sn == float('inf')).all(), splits
    # stale tail: NaN patterns in the rows at and beyond lens[b] against a zero tail
    kv_nan, kv_zero = kv.clone(), kv.clone()
    for b, n in enumerate(LENS):
      kv_nan[b, n:] = float('nan')
      kv_zero[b, n:] = 0
    assert torch.isnan(kv_nan[0, 1:].float()).all()
    on_, sn_ = ops.attn_decode(q, kv_nan, lens, NH, splits=splits, want_lse=True)
    oz_, sz_ = ops.attn_decode(q, kv_zero, lens, NH, splits=splits, want_lse=True)
    assert biteq(on_, oz_) and torch.equal(sn_, sz_) and biteq(on_, out), splits
    # lens beyond Tmax are clamped to it
    ob, sb = ops.attn_decode(q, kv, torch.tensor([1, 2, 13, 129, 5000], dtype=torch.int32).cuda(), NH, splits=splits, want_lse=True)
    assert biteq(ob, out) and torch.equal(sb, lse), splits
    # independence: a sequence alone, with the same forced split count, gives what it gives inside the batch
    if splits != 0:
      for b in range(B_):
        o1, s1 = ops.attn_decode(q[b:b + 1].contiguous(), kv[b:b + 1].contiguous(), lens[b:b + 1].contiguous(), NH, splits=splits, want_lse=True)
        assert biteq(o1[0], out[b]) and torch.equal(s1[0], lse[b]), (splits, b)
  assert q.shape == (B_, d)


# ---- the model, teacher-forced ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mdl(golden_dir):
  z = np.load(os.path.join(golden_dir, 'model.npz'))
  return {k: torch.from_numpy(z[k]) for k in z.files}


def _weights(mdl):
  return {k[2:]: v for k, v in mdl.items() if k.startswith('w:')}


def _small(P, mdl):
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  m.load_state_dict(_weights(mdl))
  return m.cuda()


def relmax(a, ref):
  a, ref = a.double().cpu(), ref.double().cpu()
  return ((a - ref).abs().max() / ref.abs().max()).item()


def _teacher_forced(m, tok, prompt_lens, T0=16, T=64):
  """Prefill tok[:, :T0] (sequence b's true prompt: its first prompt_lens[b] tokens, the rest of its row is padding), then feed every
  sequence its own true next tokens until the longest reaches T.  Returns (cache after prefill's kv clones, per-sequence logits
  [T - prompt_lens[b] + 1 ... ] aligned to positions prompt_lens[b] - 1 ... )."""
  B = tok.shape[0]
  x = tok[:, :T0].clone()
  for b, n in enumerate(prompt_lens):
    x[b, n:] = 7  # padding: must not matter
  cache, first = m.prefill(x.cuda(), None if all(n == T0 for n in prompt_lens) else prompt_lens, logits=True)
  kv0 = [t.clone() for t in cache.kv]
  steps = T - max(prompt_lens)
  rows = [first]
  for i in range(steps):
    nxt = torch.stack([tok[b, prompt_lens[b] + i] for b in range(B)]).cuda()
    rows.append(m.decode_step(nxt, cache, logits=True))
  cache.check()
  assert cache.lens.tolist() == [n + steps for n in prompt_lens]
  return kv0, torch.stack(rows, dim=1)  # [B, steps + 1, V]: sequence b's positions prompt_lens[b] - 1 + (0 .. steps)


def test_cached_logits_vs_golden_and_prefill_cache_bits(P, ops, mdl, monkeypatch):
  m = _small(P, mdl)
  tok = mdl['tokens']
  kv0, logits = _teacher_forced(m, tok, (16, 16))
  assert logits.dtype == BF16 and tuple(logits.shape) == (2, 49, 256)
  e = relmax(logits.float(), mdl['logits'][:, 15:64])
  print(f'teacher-forced cached logits vs golden, positions 15..63: relmax {e:.2e}')
  assert e < 2e-2
  # what prefill left in the cache is what the trunk's rotated qkv holds, bit for bit
  seen = []
  real = ops.qkv_rope
  monkeypatch.setattr(ops, 'qkv_rope', lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
  m(tok[:, :16].cuda(), None)
  assert len(seen) == 2
  for layer, qkv in enumerate(seen):
    assert biteq(kv0[layer][:, :16], qkv.view(2, 16, 3 * 128)[:, :, 128:]), layer


def test_cached_logits_with_ragged_prompt_lens(P, mdl):
  m = _small(P, mdl)
  tok = mdl['tokens']
  lens = (16, 9)
  _, logits = _teacher_forced(m, tok, lens)
  assert tuple(logits.shape) == (2, 49, 256)
  for b, n in enumerate(lens):  # each sequence against the golden rows at its own offsets
    e = relmax(logits[b].float(), mdl['logits'][b, n - 1:n + 48])
    print(f'ragged prompts: sequence {b} positions {n - 1}..{n + 47}: relmax {e:.2e}')
    assert e < 2e-2, (b, e)


# What one decode_step of the golden 2-layer model issues through the C ABI, recorded with the hook below on commit 37fafa5 (the last
# one with decode_step and extend written out separately): embedding; per layer norm, qkv, append, attention, out, norm, fc1, SwiGLU,
# fc2; the out norm; the fused prediction head.
DECODE_STEP_LAUNCHES = [
  'plm_embed_fwd',
  'plm_rmsnorm_fwd', 'plm_gemm_bf16_nt', 'plm_kv_append_rope', 'plm_attn_decode', 'plm_gemm_bf16_nt', 'plm_rmsnorm_fwd', 'plm_gemm_bf16_nt',
  'plm_swiglu_fwd', 'plm_gemm_bf16_nt',
  'plm_rmsnorm_fwd', 'plm_gemm_bf16_nt', 'plm_kv_append_rope', 'plm_attn_decode', 'plm_gemm_bf16_nt', 'plm_rmsnorm_fwd', 'plm_gemm_bf16_nt',
  'plm_swiglu_fwd', 'plm_gemm_bf16_nt',
  'plm_rmsnorm_fwd', 'plm_head_predict_bf16']


def test_decode_step_and_extend_issue_the_same_launches(P, mdl, monkeypatch):
  """'The same launches as one decode step, whatever n': one decode_step issues the recorded list, one extend of n = 3 the same list with
  the two cached-attention entry points replaced by their chunk forms."""
  from plainlm_amd import _lib
  m = _small(P, mdl)
  tok = mdl['tokens'].cuda()
  cache, _ = m.prefill(tok[:, :16])
  calls = []
  real = _lib.check
  monkeypatch.setattr(_lib, 'check', lambda rc, what: calls.append(what) or real(rc, what))
  m.decode_step(tok[:, 16], cache)
  assert calls == DECODE_STEP_LAUNCHES, calls
  del calls[:]
  m.extend(tok[:, 17:20], cache)
  chunk = {'plm_kv_append_rope': 'plm_kv_append_rope_rows', 'plm_attn_decode': 'plm_attn_extend'}
  assert calls == [chunk.get(c, c) for c in DECODE_STEP_LAUNCHES], calls
  monkeypatch.undo()
  cache.check()
  assert cache.lens.tolist() == [20, 20]


@pytest.mark.parametrize('mlp,nh', [('mlp', 2), ('mlp_relu_sq', 2), ('glu', 4), ('glu', 1)])
def test_cached_logits_other_mlp_classes_and_head_dims_vs_oracle(P, mlp, nh):
  ocfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=nh, mlp=mlp)
  w = O.init_params(ocfg, seed=31 + nh)
  tok = torch.from_numpy(np.random.default_rng(nh).integers(0, 256, size=(2, 64)))
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=nh, mlp=mlp))
  m.load_state_dict(w)
  m = m.cuda()
  _, logits = _teacher_forced(m, tok, (16, 16))
  with torch.no_grad():
    ref = O.forward(w, ocfg, tok)
  e = relmax(logits.float(), ref[:, 15:64])
  print(f'cached logits mlp={mlp} head_dim={128 // nh} vs fp32 oracle: relmax {e:.2e}')
  assert e < 2e-2


# ---- generate ----------------------------------------------------------------------------------------------------------------------------
def test_generate_greedy_against_the_full_forward(P, mdl):
  m = _small(P, mdl)
  prompt = mdl['tokens'][:, :16].cuda()
  N = 32
  with torch.no_grad():
    toks, lps = m.generate(prompt, N, return_logprobs=True)
    assert toks.dtype == torch.int64 and tuple(toks.shape) == (2, N) and lps.dtype == torch.float32 and tuple(lps.shape) == (2, N)
    seq = torch.cat([prompt, toks], dim=1)  # [2, 48]
    full = m(seq, None).float()  # row 15 + i predicts generated token i
    eps = 2e-2 * full.abs().max().item()
    rows = full[:, 15:15 + N]
    chosen = rows.gather(2, toks[:, :, None])[:, :, 0]
    gap = (rows.max(dim=-1).values - chosen).max().item()
    share = (rows.argmax(-1) == toks).float().mean().item()
    print(f'generate vs full forward: worst (row max - chosen logit) {gap:.3e} against 4 eps = {4 * eps:.3e}; exact matches with the '
          f'recompute argmax {share:.4f}')
    assert gap <= 4 * eps  # every generated position, none excluded
    # log-probabilities: predict's for the same tokens
    tg = torch.full_like(seq, -100)
    tg[:, 15:15 + N] = toks
    want = -m.predict(seq, targets=tg).nll[:, 15:15 + N]
    assert (lps - want).abs().max().item() <= eps, ((lps - want).abs().max().item(), eps)
    assert (lps <= 0).all()
    # two runs are bit-equal
    t2, l2 = m.generate(prompt, N, return_logprobs=True)
    assert torch.equal(t2, toks) and torch.equal(l2, lps)
    assert torch.equal(m.generate(prompt, N), toks)
    # eos: a token that appears; everything after its first appearance in a row is frozen
    eos = int(toks[0, 5].item())
    te, le = m.generate(prompt, N, eos_id=eos, return_logprobs=True)
    froze = 0
    for b in range(2):
      hit = (toks[b] == eos).nonzero()
      n = int(hit[0]) + 1 if len(hit) else N
      froze += N - n
      assert torch.equal(te[b, :n], toks[b, :n]) and torch.equal(le[b, :n], lps[b, :n]), b
      assert (te[b, n:] == eos).all() and (le[b, n:] == 0).all(), b
    assert froze > 0
    # a sampler that takes the argmax of the logits it is given reproduces greedy wherever its own top-2 margin is not zero
    margins = []

    def sample(logits):
      assert logits.dtype == torch.float32 and tuple(logits.shape) == (2, 256)
      top = logits.topk(2, dim=-1).values
      margins.append(top[:, 0] - top[:, 1])
      return logits.argmax(-1)
    ts, ls = m.generate(prompt, N, sample=sample, return_logprobs=True)
    clear = torch.stack(margins, dim=1) != 0
    assert tuple(clear.shape) == (2, N) and clear.float().mean().item() > 0.5
    assert torch.equal(ts[clear], toks[clear])
    assert ((ls - lps).abs()[clear] <= eps).all()
  # refusals that need the GPU to be reached
  with pytest.raises(RuntimeError, match='forward-only'):
    m.generate(prompt, 4)
  with torch.no_grad(), pytest.raises(ValueError, match='exceeds cfg.seq_len'):
    m.generate(prompt, 49)
  with torch.no_grad():
    ragged = m.generate(prompt, 8, prompt_lens=(16, 9))
    assert torch.equal(ragged[0], m.generate(prompt, 8)[0])  # sequence 0 does not see what sequence 1 holds
