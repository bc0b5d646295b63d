"""The workspace arena of plainlm_amd/ops.py on a real MI355X: one grow-only buffer per (device, stream) serves every wrapper that needs
scratch, so (1) no result may depend on what an earlier call left in it, and (2) the memory held is the largest request, not one buffer
per shape seen."""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
TN_CANDIDATES = ((136, 72, 1024), (128, 128, 4096), (256, 256, 16384))  # (M, N, K): a long K on few output tiles asks for split-K


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


def _calls(ops):
  """name -> a function without arguments that runs one workspace user on fixed operands and returns its result tensors."""
  from plainlm_amd import _lib
  g = torch.Generator().manual_seed(11)

  def rnd(*shape, dtype=BF16, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()

  def ids(n, V):
    return torch.randint(0, V, (n,), generator=g).cuda()
  out = {}
  for M, V, K in ((40, 1000, 64), (512, 4096, 128)):
    y, w, t = rnd(M, K), rnd(V, K, scale=0.2), ids(M, V)
    out[f'head_predict-{M}'] = lambda y=y, w=w, t=t: [r for r in ops.head_predict(y, w, t, want_lse=True)]
    if M == 40:
      out['head_score'] = lambda y=y, w=w, t=t: list(ops.head_score(y, w, t, want_lse=True))
  B, nh, hd, Tmax, n = 2, 2, 64, 256, 4  # the automatic split count is 4 here: the partials and the combine are both in use
  kv = rnd(B, Tmax, 2 * nh * hd)
  q1, qn = rnd(B, nh * hd), rnd(B * n, nh * hd)
  lens, lens0 = torch.tensor([200, 256], dtype=torch.int32).cuda(), torch.tensor([100, 252], dtype=torch.int32).cuda()
  out['attn_decode'] = lambda: list(ops.attn_decode(q1, kv, lens, nh, want_lse=True))
  out['attn_extend'] = lambda: list(ops.attn_extend(qn, kv, lens0, nh, want_lse=True))
  tn = [s for s in TN_CANDIDATES if _lib.load().plm_gemm_tn_workspace_bytes(*s) > 0]
  assert tn, 'no candidate shape of gemm_tn asks for a workspace: extend TN_CANDIDATES'
  M, N, K = tn[0]
  a, b = rnd(K, M, scale=0.1), rnd(K, N, scale=0.1)
  out['gemm_tn'] = lambda: [ops.gemm_tn(a, b)]
  tok, dout = ids(96, 512), rnd(96, 64, dtype=F32)

  def embed():
    dW = torch.empty((512, 64), dtype=F32, device='cuda')
    assert ops.embed_bwd_sorted(tok, dout, dW, False)
    return [dW]
  out['embed_bwd_sorted'] = embed
  return out


def _bits(t):
  return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.int64)


def test_no_state_crosses_calls_through_the_arena(ops):
  """Every workspace user once on a fresh arena, then all again in another order with the arena set to 0xFF bytes before every call:
  bit-equal results.  (An entry point that read a workspace byte it had not written would see the other calls' partials here.)"""
  calls = _calls(ops)
  first = {}
  for name, fn in calls.items():
    ops.release_workspaces()
    first[name] = fn()
  torch.cuda.synchronize()
  assert ops.workspace_bytes() > 0
  for order in (sorted(calls, reverse=True), sorted(calls, key=lambda s: (len(s), s))):
    for name in order:
      for buf in ops._arenas.values():
        buf.fill_(0xFF)
      again = calls[name]()
      assert len(again) == len(first[name])
      for k, (x, y) in enumerate(zip(again, first[name])):
        assert torch.equal(_bits(x), _bits(y)), (name, k)
  assert len(ops._arenas) == 1  # one device, one stream: one buffer for all of them


def test_memory_is_the_maximum_not_the_sum(ops):
  """After head_predict at M = 64 seven more row counts below it allocate nothing that stays, and KV caches of three batch sizes
  leave nothing behind when dropped.  (With one buffer per (M, V, K) kept for ever, as before the arena, memory_allocated grew by about
  0.5 MB per new row count here, and every cache shape left its decode workspace behind.)"""
  import plainlm_amd as P
  g = torch.Generator().manual_seed(5)
  V, K = 1000, 64
  w = (torch.randn(V, K, generator=g) * 0.2).to(BF16).cuda()
  ys = {M: torch.randn(M, K, generator=g).to(BF16).cuda() for M in (64, 8, 16, 24, 32, 40, 48, 56)}
  ops.release_workspaces()
  r = ops.head_predict(ys[64], w)
  del r
  torch.cuda.synchronize()
  held, base = ops.workspace_bytes(), torch.cuda.memory_allocated()
  for M in (8, 16, 24, 32, 40, 48, 56):
    r = ops.head_predict(ys[M], w)
    del r
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base and ops.workspace_bytes() == held, M
  z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'model.npz'))
  m = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  m.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')})
  m = m.cuda()
  tok = torch.from_numpy(z['tokens'])[:1, :4].cuda()
  torch.cuda.synchronize()
  base, held = torch.cuda.memory_allocated(), ops.workspace_bytes()
  for B in (1, 3, 8):  # a cache is its kv rows, its lengths and its status flag: dropped, nothing of it is left
    cache = m.new_cache(B)
    del cache
    assert torch.cuda.memory_allocated() == base and ops.workspace_bytes() == held, B
  for B in (1, 3, 8):  # a step through each cache, so that the workspaces it needs have been asked for
    cache = m.new_cache(B)
    m.extend(tok.expand(B, 4).contiguous(), cache)
    m.decode_step(tok[0, :1].expand(B).contiguous(), cache)
    cache.check()
    del cache
  torch.cuda.synchronize()
  base, held = torch.cuda.memory_allocated(), ops.workspace_bytes()
  for B in (1, 3, 8):
    cache = m.new_cache(B)
    m.extend(tok.expand(B, 4).contiguous(), cache)
    m.decode_step(tok[0, :1].expand(B).contiguous(), cache)
    del cache
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == base and ops.workspace_bytes() == held, B
