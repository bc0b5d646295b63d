"""Muon without a GPU: optim.Muon against torch.optim.Muon + torch.optim.AdamW bit for bit, the parameter partition
on the small golden model, the state_dict layout, every refusal, the argument checks and the workspace arithmetic of the new entry points,
the header / binding agreement, and the exact class on the torch reference."""

import ctypes as C
import os
import sys
from collections import namedtuple

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import muon_ref as MR  # noqa: E402

from plainlm_amd import _lib, engine, optim  # noqa: E402
from plainlm_amd import ops  # noqa: E402

SHAPES = [(16, 16), (48, 16), (16, 40), (50, 16), (16,)]  # three matrices, an embedding, a vector


@pytest.mark.parametrize('adjust_lr', ['match_rms_adamw', 'original'])
@pytest.mark.parametrize('nesterov', [True, False])
def test_twin_equals_torch_muon_plus_adamw_bit_for_bit(adjust_lr, nesterov):
  g = torch.Generator().manual_seed(0)
  ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]
  qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
  kw = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
  ours = optim.Muon([{'params': ps[:3], 'use_muon': True}, {'params': ps[3:]}], nesterov=nesterov, adjust_lr=adjust_lr, **kw)
  tm = torch.optim.Muon(qs[:3], lr=kw['lr'], weight_decay=kw['weight_decay'], nesterov=nesterov, adjust_lr_fn=adjust_lr)
  ta = torch.optim.AdamW(qs[3:], **kw)
  for step in range(3):
    for p, q in zip(ps, qs):
      grad = torch.randn(p.shape, generator=g)
      p.grad, q.grad = grad.clone(), grad.clone()
    for grp in ours.param_groups + tm.param_groups + ta.param_groups:
      grp['lr'] = kw['lr'] * (step + 1) / 3
    ours.step()
    tm.step()
    ta.step()
    for i, (p, q) in enumerate(zip(ps, qs)):
      assert torch.equal(p.detach(), q.detach()), (step, i)
  for p, q in zip(ps[:3], qs[:3]):
    assert set(ours.state[p]) == {'momentum_buffer'} and torch.equal(ours.state[p]['momentum_buffer'], tm.state[q]['momentum_buffer'])
  for p, q in zip(ps[3:], qs[3:]):
    assert set(ours.state[p]) == {'step', 'exp_avg', 'exp_avg_sq'}
    assert all(torch.equal(ours.state[p][k], ta.state[q][k]) for k in ('step', 'exp_avg', 'exp_avg_sq'))
  sd = ours.state_dict()
  assert [set(sd['state'][i]) for i in range(5)] == [{'momentum_buffer'}] * 3 + [{'step', 'exp_avg', 'exp_avg_sq'}] * 2
  assert [grp['use_muon'] for grp in sd['param_groups']] == [True, False]


def test_newton_schulz_is_torchs():
  from torch.optim._muon import _zeropower_via_newtonschulz
  g = torch.Generator().manual_seed(1)
  for s in ((16, 40), (48, 16), (32, 32)):
    u = torch.randn(s, generator=g)
    assert torch.equal(optim.newton_schulz(u), _zeropower_via_newtonschulz(u, MR.COEFFS, 5, MR.EPS))
  assert ops.MUON_NS_COEFFICIENTS == MR.COEFFS and ops.MUON_EPS == MR.EPS


def _small(tie=False):
  import plainlm_amd as P
  return P, P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu', tie_embeddings=tie))


@pytest.mark.parametrize('tie', [False, True])
def test_partition_of_the_small_model(tie):
  P, m = _small(tie)
  groups = optim.muon_param_groups(m, P.get_param_groups(m, 0.1))
  name = {id(p): n for n, p in m.named_parameters()}
  got = [sorted(name[id(p)] for p in g['params']) for g in groups]
  assert [g['use_muon'] for g in groups] == [True, False, False] and [g['weight_decay'] for g in groups] == [0.1, 0.1, 0.0]
  assert len(got[0]) == 8 and all(n.startswith('layers.') and n.endswith('.weight') and 'norm' not in n for n in got[0])
  assert all(m.get_parameter(n).ndim == 2 for n in got[0])
  assert got[1] == sorted(n for n in name.values() if not n.startswith('layers.') and 'norm' not in n)
  assert any('embed_tokens' in n or 'lm_head' in n for n in got[1]) and not any('lm_head' in n or 'embed' in n for n in got[0])
  assert got[2] and all('norm' in n for n in got[2])
  assert sum(len(x) for x in got) == len(name)


def test_refusals():
  p = [torch.nn.Parameter(torch.zeros(16, 16))]
  kw = dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1)
  with pytest.raises(ValueError, match='muon_adjust_lr'):
    optim.Muon(p, adjust_lr='keller', **kw)
  for steps in (0, -1, 2.5, 100):
    with pytest.raises(ValueError, match='ns_steps'):
      optim.Muon(p, ns_steps=steps, **kw)
  for mom in (-0.1, 1.0, 1.5):
    with pytest.raises(ValueError, match='momentum'):
      optim.Muon(p, momentum=mom, **kw)
  with pytest.raises(ValueError, match='not 2-D'):
    optim.Muon([{'params': [torch.nn.Parameter(torch.zeros(16))], 'use_muon': True}], **kw)
  with pytest.raises(ValueError, match='muon_adjust_lr'):
    ops.muon_adjusted_lr(1e-3, None, 16, 16)
  # the engine's factory
  P, m = _small()
  EC = dict(optim='muon', fused_optim=True, lr=3e-3, weight_decay=0.1, beta1=0.9, beta2=0.95)
  cfg = lambda **over: namedtuple('Config', list(EC) + list(over))(**EC, **over)  # noqa: E731
  groups = P.get_param_groups(m, 0.1)
  with pytest.raises(RuntimeError, match='enable_main_grad'):
    engine.intialize_optimizer(groups, cfg(), m)
  with pytest.raises(ValueError, match='needs the model'):
    engine.intialize_optimizer(groups, cfg(), None)
  with pytest.raises(ValueError, match='muon_adjust_lr'):
    engine.intialize_optimizer(groups, cfg(muon_adjust_lr='keller', ), m)
  with pytest.raises(ValueError, match='ns_steps'):
    engine.intialize_optimizer(groups, cfg(muon_ns_steps=0), m)
  with pytest.raises(ValueError, match='momentum'):
    engine.intialize_optimizer(groups, cfg(muon_momentum=1.0), m)
  mx = P.Transformer(P.ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=1, n_heads=2, mlp='glu', linear_precision='mxfp8'))
  with pytest.raises(NotImplementedError, match='mxfp8'):
    engine.intialize_optimizer(P.get_param_groups(mx, 0.1), cfg(), mx)
  twin = engine.intialize_optimizer(groups, namedtuple('Config', list(EC))(**dict(EC, fused_optim=False)), m)
  assert type(twin) is optim.Muon and twin.defaults['momentum'] == 0.95 and twin.defaults['nesterov'] is True and \
    twin.defaults['ns_steps'] == 5 and twin.defaults['adjust_lr'] == 'match_rms_adamw'


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------------------
def _rc(name, *args):
  lib = _lib.load()
  rc = getattr(lib, name)(*args)
  return rc, (lib.plm_last_error_string() or b'').decode()


def _i64(*v):
  return (C.c_int64 * len(v))(*v)


def test_header_bindings_and_abi():
  names = set(_lib.header_functions())
  new = {'plm_gemm_bf16_nt_batched', 'plm_muon_workspace_bytes', 'plm_muon_prepare', 'plm_muon_orthogonalize', 'plm_muon_apply'}
  assert new <= names and names == set(_lib.SIGNATURES)
  assert _lib.EXPECTED_ABI == 112 and _lib.load().plm_version() == 112
  assert C.sizeof(_lib.NtBatchItem) == 10 * 8 + 3 * 8 + 2 * 4 and C.sizeof(_lib.MuonItem) == 5 * 8 + 3 * 8 + 8
  assert _lib.NT_BATCH_GROUP == 32 and '#define PLM_NT_BATCH_GROUP 32' in open(_lib.HEADER_PATH).read()


def test_workspace_query_arithmetic():
  lib = _lib.load()
  shapes = [(64, 96), (96, 64), (768, 768), (2304, 768), (72, 200)]
  blocks, block_bytes, tiles = ops.muon_layout(shapes)
  want = sum(2 * (4 * min(r, c) * max(r, c) + 2 * min(r, c) ** 2) for r, c in shapes)
  assert block_bytes == want and tiles == sum(-(-r // 64) * -(-c // 64) for r, c in shapes)
  assert ops.muon_workspace_bytes(shapes) == want + -(-4 * tiles // 16) * 16
  assert blocks[1].m == 64 and blocks[1].n == 96 and blocks[1].x[0] == blocks[0].bm + 64 * 64   # contiguous, in list order
  for b in blocks:
    assert b.xt[0] == b.x[0] + b.m * b.n and b.x[1] == b.xt[0] + b.m * b.n and b.a == b.xt[1] + b.m * b.n and b.bm == b.a + b.m * b.m
  # the 160M shape: 12 layers of w_qkv, w_out, a GLU fc1 and fc2 at d = 768, hidden 2048
  shapes160 = [(2304, 768), (768, 768), (4096, 768), (768, 2048)] * 12
  assert ops.muon_workspace_bytes(shapes160) == 12 * 2 * (4 * 768 * (2304 + 768 + 4096 + 2048) + 8 * 768 * 768) + 4 * 12 * (36 * 12 + 144 + 64 * 12 + 12 * 32)
  for bad in ([(64, 100)], [(0, 64)], [(64, -8)], [(1 << 16, 1 << 14)]):
    assert lib.plm_muon_workspace_bytes(_i64(*[r for r, _ in bad]), _i64(*[c for _, c in bad]), 1) == 0
    with pytest.raises(ValueError):
      ops.muon_workspace_bytes(bad)
  assert lib.plm_muon_workspace_bytes(None, None, 1) == 0 and lib.plm_muon_workspace_bytes(_i64(64), _i64(64), 0) == 0


def test_argument_checks_without_a_gpu():
  """Every refusal comes from the argument check, before anything is launched (the pointers are plausible and never dereferenced)."""
  INVALID, WORKSPACE = -1, -4
  p = 0x100000
  item = lambda **kw: _lib.NtBatchItem(**{**dict(A=p, lda=64, B=p, ldb=64, C=p, ldc=64, D=None, ldd=0, Ct=None, ldct=0, M=64, N=64, K=64,  # noqa: E731
                                              alpha=1.0, beta=0.0), **kw})
  def gemm(*items):
    t = (_lib.NtBatchItem * len(items))(*items)
    return _rc('plm_gemm_bf16_nt_batched', t, len(items), None)
  assert gemm(item(M=60))[0] == INVALID and 'multiples of 8' in gemm(item(M=60))[1]
  assert gemm(item(K=0))[0] == INVALID and gemm(item(lda=56))[0] == INVALID and gemm(item(ldc=68))[0] == INVALID
  assert gemm(item(A=None))[0] == INVALID and 'aligned' in gemm(item(B=p + 2))[1]
  assert 'ldd' in gemm(item(D=p, ldd=32))[1] and 'ldct' in gemm(item(Ct=p, ldct=60))[1]
  rc, msg = gemm(*([item()] * 40 + [item(N=12)]))   # a bad item beyond the first group: refused before the first launch
  assert rc == INVALID and 'item 40' in msg
  assert _rc('plm_gemm_bf16_nt_batched', None, 1, None)[0] == INVALID
  assert _rc('plm_gemm_bf16_nt_batched', (_lib.NtBatchItem * 1)(item()), 0, None)[0] == INVALID

  mi = lambda **kw: _lib.MuonItem(**{**dict(p=p, g=p, buf=p, dst=p, dst_t=p, rows=64, cols=96, ld_t=64, lr_adj=0.01), **kw})  # noqa: E731
  tab = lambda *it: (_lib.MuonItem * len(it))(*it)  # noqa: E731
  need = ops.muon_workspace_bytes([(64, 96)])
  prep = lambda t, n=1, mom=0.95, eps=1e-7, nrm=p, ws=p, nb=need: _rc('plm_muon_prepare', t, n, mom, 1, eps, None, nrm, ws, nb, None)  # noqa: E731
  assert prep(tab(mi(rows=60)))[0] == INVALID and prep(tab(mi(g=None)))[0] == INVALID and prep(tab(mi(buf=p + 4)))[0] == INVALID
  assert 'momentum' in prep(tab(mi()), mom=1.0)[1] and prep(tab(mi()), mom=-0.5)[0] == INVALID and prep(tab(mi()), eps=-1.0)[0] == INVALID
  assert prep(tab(mi()), nrm=None)[0] == INVALID and prep(None)[0] == INVALID and prep(tab(mi()), n=0)[0] == INVALID
  assert prep(tab(mi()), nb=need - 1)[0] == WORKSPACE and prep(tab(mi()), ws=None)[0] == WORKSPACE and prep(tab(mi()), ws=p + 8)[0] == WORKSPACE
  assert prep(tab(mi(), mi(cols=100)), n=2)[0] == INVALID
  orth = lambda r=64, c=96, n=1, steps=5, ws=p, nb=need: _rc('plm_muon_orthogonalize', _i64(r), _i64(c), n, steps, 3.4445, -4.775, 2.0315, ws, nb, None)  # noqa: E731
  assert orth(steps=0)[0] == INVALID and orth(steps=100)[0] == INVALID and orth(r=60)[0] == INVALID and orth(n=0)[0] == INVALID
  assert orth(nb=need - 1)[0] == WORKSPACE and orth(ws=None)[0] == WORKSPACE
  assert 'workspace of %d bytes' % need in orth(nb=0)[1]
  app = lambda t, n=1, steps=5, ws=p, nb=need: _rc('plm_muon_apply', t, n, 0.999, steps, ws, nb, None)  # noqa: E731
  assert app(tab(mi(p=None)))[0] == INVALID and app(tab(mi(dst_t=None)))[0] == INVALID and app(tab(mi(ld_t=56)))[0] == INVALID
  assert app(tab(mi(ld_t=68)))[0] == INVALID and app(tab(mi(dst=p + 2)))[0] == INVALID and app(tab(mi()), steps=-1)[0] == INVALID
  assert app(tab(mi()), nb=need - 16)[0] == WORKSPACE and app(None)[0] == INVALID


# ---- the exact class on the torch reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,cols', [(64, 64), (64, 128), (128, 64)])
def test_exact_class_on_the_torch_reference(rows, cols):
  """U = 0.37 P: torch's CPU iteration gives zeros where P is 0 and one value elsewhere, within one bf16 ulp of 0.69140625 for all three
  shapes; muon_ref.scalar_chain (the recurrence of the kernels' stated epilogue) lies within that ulp too, and the bf16-emulating and
  fp64 references agree with it to their precision."""
  Pm = MR.partial_permutation(rows, cols, seed=rows + cols)
  assert Pm.shape == (rows, cols) and Pm.sum() == min(rows, cols) and Pm.sum(0).max() == 1 and Pm.sum(1).max() == 1
  o = optim.newton_schulz(0.37 * Pm)
  assert not o[Pm == 0].any()
  nz = o[Pm != 0].float()
  assert (nz == nz[0]).all() and abs(nz[0].item() - 0.69140625) <= 2.0 ** -8
  chain = MR.scalar_chain(0.37, min(rows, cols))
  assert abs(chain - 0.69140625) <= 2.0 ** -8 and chain == float(np.float32(chain))
  x0, nrm = MR.x0_of(0.37 * Pm)
  emu = MR.ns_bf16(x0)
  emu = emu.t() if rows > cols else emu
  assert not emu[Pm == 0].any() and (emu[Pm != 0].float() == chain).all()
  R = MR.ns_fp64(x0)
  R = R.t() if rows > cols else R
  assert not R[Pm == 0].any() and abs(R[Pm != 0] - chain).max().item() < 2e-2
