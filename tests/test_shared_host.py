"""Shared-prefix decoding without a GPU: every refusal comes before anything is launched, the split rule and the
workspace size are pure functions of the shapes, and SharedPrefixCache keeps its books on any device."""

import pytest
import torch

import plainlm_amd
from plainlm_amd import _lib, generate as Gn


def small(**kw):
  cfg = dict(vocab_size=64, seq_len=64, dim=64, expand=2, n_layers=2, n_heads=2, mlp='glu')
  cfg.update(kw)
  return plainlm_amd.Transformer(plainlm_amd.ModelConfig(**cfg))


def prefix(P=2, Tmax=12, lens=(12, 5), kv_dtype='bf16'):
  c = Gn.KVCache(2, P, Tmax, 2, 32, 'cpu', kv_dtype)
  c.set_lens(torch.tensor(lens, dtype=torch.int32))
  return c


def test_shared_prefix_cache_bookkeeping():
  c = Gn.SharedPrefixCache(prefix(), 3, 7)
  assert (c.P, c.G, c.B, c.Tmax) == (2, 3, 6, 7) and c.kv_dtype == 'bf16'
  assert c.rot0.tolist() == [12, 12, 12, 5, 5, 5] and c.rot0.dtype == torch.int32
  assert [tuple(t.shape) for t in c.kv] == [(6, 7, 128)] * 2 and c.kv[0].dtype == torch.bfloat16
  assert c.pos.tolist() == [-1] * 6 and c.lens.tolist() == [0] * 6
  c.advance()
  assert c.pos.tolist() == [0] * 6 and c.lens.tolist() == [1] * 6 and c.pos.data_ptr() == c._pl.data_ptr()
  # the prefix once: (Tp_max + G * Ts_max) rows per prompt, 4 * dim bytes per row and layer
  assert c.cache_bytes() == 2 * (12 + 3 * 7) * 4 * 64 * 2
  # the issue's figures: 12 layers of 3072-byte rows, prompt 4096, 32 samples of 64 tokens, against the prompt held 32 times
  assert (4096 + 32 * 64) * 3072 * 12 == 226492416 and 32 * (4096 + 64) * 3072 * 12 == 4907335680
  c.check()
  c.status[0] = 1
  with pytest.raises(RuntimeError, match='larger max_new_tokens'):
    c.check()


def test_refusals_come_before_any_launch(monkeypatch):
  monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('a refusal reached the library'))
  monkeypatch.setattr(Gn, 'refuse_cpu', lambda t: None)  # host tensors stand in for device ones
  m = small()
  with pytest.raises(ValueError, match="'fp8' cache cannot be shared"):
    m.fork(prefix(kv_dtype='fp8'), 2, 4)
  shared = m.fork(prefix(), 2, 4)
  with pytest.raises(TypeError, match='already a fork'):
    m.fork(shared, 2, 4)
  with pytest.raises(TypeError, match='prefilled KVCache'):
    m.fork(object(), 2, 4)
  for bad in (0, True, 2.0):
    with pytest.raises(ValueError, match='n_samples'):
      m.fork(prefix(), bad, 4)
  with pytest.raises(ValueError, match='max_new_tokens'):
    m.fork(prefix(), 2, 0)
  with pytest.raises(ValueError, match='another model shape'):
    small(n_layers=3).fork(prefix(), 2, 4)
  tok = torch.zeros(4, 3, dtype=torch.int64)
  with pytest.raises(TypeError, match='decode steps only'):
    m.extend(tok, shared)
  with pytest.raises(TypeError, match='decode steps only'):
    m.extend(tok, shared, fused=True)
  mx = small(linear_precision='mxfp8', dim=128)
  with pytest.raises(ValueError, match='mxfp8 has no shared-prefix'):
    mx.fork(prefix(), 2, 4)
  with pytest.raises(ValueError, match='mxfp8 has no shared-prefix'), torch.no_grad():
    mx.generate_samples(torch.zeros(1, 8, dtype=torch.int64), 2, 4)
  with pytest.raises(ValueError, match='mxfp8 has no shared-prefix'):
    mx.decode_step(torch.zeros(4, dtype=torch.int64), shared)
  with pytest.raises(ValueError, match='leave fused off'):  # P * G = 2 * 17 rows
    m.decode_step(torch.zeros(34, dtype=torch.int64), m.fork(prefix(), 17, 4), fused=True)
  with pytest.raises(ValueError, match='do not match the cache'):
    m.decode_step(torch.zeros(3, dtype=torch.int64), shared)


@pytest.mark.parametrize('bad', [dict(n_samples=0), dict(max_new_tokens=0), dict(max_new_tokens=60), dict(top_p=2.0), dict(temperature=-1.0),
                                 dict(n_samples=17, fused=True)])
def test_generate_samples_refuses_before_the_prefill(monkeypatch, bad):
  m = small()
  monkeypatch.setattr(m, 'prefill', lambda *a, **k: pytest.fail('prefill ran'))
  monkeypatch.setattr(Gn, 'refuse_cpu', lambda t: None)  # host tensors stand in for device ones
  kw = dict(n_samples=2, max_new_tokens=4)
  kw.update(bad)
  with pytest.raises(ValueError), torch.no_grad():
    m.generate_samples(torch.zeros(2, 8, dtype=torch.int64), kw.pop('n_samples'), kw.pop('max_new_tokens'), **kw)


@pytest.mark.parametrize('P,G,nh,Tp,forced,want', [(1, 32, 12, 4096, 0, 16), (1, 8, 12, 1024, 0, 4), (1, 33, 12, 4096, 0, 16), (1, 64, 12, 65536, 0, 22),
                                                   (8, 4, 12, 4096, 0, 6), (1, 1, 1, 100000, 0, 64), (2, 5, 2, 255, 0, 1), (2, 5, 2, 257, 0, 2),
                                                   (2, 5, 2, 300, 3, 3)])
def test_split_rule_and_workspace_are_pure_functions_of_the_shapes(P, G, nh, Tp, forced, want):
  """Two workgroups per CU (256 of them) over P * nh * ceil(G / 32) workgroups per split, no split under 256 keys of Tp_max, at most 64;
  the workspace holds (S_p + S_s) fp32 partials (m, l, acc[hd]) per (sample, head), a multiple of 16 bytes: the library's answer pins S_p."""
  lib = _lib.load()
  assert want == (forced or max(1, min(-(-512 // (P * nh * -(-G // 32))), -(-Tp // 256), 64)))
  hd, Ts = 64, 64
  Ss = _decode_splits(lib, P * G, nh, hd, Ts)
  need = (P * G * nh * (want + Ss) * (2 + hd) * 4 + 15) // 16 * 16
  assert lib.plm_attn_decode_shared_workspace_bytes(P, G, nh, hd, Tp, Ts, forced, 0) == need
  hidden = 96
  rows = P * G * (2 * nh * hd * 2 + hidden * 2)
  assert lib.plm_decode_layer_shared_workspace_bytes(P, G, nh, hd, hidden, Tp, Ts, forced, 0) == (need + rows if P * G <= 32 else 0)


def _decode_splits(lib, B, nh, hd, Tmax):
  """plm_attn_decode's automatic split count, read off its workspace size."""
  return lib.plm_attn_decode_workspace_bytes(B, nh, hd, Tmax, 0) // (B * nh * (2 + hd) * 4)


def test_workspace_queries_refuse_what_the_launches_refuse():
  lib = _lib.load()
  ok = (2, 5, 2, 64, 300, 9, 0, 0)
  assert lib.plm_attn_decode_shared_workspace_bytes(*ok) > 0
  for i, v in ((0, 0), (1, 0), (3, 48), (4, 0), (5, 0), (6, 65), (7, -1)):
    bad = list(ok)
    bad[i] = v
    assert lib.plm_attn_decode_shared_workspace_bytes(*bad) == 0, bad
  assert lib.plm_decode_layer_shared_workspace_bytes(2, 17, 2, 64, 96, 300, 9, 0, 0) == 0  # P * G > 32
