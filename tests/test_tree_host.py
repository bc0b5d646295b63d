"""Tree verification without a GPU: refusals before any launch; chunk width and workspace from the shapes alone."""

import pytest
import torch

from plainlm_amd import _lib, generate as Gn
from test_shared_host import prefix, small


def test_refusals_come_before_any_launch(monkeypatch):
  monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('a refusal reached the library'))
  monkeypatch.setattr(Gn, 'refuse_cpu', lambda t: None)  # host tensors stand in for device ones
  m = small()
  tok = lambda B, n: torch.zeros(B, n, dtype=torch.int64)  # noqa: E731
  par = lambda B, n: torch.zeros(B, n, dtype=torch.int32)  # noqa: E731
  with pytest.raises(ValueError, match="'fp8' cache has no tree path"):
    m.extend_tree(tok(2, 3), par(2, 3), prefix(kv_dtype='fp8'))
  with pytest.raises(ValueError, match="'fp8' cache has no tree path"):
    prefix(kv_dtype='fp8').commit_tree(par(2, 3), torch.zeros(2, dtype=torch.int32))
  with pytest.raises(TypeError, match='decode steps only'):
    m.extend_tree(tok(4, 3), par(4, 3), m.fork(prefix(), 2, 4))
  with pytest.raises(NotImplementedError, match='mxfp8'):
    small(linear_precision='mxfp8', dim=128).extend_tree(tok(2, 3), par(2, 3), prefix())
  with pytest.raises(ValueError, match='1 to 32 rows'):
    m.extend_tree(tok(2, 33), par(2, 33), prefix(Tmax=64))
  with pytest.raises(ValueError, match='leave fused off'):  # 2 x 17 rows
    m.extend_tree(tok(2, 17), par(2, 17), prefix(Tmax=64), fused=True)


@pytest.mark.parametrize('bad,err', [(dict(n_draft=0), ValueError), (dict(n_draft=32), ValueError), (dict(n_branch=0), ValueError),
                                     (dict(n_branch=9), ValueError), (dict(n_branch=2.0), TypeError), (dict(ngram=(3, 2)), ValueError),
                                     (dict(max_new_tokens=60), ValueError), (dict(n_draft=8, n_branch=2, fused=True), ValueError),
                                     (dict(temperature=0.8), TypeError), (dict(top_k=5), TypeError), (dict(max_rows=1), ValueError)])
def test_generate_lookup_tree_refuses_before_the_prefill(monkeypatch, bad, err):
  m = small()
  monkeypatch.setattr(m, 'prefill', lambda *a, **k: pytest.fail('prefill ran'))
  monkeypatch.setattr(Gn, 'refuse_cpu', lambda t: None)
  kw = dict(max_new_tokens=4)
  kw.update(bad)
  with pytest.raises(err), torch.no_grad():
    m.generate_lookup_tree(torch.zeros(2, 8, dtype=torch.int64), kw.pop('max_new_tokens'), **kw)


def test_chunk_width_and_workspace_are_functions_of_the_shapes_alone():
  """The chunk is min(1 + n_draft * n_branch, 32, max_rows) rows (n_branch = 1: the chain's k + 1); the workspace holds S_p prefix partials by
  plm_attn_decode_shared's rule at P = B, G = n and ONE chunk partial behind them, fp32 (m, l, acc[hd]) per (row, head)."""
  assert [Gn.tree_rows(k, nb) for k, nb in ((8, 1), (7, 3), (8, 3), (31, 1), (31, 8))] == [9, 22, 25, 32, 32]
  cfg = small().cfg
  assert Gn.check_lookup_tree(8, 16, 4, 3, (1, 4), cfg) == (8 + 16 + 13, 13) and Gn.check_lookup_tree(8, 16, 7, 3, (1, 4), cfg, 8) == (32, 8)
  lib = _lib.load()
  B, n, nh, hd, T, hidden = 2, 5, 2, 64, 300, 96
  shared = lib.plm_attn_decode_shared_workspace_bytes(B, n, nh, hd, T, 1, 0, 1)  # S_p by the same rule, one suffix partial
  for sp in (0, 3):
    need = lib.plm_attn_extend_tree_workspace_bytes(B, n, nh, hd, T, sp)
    assert need == (shared if sp == 0 else (B * n * nh * 4 * (2 + hd) * 4 + 15) // 16 * 16)
    assert lib.plm_extend_layer_tree_workspace_bytes(B, n, nh, hd, hidden, T, sp) == need + B * n * (2 * nh * hd * 2 + hidden * 2)
  assert lib.plm_extend_layer_tree_workspace_bytes(4, 22, nh, hd, hidden, T, 0) == 0  # B * n > 32
  for bad in ((0, n, nh, hd, T, 0), (B, 0, nh, hd, T, 0), (B, 33, nh, hd, T, 0), (B, n, nh, 48, T, 0), (B, n, nh, hd, 0, 0), (B, n, nh, hd, T, 65)):
    assert lib.plm_attn_extend_tree_workspace_bytes(*bad) == 0, bad
