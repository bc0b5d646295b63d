"""Host-side logic of the dense attention mask mode: the `attn_mask_mode` model setting, DenseMask's argument checks (before anything touches
the GPU) and the register budget of csrc/attn_masked.hip's kernels."""

import ast
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
  c = dict(model='transformer', vocab_size=256, d_model=64, expand='8/3', n_layers=1, n_heads=1, mlp_class='glu', seq_len=32,
           tie_embeddings=False)
  c.update(kw)
  return SimpleNamespace(**c)


def test_construct_model_reads_attn_mask_mode():
  from plainlm_amd import construct_model
  model, mcfg = construct_model(_cfg())
  assert mcfg.attn_mask_mode == 'doc' and model.cfg.attn_mask_mode == 'doc'  # the reference's configs have no such key
  model, mcfg = construct_model(_cfg(attn_mask_mode='dense'))
  assert mcfg.attn_mask_mode == 'dense' and model.cfg.attn_mask_mode == 'dense'
  model, mcfg = construct_model(_cfg(attn_mask_mode='doc'))
  assert mcfg.attn_mask_mode == 'doc'
  for bad in ('sparse', 'Dense', None, 1):
    with pytest.raises(ValueError, match='attn_mask_mode'):
      construct_model(_cfg(attn_mask_mode=bad))


def test_model_config_refuses_an_unknown_attn_mask_mode():
  from plainlm_amd import ModelConfig, Transformer
  with pytest.raises(ValueError, match='attn_mask_mode'):
    Transformer(ModelConfig(vocab_size=256, seq_len=32, dim=64, expand=8 / 3, n_layers=1, n_heads=1, mlp='glu', attn_mask_mode='bool'))


@pytest.mark.parametrize('mask,err', [
  (torch.ones(2, 8, 8, dtype=torch.int32), TypeError),
  (torch.ones(2, 8, 8, dtype=torch.uint8), TypeError),
  (torch.ones(2, 8, 8, dtype=torch.float32), TypeError),
  ([[True]], TypeError),
  (torch.ones(2, 8, 12, dtype=torch.bool), ValueError),
  (torch.ones(8, dtype=torch.bool), ValueError),
  (torch.ones(1, 2, 8, 8, dtype=torch.bool), ValueError),
  (torch.ones(2, 0, 0, dtype=torch.bool), ValueError),
  (torch.ones(2, 6, 6, dtype=torch.bool), ValueError),  # T must be a multiple of 4
])
def test_dense_mask_refuses_bad_shapes_and_dtypes(mask, err):
  from plainlm_amd.functional import DenseMask
  with pytest.raises(err):
    DenseMask(mask, 2)


def test_dense_mask_has_no_cpu_path():
  from plainlm_amd.functional import DenseMask
  with pytest.raises(RuntimeError, match='GPU'):
    DenseMask(torch.ones(2, 8, 8, dtype=torch.bool), 2)


@pytest.mark.timeout(600)
def test_register_budget_of_the_masked_attention_kernels():
  """tools/isa_scan.py on csrc/attn_masked.hip: no VGPR / SGPR spill and no scratch in the pack kernel or any of the nine masked attention
  kernels (head dims 32, 64, 128 x forward, dQ, dK/dV)."""
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'isa_scan.py'), 'attn_masked.hip'], capture_output=True, text=True, timeout=560)
  assert r.returncode == 0, r.stderr[-2000:]
  lines = r.stdout.splitlines()
  seen = {}
  for i, l in enumerate(lines):
    if i + 1 < len(lines) and lines[i + 1].strip().startswith("{'vgpr'"):
      seen[l.strip()] = ast.literal_eval(lines[i + 1].strip())
  names = [n for n in seen if 'masked' in n or 'mask_pack' in n]
  assert len(names) == 10, sorted(seen)
  for n in names:
    meta = seen[n]
    assert meta['vspill'] == 0 and meta['sspill'] == 0 and meta['scratch'] == 0, (n, meta)
