"""MXFP8 without a GPU: the CPU reference quantizer (tests/mx_ref.py, which the GPU tests trust) against the scale rule on constructed
blocks, the boundary of the new entry points, and what hipcc made of csrc/mx.hip."""
import ast
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mx_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF = torch.bfloat16


def _block(first, rest=0.0, n=32):
  x = torch.full((1, n), rest, dtype=torch.float64)
  x[0, 0] = first
  return x


def _e(x):
  return int(mx_ref.quantize(x)[1][0, 0]) - 127


def test_scale_rule_at_its_edges():
  # amax = 448 * 2^e exactly: that e, the element is 448 (0x7E); just above it: e + 1
  for e in (-20, -1, 0, 3, 50):
    x = _block(448.0 * 2.0 ** e)
    assert _e(x) == e and int(mx_ref.quantize(x)[0][0, 0]) == 0x7E
    assert _e(_block(448.0 * 2.0 ** e * (1 + 2 ** -7))) == e + 1
  # powers of two: 2^E sits at 256 = 0x78 (2^8 in e4m3: exponent 15, mantissa 0)
  for E in (-100, -8, 0, 1, 7, 100):
    x = _block(2.0 ** E)
    assert _e(x) == E - 8 and int(mx_ref.quantize(x)[0][0, 0]) == 0x78
  # 1.75 * 2^E is the last amax kept at E - 8, the next bf16 up moves to E - 7
  assert _e(_block(1.75)) == -8 and _e(_block(1.7578125)) == -7
  # bf16 subnormals: E below -126, and the clamp of e at -127 (the scale byte never goes below 0)
  assert _e(_block(2.0 ** -118)) == -126 and _e(_block(2.0 ** -119)) == -127 and _e(_block(2.0 ** -120)) == -127
  d, s = mx_ref.quantize(_block(2.0 ** -130, 2.0 ** -133))  # bf16 subnormals: e = -138 clamped to -127
  assert int(s[0, 0]) == 0 and int(d[0, 0]) == 0x20 and int(d[0, 1]) == 0x08  # 2^-3 and 2^-6 after the 2^127 scaling
  assert float(mx_ref.dequantize(d, s)[0, 0]) == 2.0 ** -130


def test_rounding_of_elements():
  # 447.9 -> 448 and 3.3e-3 -> 2^-8 (RNE, subnormals), relative to a block scale of 2^0 (amax 448)
  d, s = mx_ref.quantize(torch.tensor([[448.0, 447.9, 3.3e-3, -3.3e-3, 1e-4, 2.0 ** -10, 3 * 2.0 ** -10] + [0.0] * 25], dtype=torch.float64))
  assert int(s[0, 0]) == 127
  assert d[0, :7].tolist() == [0x7E, 0x7E, 0x02, 0x82, 0x00, 0x00, 0x02]


def test_zero_nonfinite_and_padding_blocks():
  x = torch.zeros(3, 200)
  x[1, 5] = float('nan')
  x[2, 40] = float('inf')
  x[2, 100] = -float('inf')
  x[0, 130] = 1.0
  d, s = mx_ref.quantize(x)
  assert d.shape == (3, 256) and s.shape == (3, 8)
  assert s[0].tolist() == [0, 0, 0, 0, 127 - 8, 0, 0, 0] and d[0, 128:160].tolist() == [0, 0, 0x78] + [0] * 29
  assert int(s[1, 0]) == 0xFF and (d[1, :32] == 0x7F).all() and (s[1, 1:] == 0).all()
  assert int(s[2, 1]) == 0xFF and int(s[2, 3]) == 0xFF and (d[2, 32:64] == 0x7F).all() and (d[2, 96:128] == 0x7F).all()
  assert (d[:, 200:] == 0).all() and (s[:, 7] == 0).all()  # padding: zero elements, scale byte 0
  assert torch.isnan(mx_ref.dequantize(d, s)[1, :32]).all()


def test_transposed_copy_is_the_quantized_transpose_and_round_trip_error():
  g = torch.Generator().manual_seed(0)
  x = (torch.randn(70, 45, generator=g) * 100).to(BF)
  dt, st = mx_ref.quantize(x.t())
  assert dt.shape == (45, 128) and st.shape == (45, 4)
  back = mx_ref.dequantize(dt, st)[:, :70].t()
  rel = (back - x.double()).abs() / x.double().abs().clamp_min(1e-30)
  assert float(rel[x.double().abs() > 1].max()) <= 2.0 ** -4  # 3 mantissa bits, RNE


def test_mx_entry_points_refuse_bad_shapes_without_a_gpu():
  import ctypes as C
  from plainlm_amd import _lib
  lib = _lib.load()
  p = lambda a=0x100000: C.c_void_p(a)
  def refused(name, *args):
    rc = getattr(lib, name)(*args)
    assert rc < 0, (name, rc)
    return (lib.plm_last_error_string() or b'').decode()
  assert 'multiple of 128' in refused('plm_gemm_mx_nt', p(), p(), p(), p(), p(), 64, 64, 64, 100, 0, None)
  assert 'output mode' in refused('plm_gemm_mx_nt', p(), p(), p(), p(), p(), 64, 64, 64, 128, 7, None)
  assert 'aligned' in refused('plm_gemm_mx_nt', p(0x100008), p(), p(), p(), p(), 64, 64, 64, 128, 0, None)
  assert 'cols % 8' in refused('plm_mx_quant', p(), 16, 4, 12, p(), p(), None, None, None)
  assert 'neither output' in refused('plm_mx_quant', p(), 16, 4, 16, None, None, None, None, None)
  assert 'both its data' in refused('plm_mx_quant', p(), 16, 4, 16, p(), None, None, None, None)
  assert 'ld=' in refused('plm_mx_quant', p(), 8, 4, 16, p(), p(), None, None, None)
  items = (_lib.MxQuantItem * 2)(_lib.MxQuantItem(0x100000, 16, 4, 16, 0x100000, 0x100000, 0, 0), _lib.MxQuantItem(0x100000, 16, 4, 16, 0, 0, 0, 0))
  assert 'item 1' in refused('plm_mx_quant_multi', items, 2, None)
  assert lib.plm_version() == 112


@pytest.mark.timeout(600)
def test_isa_of_the_mx_kernels():
  """tools/isa_scan.py mx.hip: no spill or scratch in either kernel; the GEMM runs on the scaled MFMA (never the unscaled fp8 one, which
  only reaches the bf16 rate) and its K loop has no draining vmcnt(0) that is not behind a branch."""
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'isa_scan.py'), 'mx.hip'], capture_output=True, text=True, timeout=560)
  assert r.returncode == 0, r.stderr[-2000:]
  lines = r.stdout.splitlines()
  seen = {}
  for i, l in enumerate(lines):
    if i + 1 < len(lines) and lines[i + 1].strip().startswith("{'vgpr'"):
      seen[l.strip()] = (ast.literal_eval(lines[i + 1].strip()), lines[i + 2] if i + 2 < len(lines) else '')
  assert set(seen) == {'mx_quant_kernel', 'gemm_mx_nt_kernel'}, sorted(seen)
  for name, (meta, _) in seen.items():
    assert meta['vspill'] == 0 and meta['sspill'] == 0 and meta['scratch'] == 0, (name, meta)
  span = seen['gemm_mx_nt_kernel'][1]
  assert 'unconditional vmcnt(0): 0 ' in span and 'vector loads (no LDS-DMA): 0' in span, span
  src = os.path.join(ROOT, 'plainlm_amd', 'csrc', 'mx.hip')
  with __import__('tempfile').TemporaryDirectory() as td:
    subprocess.run(['/opt/rocm/bin/hipcc', '-O3', '-std=c++17', '--offload-arch=gfx950', '-mllvm', '-amdgpu-mfma-vgpr-form=1', '-c', src, '-o',
                    os.path.join(td, 'x.o'), '-save-temps=obj'], cwd=td, check=True, capture_output=True, timeout=500)
    asm = open(os.path.join(td, [f for f in os.listdir(td) if f.endswith('gfx950.s')][0])).read()
  body = asm.split('_Z17gemm_mx_nt_kernel', 1)[1].split('s_endpgm', 1)[0]
  assert body.count('v_mfma_scale_f32_32x32x64_f8f6f4') >= 8
  assert '_fp8_fp8' not in body and '_bf8' not in body


def _cfg(**over):
  from collections import namedtuple
  c = dict(model='transformer', vocab_size=256, d_model=128, expand='8/3', n_layers=2, n_heads=2, mlp_class='glu', seq_len=64,
           tie_embeddings=False)
  c.update(over)
  return namedtuple('Cfg', c.keys())(**c)


def test_linear_precision_config():
  """ModelConfig / construct_model: linear_precision is 'bf16' (default) or 'mxfp8', anything else is refused; the default and an explicit
  'bf16' build identical modules; mxfp8 marks exactly the four linears of every block and leaves state_dict keys and shapes as they are."""
  from plainlm_amd import construct_model
  from plainlm_amd.transformer import HipLinear, ModelConfig, Transformer
  with pytest.raises(ValueError, match='linear_precision'):
    construct_model(_cfg(linear_precision='fp8'))
  with pytest.raises(ValueError, match='linear_precision'):
    Transformer(ModelConfig(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, linear_precision='e4m3'))
  built = {}
  for tag, over in (('default', {}), ('bf16', dict(linear_precision='bf16')), ('mxfp8', dict(linear_precision='mxfp8'))):
    torch.manual_seed(0)
    m, mc = construct_model(_cfg(**over))
    built[tag] = (m, mc)
  assert built['default'][1].linear_precision == 'bf16' and built['mxfp8'][1].linear_precision == 'mxfp8'
  sd = {k: v.shape for k, v in built['default'][0].state_dict().items()}
  for tag in ('bf16', 'mxfp8'):
    other = built[tag][0].state_dict()
    assert {k: v.shape for k, v in other.items()} == sd
    assert all(torch.equal(other[k], v) for k, v in built['default'][0].state_dict().items())
  assert repr(built['default'][0]) == repr(built['bf16'][0])
  for tag, want in (('default', 0), ('bf16', 0), ('mxfp8', 8)):
    m = built[tag][0]
    assert sum(x.mx for x in m.modules() if isinstance(x, HipLinear)) == want
    assert not m.lm_head.mx
