"""The block-linear autograd Functions (functional.LinearFn, QKVRopeFn, MLPFn and GradSink's weight-gradient queue) make the ops calls of
the commit before the bf16 / mxfp8 pairs became one family: tests/golden/make_functional_trace_parent.py, run once on that commit, wrote
functional_trace_parent.json; the same code replays every scenario here, on CPU tensors against recording fakes, and the two traces
must be equal as a whole - the calls and their order, every operand's dtype, shape and strides, every scalar and keyword, what each
forward saves and keeps alive, the gradients handed to autograd, and the order and contents of the sink's queue and flushes."""
import functools
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _load_generator():
  spec = importlib.util.spec_from_file_location('make_functional_trace_parent', os.path.join(GOLDEN, 'make_functional_trace_parent.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


GEN = _load_generator()
with open(os.path.join(GOLDEN, 'functional_trace_parent.json')) as f:
  PARENT = json.load(f)['scenarios']


@functools.lru_cache(maxsize=None)
def replayed():
  return GEN.record_all()


def test_every_scenario_is_recorded_and_replayed():
  want = {f'{p}-{m}-{s}-{g}' for p in GEN.PRECISIONS for m in GEN.MODULES for s in ('autograd', 'sink') for g in GEN.GRAD_PATTERNS}
  want |= {'sink-five-linears-groups-of-three', 'sink-one-mx-two-bf16', 'sink-single-bf16', 'sink-grouping-refused', 'sink-two-passes-one-window'}
  assert set(PARENT) == want
  assert set(replayed()) == want


@pytest.mark.parametrize('name', sorted(PARENT))
def test_trace_equals_the_parent(name):
  got, want = replayed()[name], PARENT[name]
  assert got['modules'] == want['modules']  # class names, state_dict keys and shapes, hidden_dim, kind
  assert len(got['passes']) == len(want['passes'])
  for i, (g, w) in enumerate(zip(got['passes'], want['passes'])):
    for key in ('ops', 'saved', 'alive', 'grads'):
      assert g[key] == w[key], f'{name}, pass {i}: {key} differ'
  assert got == want


def test_the_recording_sees_what_it_is_there_for():
  """Guards the recording itself against going blind: the facts the scenarios were chosen to show are in the parent's file."""
  def names(scenario, i):
    return [e[0] for e in PARENT[scenario]['passes'][i]['ops']]
  # the fused epilogues of bf16 GLU; the lazy casts appear in the first pass, not in the second, and again after invalidate()
  assert names('bf16-glu-autograd-all', 0) == ['cast_bf16_t'] * 2 + ['fc1_swiglu', 'gemm_nt', 'fc2_dx_swiglu_bwd', 'gemm_tn', 'gemm_nt', 'gemm_tn']
  assert names('bf16-glu-autograd-all', 1) == names('bf16-glu-autograd-all', 0)[2:]
  assert names('bf16-glu-autograd-all', 2) == names('bf16-glu-autograd-all', 0)
  assert names('mxfp8-glu-autograd-all', 1).count('mx_quant') == 4 and names('mxfp8-glu-autograd-all', 0).count('mx_quant') == 6
  # skipped calls: no dX GEMM without a gradient for x, no dW GEMM without one for the weights
  assert names('bf16-linear-autograd-no_x', 1) == ['gemm_nt', 'gemm_tn'] and names('bf16-linear-autograd-no_w', 1) == ['gemm_nt', 'gemm_nt']
  # kept alive by the MX MLP: u through save_for_backward; of the two quantized inputs only the copies blocked along the tokens (.1)
  p = PARENT['mxfp8-glu-autograd-all']['passes'][1]
  assert p['saved'] == ['bfloat16[24, 256]s[256, 1]']
  assert p['alive'] == ['0:mx_quant.1', '1:gemm_mx_nt.0', '3:mx_quant.1', '4:gemm_mx_nt.0']
  # the sink: a flush in mid-queue; MX items first, then one grouped launch; a single bf16 item goes to gemm_tn; a refusal to gemm_tn each
  flushes = [e[2] for e in PARENT['sink-five-linears-groups-of-three']['passes'][0]['ops'] if e[0] == 'flush']
  assert [len(f) for f in flushes] == [3, 2]
  assert names('sink-one-mx-two-bf16', 0)[-3:] == ['flush', 'gemm_mx_nt', 'gemm_tn_grouped']
  assert names('sink-single-bf16', 0)[-2:] == ['flush', 'gemm_tn']
  assert names('sink-grouping-refused', 0)[-5:] == ['flush', 'gemm_tn_grouped', 'gemm_tn', 'gemm_tn', 'gemm_tn']
  assert [a for e in PARENT['sink-two-passes-one-window']['passes'][1]['ops'] if e[0] == 'flush' for _, a in e[2]] == [True, True]
