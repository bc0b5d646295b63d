"""Transformer's generation methods refuse what they refused before they moved into generate.Generation, with the same exception and
the same text: tests/golden/make_generate_trace_parent.py, run once on the commit before, wrote generate_trace_parent.json; the same
code replays every scenario here with models and tensors on the CPU (tests/test_generate_trace_gpu.py replays the device's scenarios
and the five recorded calls).  On the CPU every scenario is refused, at the latest for being there, so what is compared is which
refusal comes first: the order of the checks."""
import functools
import importlib.util
import inspect
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _load_generator():
  spec = importlib.util.spec_from_file_location('make_generate_trace_parent', os.path.join(GOLDEN, 'make_generate_trace_parent.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


GEN = _load_generator()
with open(os.path.join(GOLDEN, 'generate_trace_parent.json')) as f:
  PARENT = json.load(f)

# Every refusal whose type or text differs from the parent's, as '<device>:<scenario>': one line of reason each.  The same inputs are refused.
ALLOWED = {}


@functools.lru_cache(maxsize=None)
def replayed_refusals(dev):
  return GEN.record_refusals(dev)


def assert_refusals_equal_the_parent(dev):
  got, want = replayed_refusals(dev), PARENT['refusals'][dev]
  assert set(got) == set(want)
  for name in want:
    assert want[name][0] != 'no exception' and got[name][0] != 'no exception', name
    assert got[name][2] == 0 and want[name][2] == 0, f'{name}: a library call before the refusal'
    if f'{dev}:{name}' in ALLOWED:
      assert got[name] != want[name], f'{dev}:{name} is listed in ALLOWED but equals the parent'
      continue
    assert got[name] == want[name], f'{dev}:{name}'


def test_refusals_on_the_cpu_equal_the_parent():
  assert_refusals_equal_the_parent('cpu')
  assert all(name in PARENT['refusals'][dev] for dev, name in (k.split(':', 1) for k in ALLOWED))


def test_the_recording_sees_what_it_is_there_for():
  """Guards the recording against going blind: the facts the scenarios were chosen to show are in the parent's file."""
  cpu, dev = PARENT['refusals']['cpu'], PARENT['refusals']['cuda']
  assert set(cpu) == set(dev) and len(dev) > 90
  assert {v[0] for v in dev.values()} == {'TypeError', 'ValueError', 'RuntimeError', 'NotImplementedError'}
  assert {n.split('/')[0] for n in dev} == {'prefill', 'decode_step', 'new_cache', 'extend', 'generate', 'generate_speculative'}
  assert len({v[1] for v in dev.values()}) > 45  # that many distinct messages
  # the order of the checks differs between the methods, and the doubly bad inputs show it
  assert dev['prefill/cpu+mxfp8'][0] == 'NotImplementedError' and dev['generate/cpu+mxfp8'][0] == 'RuntimeError'
  assert dev['prefill/dtype+cpu'][0] == 'TypeError' and dev['generate/dtype+cpu'][0] == 'RuntimeError'
  assert 'forward-only' in dev['generate/grad+mxfp8'][1] and 'forward-only' in dev['generate/non-tensor+grad'][1]
  assert 'inputs are on CPU' in dev['generate_speculative/cpu+draft-type'][1] and dev['generate_speculative/draft-type+grad'][0] == 'TypeError'
  assert 'forward-only' in dev['generate_speculative/draft-grad'][1]  # the draft alone is trainable
  assert "the target's" in dev['generate_speculative/over-length-target'][1] and "the draft's" in dev['generate_speculative/over-length-draft'][1]
  assert all('inputs are on CPU' in cpu[n][1] for n in cpu if n.startswith('generate/') and n not in ('generate/non-tensor', 'generate/non-tensor+grad'))
  # the five calls: bit-stable on the parent, one sequence frozen by eos_id, a fully accepted round and a rollback
  res, eos = PARENT['results'], PARENT['eos_id']
  assert len(res) == 5 and all(PARENT['stable'].values())
  assert res['generate:greedy']['tokens'][0][-2:] == [eos, eos] and eos not in res['generate:greedy']['tokens'][1]
  assert res['speculative:greedy-self-draft']['stats']['accepted'] == res['speculative:greedy-self-draft']['stats']['drafted']
  rollback = res['speculative:greedy-1-layer-draft']['stats']
  assert sum(rollback['accepted']) < sum(rollback['drafted']) and rollback['rounds'] == 5
  assert 'plm_spec_verify_bf16' in res['speculative:sampled']['entries'] and 'plm_sample_logits_bf16' in res['generate:sampled']['entries']


def test_generation_lives_in_generate_py():
  import plainlm_amd.generate as G
  import plainlm_amd.transformer as T
  for name in ('prefill', 'decode_step', 'new_cache', 'extend', 'generate', 'generate_speculative'):
    assert name not in vars(T.Transformer) and inspect.unwrap(getattr(G.Generation, name)).__module__ == G.__name__, name
  assert issubclass(T.Transformer, G.Generation) and not hasattr(G, 'transformer')
  src = inspect.getsource(G)
  assert 'import transformer' not in src and 'from .transformer' not in src
  body = inspect.getsource(G.Generation.generate_speculative).split('"""')[2]
  assert 'def ' not in body and 'lambda' not in body  # the round's state is _SpecSession's, not captured variables
