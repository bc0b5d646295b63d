"""What the six generation methods of Transformer (prefill, decode_step, new_cache, extend, generate, generate_speculative) refuse and
compute on commit dc47b4e, the last one with those methods written out in transformer.py, recorded for
tests/test_generate_trace_host.py and tests/test_generate_trace_gpu.py, which replay this file's functions and demand equality.

generate_trace_parent.json:
  'refusals': {'cpu' | 'cuda': {scenario: [exception type, full text, library calls made]}} - every bad input the methods distinguish
              (and inputs bad in two ways at once, which pin the order of the checks), once with models and tensors on the CPU (every
              scenario is refused there, at the latest for being on the CPU) and once with them on the device.
  'results':  {call: {'entries': the C-ABI entry points in order, 'tokens', 'logprob_bits' (int32 patterns), 'stats'}} for five calls on
              the golden 2-layer model (d 128, 2 heads, V 256, seq_len 64), B = 2, prompt width 16, prompt_lens (16, 9), 6 new tokens,
              n_draft 3, and an eos_id ('eos_id') that one of the two sequences emits early.
  'stable':   {call: were two recordings on fresh models equal as a whole?}

Run on an MI355X from a checkout of commit dc47b4e with its library built:
  python tests/golden/make_generate_trace_parent.py [output .json]
"""
import contextlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import plainlm_amd as P  # noqa: E402
from plainlm_amd import _lib  # noqa: E402
from plainlm_amd.generate import KVCache  # noqa: E402

SMALL = dict(vocab_size=256, seq_len=64, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu')
LENS, N, K = (16, 9), 6, 3


@contextlib.contextmanager
def library_calls():
  """The names _lib.check is handed while the block runs (every launch of the package reports through it), in order."""
  calls, real = [], _lib.check
  _lib.check = lambda rc, what: calls.append(what) or real(rc, what)
  try:
    yield calls
  finally:
    _lib.check = real


def refusal_scenarios(dev):
  """{scenario: (thunk, run with grad enabled?)} on device ``dev``; every thunk raises before anything is launched."""
  model = lambda **kw: P.Transformer(P.ModelConfig(**{**SMALL, **kw})).to(dev)  # noqa: E731
  m, mx, frozen = model(), model(linear_precision='mxfp8'), model().requires_grad_(False)
  other, wide, short = model(n_layers=1, n_heads=4), model(vocab_size=264), model(seq_len=32)
  tok = torch.zeros((2, 16), dtype=torch.int64, device=dev)
  cache, cache1 = KVCache(2, 2, 64, 2, 64, dev), KVCache(1, 2, 64, 4, 32, dev)
  S = {}

  def add(name, thunk, grad=False):
    assert name not in S
    S[name] = (thunk, grad)

  methods = {'prefill': (lambda mm, t: mm.prefill(t), tok), 'decode_step': (lambda mm, t: mm.decode_step(t, cache), tok[:, 0].contiguous()),
             'extend': (lambda mm, t: mm.extend(t, cache), tok[:, :3].contiguous()), 'generate': (lambda mm, t: mm.generate(t, 4), tok),
             'generate_speculative': (lambda mm, t: mm.generate_speculative(t, 4, other, n_draft=K), tok)}
  for name, (call, good) in methods.items():
    for kind, mm, t, grad in (('non-tensor', m, good.tolist(), False), ('dtype', m, good.int(), False), ('cpu', m, good.cpu(), False),
                              ('dtype+cpu', m, good.int().cpu(), False), ('rank', m, good[None], False), ('mxfp8', mx, good, False),
                              ('cpu+mxfp8', mx, good.cpu(), False), ('cpu+grad', m, good.cpu(), True)):
      add(f'{name}/{kind}', lambda call=call, mm=mm, t=t: call(mm, t), grad)
    if name.startswith('generate'):  # the two forward-only methods
      for kind, mm, t in (('grad', m, good), ('non-tensor+grad', m, good.tolist()), ('grad+mxfp8', mx, good)):
        add(f'{name}/{kind}', lambda call=call, mm=mm, t=t: call(mm, t), True)
  add('decode_step/batch', lambda: m.decode_step(tok[:3, 0].new_zeros(3), cache))
  add('extend/batch', lambda: m.extend(tok.new_zeros((3, 3)), cache))
  add('extend/empty-chunk', lambda: m.extend(tok[:, :0], cache))
  add('extend/cache-shape', lambda: m.extend(tok[:, :3], cache1))
  add('extend/token_lens-count', lambda: m.extend(tok[:, :3], cache, token_lens=[1, 2, 3]))
  add('extend/token_lens-values', lambda: m.extend(tok[:, :3], cache, token_lens=[1, 9]))
  add('extend/token_lens-device-dtype', lambda: m.extend(tok[:, :3], cache, token_lens=torch.ones(2, dtype=torch.int64, device=dev)))
  add('prefill/prompt_lens-device', lambda: m.prefill(tok, prompt_lens=torch.tensor(LENS, device=dev)))
  add('prefill/prompt_lens-count', lambda: m.prefill(tok, prompt_lens=[16]))
  add('prefill/prompt_lens-values', lambda: m.prefill(tok, prompt_lens=[16, 17]))
  add('prefill/max_len-small', lambda: m.prefill(tok, max_len=8))
  add('prefill/max_len-large', lambda: m.prefill(tok, max_len=65))
  add('new_cache/B0', lambda: m.new_cache(0))
  add('new_cache/max_len-small', lambda: m.new_cache(2, max_len=0))
  add('new_cache/max_len-large', lambda: m.new_cache(2, max_len=65))
  add('new_cache/mxfp8', lambda: mx.new_cache(2))
  add('new_cache/cpu-model', lambda: P.Transformer(P.ModelConfig(**SMALL)).new_cache(2))
  both = {'generate': lambda *a, **kw: m.generate(*a, **kw), 'generate_speculative': lambda p, n, **kw: m.generate_speculative(p, n, other, **kw)}
  for name, gen in both.items():
    add(f'{name}/max_new_tokens-0', lambda gen=gen: gen(tok, 0))
    add(f'{name}/over-length', lambda gen=gen: gen(tok, 49))
    add(f'{name}/empty-prompt', lambda gen=gen: gen(tok[:, :0], 4))
    add(f'{name}/prompt_lens-device', lambda gen=gen: gen(tok, 4, prompt_lens=torch.tensor(LENS, device=dev)))
    add(f'{name}/temperature0+filter', lambda gen=gen: gen(tok, 4, temperature=0.0, top_k=5))
    add(f'{name}/temperature-negative', lambda gen=gen: gen(tok, 4, temperature=-1.0))
    add(f'{name}/top_p-0', lambda gen=gen: gen(tok, 4, temperature=0.8, top_p=0.0))
    add(f'{name}/top_k-negative', lambda gen=gen: gen(tok, 4, top_k=-1))
  add('generate/sample+temperature', lambda: m.generate(tok, 4, sample=lambda x: x.argmax(-1), temperature=0.8))
  add('generate/sample+seed', lambda: m.generate(tok, 4, sample=lambda x: x.argmax(-1), seed=1))
  spec = lambda draft, n=4, mm=m, **kw: mm.generate_speculative(tok, n, draft, **kw)  # noqa: E731
  add('generate_speculative/draft-type', lambda: spec(None))
  add('generate_speculative/cpu+draft-type', lambda: m.generate_speculative(tok.cpu(), 4, None))
  add('generate_speculative/draft-type+grad', lambda: spec(None), True)
  add('generate_speculative/draft-vocab', lambda: spec(wide))
  add('generate_speculative/draft-mxfp8', lambda: spec(mx))
  add('generate_speculative/draft-grad', lambda: spec(other, mm=frozen), True)
  add('generate_speculative/draft-on-cpu', lambda: spec(P.Transformer(P.ModelConfig(**SMALL))))
  add('generate_speculative/n_draft-float', lambda: spec(other, n_draft=2.0))
  add('generate_speculative/n_draft-bool', lambda: spec(other, n_draft=True))
  add('generate_speculative/n_draft-0', lambda: spec(other, n_draft=0))
  add('generate_speculative/n_draft-32', lambda: spec(other, n_draft=32))
  add('generate_speculative/over-length-target', lambda: spec(other, 44, n_draft=4))  # 16 + 44 + 4 + 1 > 64
  add('generate_speculative/over-length-draft', lambda: spec(short, 14, n_draft=4))  # 16 + 14 + 4 + 1 > 32
  return S


def record_refusals(dev):
  out = {}
  for name, (thunk, grad) in refusal_scenarios(dev).items():
    with library_calls() as calls, torch.set_grad_enabled(grad):
      try:
        thunk()
        out[name] = ['no exception', '', len(calls)]
      except Exception as e:  # noqa: BLE001 - the type is what is recorded
        out[name] = [type(e).__name__, str(e), len(calls)]
  return out


def golden_models():
  """(target, self-draft = the target's weights in another module, a random 1-layer draft with other heads and another MLP class)."""
  z = np.load(os.path.join(HERE, 'model.npz'))
  w = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('w:')}
  pair = [P.Transformer(P.ModelConfig(**SMALL)) for _ in range(2)]
  for m in pair:
    m.load_state_dict(w)
  torch.manual_seed(5)
  other = P.Transformer(P.ModelConfig(**{**SMALL, 'expand': 2.0, 'n_layers': 1, 'n_heads': 4, 'mlp': 'mlp_relu_sq'}))
  return pair[0].cuda(), pair[1].cuda(), other.cuda(), torch.from_numpy(z['tokens'])[:, :16].cuda()


def pick_eos():
  """A token that exactly one of the two sequences emits, before its last position, when decoding greedily without eos_id."""
  m, _, _, prompt = golden_models()
  with torch.no_grad():
    rows = m.generate(prompt, N, prompt_lens=LENS).tolist()
  return next(t for b in (0, 1) for t in rows[b][1:N - 1] if t not in rows[1 - b])


def record_results(eos_id):
  """{call: record} of the five calls, on fresh models (so the first call also casts the weight shadows)."""
  m, twin, other, prompt = golden_models()
  kw = dict(prompt_lens=LENS, eos_id=eos_id, return_logprobs=True)
  skw = dict(n_draft=K, return_stats=True, **kw)
  calls = {'generate:greedy': lambda: m.generate(prompt, N, **kw),
           'generate:sampled': lambda: m.generate(prompt, N, temperature=0.8, top_k=5, seed=1, **kw),
           'speculative:greedy-self-draft': lambda: m.generate_speculative(prompt, N, twin, **skw),
           'speculative:greedy-1-layer-draft': lambda: m.generate_speculative(prompt, N, other, **skw),
           'speculative:sampled': lambda: m.generate_speculative(prompt, N, other, temperature=0.8, top_k=5, seed=1, **skw)}
  out = {}
  for name, call in calls.items():
    with library_calls() as entries, torch.no_grad():
      toks, lps, *stats = call()
    out[name] = dict(entries=list(entries), tokens=toks.tolist(), logprob_bits=lps.contiguous().view(torch.int32).tolist())
    if stats:
      out[name]['stats'] = {k: v.tolist() if isinstance(v, torch.Tensor) else v for k, v in stats[0].items()}
  return out


def main():
  eos_id = pick_eos()
  results, again = record_results(eos_id), record_results(eos_id)
  frozen = [name for name, r in results.items() if any(row[-2:] == [eos_id, eos_id] for row in r['tokens'])]
  assert 'generate:greedy' in frozen
  trace = dict(commit='dc47b4e', eos_id=eos_id, refusals={dev: record_refusals(dev) for dev in ('cpu', 'cuda')}, results=results,
               stable={name: results[name] == again[name] for name in results})
  path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'generate_trace_parent.json')
  with open(path, 'w') as f:
    json.dump(trace, f, indent=1)
  bad = [f'{dev}:{n}' for dev, r in trace['refusals'].items() for n, v in r.items() if v[0] == 'no exception' or v[2]]
  print(f'{path}: {sum(map(len, trace["refusals"].values()))} refusals, not refused cleanly: {bad}; eos_id {eos_id} freezes a sequence in {frozen}; '
        f'stable {trace["stable"]}')


if __name__ == '__main__':
  main()
