"""Beam search without a GPU: every refusal of generate_beam / fork_beam comes before anything is launched."""

import pytest
import torch

from plainlm_amd import _lib, generate as Gn

from test_shared_host import prefix, small


@pytest.mark.parametrize('bad,exc,match', [
    (dict(num_beams=0), ValueError, r'num_beams must be in \[1, 32\]'), (dict(num_beams=33), ValueError, r'num_beams must be in \[1, 32\]'),
    (dict(num_beams=True), TypeError, 'num_beams must be an int'), (dict(num_return=3), ValueError, 'num_return must be in'),
    (dict(num_return=0), ValueError, 'num_return must be in'), (dict(num_beams=32, num_return=1, vocab=56), ValueError, 'too small for 32 beams'),
    (dict(temperature=1.0), ValueError, 'no sampling arguments'), (dict(top_k=5), ValueError, 'no sampling arguments'),
    (dict(top_p=0.9), ValueError, 'no sampling arguments'), (dict(seed=1), ValueError, 'no sampling arguments'),
    (dict(sample=lambda x: x), ValueError, 'no sampling arguments'), (dict(num_beams=17, num_return=1, fused=True), ValueError, 'leave fused off'),
    (dict(max_new_tokens=0), ValueError, 'max_new_tokens'), (dict(max_new_tokens=60), ValueError, 'exceeds'),
    (dict(length_penalty=float('inf')), ValueError, 'length_penalty'), (dict(eos_id=64), ValueError, 'eos_id'),
    (dict(mx=True), ValueError, 'mxfp8 has no shared-prefix')])
def test_generate_beam_refuses_before_the_prefill(monkeypatch, bad, exc, match):
  bad = dict(bad)
  m = small(linear_precision='mxfp8', dim=128) if bad.pop('mx', False) else small(vocab_size=bad.pop('vocab', 64))
  monkeypatch.setattr(m, 'prefill', lambda *a, **k: pytest.fail('prefill ran'))
  monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('a refusal reached the library'))
  monkeypatch.setattr(Gn, 'refuse_cpu', lambda t: None)  # host tensors stand in for device ones
  kw = dict(max_new_tokens=4, num_beams=2, num_return=2)
  kw.update(bad)
  with pytest.raises(exc, match=match), torch.no_grad():
    m.generate_beam(torch.zeros(2, 8, dtype=torch.int64), kw.pop('max_new_tokens'), kw.pop('num_beams'), **kw)


def test_beam_state_refusals_and_books(monkeypatch):
  monkeypatch.setattr(_lib, 'load', lambda: pytest.fail('a refusal reached the library'))
  monkeypatch.setattr(Gn, 'refuse_cpu', lambda t: None)
  m = small()
  with pytest.raises(ValueError, match="'fp8' cache cannot be shared"):
    m.fork_beam(prefix(kv_dtype='fp8'), 2, 4)
  with pytest.raises(ValueError, match='num_beams'):
    m.fork_beam(prefix(), 33, 4)
  with pytest.raises(ValueError, match='mxfp8 has no shared-prefix'):
    small(linear_precision='mxfp8', dim=128).fork_beam(prefix(), 2, 4)
  st = m.fork_beam(prefix(), 3, 7)
  b = st.beam
  assert isinstance(st, Gn.SharedPrefixCache) and (b.P, b.G, b.N, b.steps) == (2, 3, 7, 0)
  assert tuple(b.anc.shape) == (6, 7) and b.anc.dtype == torch.uint8 and tuple(b.tok_hist.shape) == (2, 7, 3)
  b.steps = 1  # the table the last advance wrote is the other half of the pair
  assert b.anc.data_ptr() == b._anc[1].data_ptr()
  assert m.fork(prefix(), 3, 7).beam is None
  tok = torch.zeros(6, 2, dtype=torch.int64)
  for call in (lambda: m.extend(tok, st), lambda: m.extend(tok, st, fused=True),
               lambda: m.extend_tree(tok, torch.zeros(6, 2, dtype=torch.int32), st)):
    with pytest.raises(TypeError, match='decode steps only'):  # no chunks, hence no speculative or lookup rounds, on a beam state
      call()
  with pytest.raises(TypeError, match='already a fork'):
    m.fork_beam(st, 2, 4)
  with pytest.raises(ValueError, match='leave fused off'):  # P * G = 2 * 17 rows
    m.decode_step(torch.zeros(34, dtype=torch.int64), m.fork_beam(prefix(), 17, 4), fused=True)
