"""The device half of tests/test_generate_trace_host.py: on a real MI355X every bad input is refused with the parent's exception and
text before any library call, and the five recorded calls on the golden 2-layer model (greedy and sampled generate; speculative decoding
greedy with the model as its own draft, greedy with a 1-layer draft, sampled) issue the parent's C-ABI entry points in the parent's
order and return its tokens, its log-probabilities bit for bit, and its statistics.  Bit equality is the fair demand: the same kernels
run in the same order on the same operands, and the parent's two recordings were equal (the file's 'stable')."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_generate_trace_host import GEN, PARENT, assert_refusals_equal_the_parent  # noqa: E402


@pytest.fixture(scope='module')
def replayed():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  return GEN.record_results(PARENT['eos_id'])


def test_refusals_on_the_device_equal_the_parent_and_launch_nothing():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  assert_refusals_equal_the_parent('cuda')


@pytest.mark.parametrize('call', sorted(PARENT['results']))
def test_results_equal_the_parent(replayed, call):
  got, want = replayed[call], PARENT['results'][call]
  assert PARENT['stable'][call]  # else only the tokens could be compared
  assert set(got) == set(want)
  for key in ('tokens', 'stats', 'entries', 'logprob_bits'):
    if key in want:
      assert got[key] == want[key], f'{call}: {key} differ'
