"""Where the launches of include/plainlm_hip_ext.h read and write, on a real MI355X: the footprint guarantee of
tests/test_footprint_gpu.py for the entry points that file's table cannot list (its completeness test is tied to plainlm_hip.h).
Same machinery (tests/footprint.py: every buffer between margins, two runs that differ in one fill byte; W / I / C+R / U are bit
equality), same shapes and strides as the scoring head's rows there, and a completeness test of its own over the ext header."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64
CASES = {}      # id -> (entry points covered, case function)


@pytest.fixture(scope='module')
def ops():
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops as _ops
  return _ops


def L():
  from plainlm_amd import _lib
  return _lib.load()


def P(b):
  """Device pointer of an arena buffer, NULL for None."""
  return C.c_void_p(0) if b is None else C.c_void_p(b.ptr)


def call(name, *args):
  from plainlm_amd import _lib, ops
  _lib.check(getattr(L(), name)(*args, ops._stream()), name)


def rnd(seed, *shape, dtype=F32):
  return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _head_predict_cases():
  for M, V, K, path in ((520, 264, 64, 'persistent'), (136, 777, 64, '128x128')):
    for full in (1, 0):   # every output and the targets; then only what is mandatory (targets / entropy / nll / lse null)
      def fn(ar, M=M, V=V, K=K, path=path, full=full):
        # the header's condition: shapes plm_gemm_bf16_nt serves with a 128x128 kernel (M < 512, V % 8 != 0) go through that kernel
        assert (path == '128x128') == (M < 512 or V % 8 != 0)
        assert V % 192 != 0 and V % 128 != 0 and M % 128 != 0, 'ragged last tile'
        nbytes = int(L().plm_head_predict_workspace_bytes(M, V, K))
        assert nbytes > 0
        Y = ar.inp('Y', rnd(85, M, K, dtype=BF16), ld=K + 8, misalign=True)
        W = ar.inp('W', rnd(86, V, K, dtype=BF16), ld=K + 8)
        t = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(87))
        t[0], t[1], t[2], t[M - 1] = 0, V - 1, -100, V      # both ends, two ignored rows
        targets = ar.inp('targets', t, index_margin=(0, V - 1)) if full else None
        pred = ar.out('pred', I64, M)
        logp = ar.out('logp', F32, M)
        entropy = ar.out('entropy', F32, M) if full else None
        nll = ar.out('nll', F32, M) if full else None
        lse = ar.out('lse', F32, M) if full else None
        ws = ar.ws('workspace', nbytes)
        return lambda: call('plm_head_predict_bf16', P(Y), K + 8, P(W), K + 8, P(targets), P(pred), P(logp), P(entropy), P(nll), P(lse),
                            M, V, K, P(ws), nbytes)
      CASES[f'head_predict-{M}x{V}x{K}-{path}-{"all" if full else "min"}'] = (('plm_head_predict_bf16', 'plm_head_predict_workspace_bytes'), fn)


_head_predict_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(ops, cid):
  entries, fn = CASES[cid]
  try:
    FP.run_case(f'{entries[0]} [{cid}]', fn, 'cuda', sync=torch.cuda.synchronize)
  except RuntimeError as e:
    if 'rc=-1' in str(e) or 'rc=-4' in str(e):   # a refused argument: an ordinary failure of this case
      raise
    pytest.exit(f'{cid}: {e}: a launch failed on the device, nothing more is started on it', returncode=3)


def test_every_ext_entry_point_is_in_the_table():
  """Every function of include/plainlm_hip_ext.h has a row here (all of them launch, or size what a launch needs)."""
  from plainlm_amd import _lib
  covered = {e for entries, _ in CASES.values() for e in entries}
  want = set(_lib.ext_header_functions())
  assert want - covered == set(), sorted(want - covered)
  assert covered - want == set(), sorted(covered - want)
