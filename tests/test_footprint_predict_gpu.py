"""Where the launches of the prediction head read and write, on a real MI355X: the footprint cases of plm_head_predict_bf16 and its
workspace query.  Same machinery as tests/test_footprint_gpu.py (tests/footprint.py: every buffer between margins, two runs that differ
in one fill byte; W / I / C+R / U are bit equality), same shapes and strides as the scoring head's rows there.  That file's completeness
test counts these rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, I64 = torch.bfloat16, torch.float32, torch.int64
CASES = {}      # id -> (entry points covered, case function)


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
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
