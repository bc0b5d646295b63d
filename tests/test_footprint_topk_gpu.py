"""Where the launches of the top-k head read and write, on a real MI355X: the footprint cases of plm_head_topk_bf16, its workspace query
and its chunk query.  Same machinery as tests/test_footprint_gpu.py (tests/footprint.py: every buffer between margins, two runs that
differ in one fill byte; W / I / C+R / U are bit equality).  Both row kernels (the row staged in LDS, and a row beyond the LDS budget),
a ragged V (pad columns of the workspace row hold the fill: NaN in the second run), more rows than a chunk, lse / rank / targets null
and non-null.  tests/test_footprint_gpu.py's completeness test counts these rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
CASES = {}      # id -> (entry points covered, case function)
ENTRIES = ('plm_head_topk_bf16', 'plm_head_topk_workspace_bytes', 'plm_head_topk_chunk_rows')


def rnd(seed, *shape, dtype=F32):
  return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def _head_topk_cases():
  for M, V, K, k, path in ((None, 777, 64, 5, 'lds-chunks'), (3, 50280, 64, 64, 'lds'), (3, 65601, 64, 64, 'global'), (3, 65537, 64, 1, 'global')):
    for full in (1, 0):   # every output and the targets; then only what is mandatory (targets / lse / rank null)
      def fn(ar, M=M, V=V, K=K, k=k, path=path, full=full):
        M = int(L().plm_head_topk_chunk_rows()) + 9 if M is None else M
        assert (path == 'global') == ((V + 7) // 8 * 16 > 128 * 1024)  # head_topk.hip's HT_ROW_LDS_BYTES
        nbytes = int(L().plm_head_topk_workspace_bytes(M, V, K, k))
        assert nbytes > 0
        Y = ar.inp('Y', rnd(95, M, K, dtype=BF16), ld=K + 8, misalign=True)
        W = ar.inp('W', rnd(96, V, K, dtype=BF16), ld=K + 8)
        t = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(97))
        t[0], t[1], t[2] = V - 1, -100, V      # the last column, two ignored rows
        targets = ar.inp('targets', t, index_margin=(0, V - 1)) if full else None
        tok = ar.out('tok', I64, M, k)
        logp = ar.out('logp', F32, M, k)
        lse = ar.out('lse', F32, M) if full else None
        rank = ar.out('rank', I32, M) if full else None
        ws = ar.ws('workspace', nbytes)
        return lambda: call('plm_head_topk_bf16', P(Y), K + 8, P(W), K + 8, P(targets), k, P(tok), P(logp), P(lse), P(rank), M, V, K, P(ws), nbytes)
      CASES[f'head_topk-{M or "chunk+9"}x{V}x{K}-k{k}-{path}-{"all" if full else "min"}'] = (ENTRIES, fn)


_head_topk_cases()


@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])
