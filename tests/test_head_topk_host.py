"""CPU tests (no GPU) of the top-k head: the reference of tests/topk_ref.py on hand-built rows, and the refusals of the entry point and
of the Python layers, all before any HIP call."""

import ctypes as C
import os
import sys

import pytest
import torch

import plainlm_amd as P
from plainlm_amd import _lib, engine, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as R  # noqa: E402

INF, NAN = float('inf'), float('nan')
ROWS = {  # name -> (row, target, k, tok, rank)
  'tie straddles the k-th place': ([1., 3., 2., 3., 2., 2.], 5, 3, [1, 3, 2], 4),
  'fewer than k finite': ([NAN, 0.5, -INF, INF, -1.], 4, 3, [1, 4, -1], 1),
  'all equal': ([2., 2., 2., 2.], 3, 2, [0, 1], 3),
  'all NaN': ([NAN, NAN, NAN], 1, 2, [-1, -1], 3),
  'ignored target': ([0., 1., -0., 5.], -100, 3, [3, 1, 0], -1),
  'non-finite target': ([0., INF, 2.], 1, 1, [2], 3),
}


@pytest.mark.parametrize('name', list(ROWS))
def test_reference_on_hand_built_rows(name):
  row, tg, k, tok, rank = ROWS[name]
  x = torch.tensor([row])
  r = R.topk_reference(x, k, torch.tensor([tg]))
  assert r['tok'][0].tolist() == tok and r['rank'].tolist() == [rank] and r['rank'].dtype == torch.int32
  fin = [v for v in row if abs(v) < INF]  # (NaN fails the comparison)
  lse = torch.logsumexp(torch.tensor(fin, dtype=torch.float64), 0).item() if fin else -INF
  assert r['lse'][0].item() == pytest.approx(lse, abs=1e-12) or (not fin and r['lse'][0].item() == -INF)
  want = [row[t] - lse if t >= 0 else -INF for t in tok]
  assert r['logp'][0].tolist() == pytest.approx(want, abs=1e-12)
  assert R.kth_place_ties(x, k).tolist() == [name in ('tie straddles the k-th place', 'all equal', 'ignored target')]  # (the last: +0 == -0)


def _lib_loaded():
  if not os.path.exists(_lib.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _lib.load()


def test_entry_point_refuses_bad_arguments_without_a_gpu():
  lib = _lib_loaded()
  assert _lib.EXPECTED_ABI == 112 == lib.plm_version()  # additive: the number did not move
  p = lambda: C.c_void_p(0x100000)  # plausible, never dereferenced
  big = 1 << 40
  good = dict(Y=p(), ldy=768, W=p(), ldw=768, targets=p(), k=5, tok=p(), logp=p(), lse=None, rank=None, M=512, V=1024, K=768, ws=p(), n=big, s=None)
  for change, word in ((dict(Y=None), 'null pointer'), (dict(tok=None), 'null pointer'), (dict(logp=None), 'null pointer'), (dict(ws=None), 'null pointer'),
                       (dict(targets=None, rank=p()), 'rank needs targets'), (dict(k=0), 'k=0'), (dict(k=65), 'k=65'), (dict(k=9, V=8), 'k=9'),
                       (dict(K=776, ldy=776, ldw=776), 'K % 64'), (dict(ldy=772), 'multiples of 8'), (dict(ldw=760), 'multiples of 8'),
                       (dict(W=C.c_void_p(0x100002)), 'aligned'), (dict(rank=C.c_void_p(0x100002)), 'aligned'),
                       (dict(n=lib.plm_head_topk_workspace_bytes(512, 1024, 768, 5) - 1), 'workspace')):
    rc = lib.plm_head_topk_bf16(*{**good, **change}.values())
    msg = (lib.plm_last_error_string() or b'').decode()
    assert rc == (-4 if word == 'workspace' else -1) and 'plm_head_topk_bf16' in msg and word in msg, (change, rc, msg)
  chunk = lib.plm_head_topk_chunk_rows()
  assert chunk == ops.head_topk_chunk_rows() and chunk in (256, 512, 1024)
  ld = 50280 * 2
  assert lib.plm_head_topk_workspace_bytes(3, 50280, 768, 5) == (3 * ld + 255) // 256 * 256
  assert lib.plm_head_topk_workspace_bytes(1 << 20, 50280, 768, 64) == chunk * ld  # the chunk of logits, nothing else
  assert lib.plm_head_topk_workspace_bytes(8, 50280, 768, 65) == 0 == lib.plm_head_topk_workspace_bytes(8, 4, 64, 5)


def test_python_layers_validate_and_have_no_cpu_path():
  y, w = torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(16, 64, dtype=torch.bfloat16)
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.head_topk(y, w, 5)
  with pytest.raises(RuntimeError, match='no CPU path'):
    ops.head_topk(y, w, 5, torch.zeros(8, dtype=torch.int64))
  for k in (0, 65, 2.0):
    with pytest.raises(ValueError, match='k='):
      ops.head_topk(y, w, k)
  assert ops.HeadTopKOut._fields == ('tok', 'logp', 'lse', 'rank') and P.HeadTopK._fields == ('tokens', 'logprobs', 'lse', 'rank')
  assert 'HeadTopK' in P.__all__ and callable(engine.HipEngine.eval_topk)
  model = P.Transformer(P.ModelConfig(vocab_size=512, seq_len=128, dim=128, expand=8 / 3, n_layers=2, n_heads=2, mlp='glu'))
  ids = torch.zeros(1, 128, dtype=torch.int64)
  with pytest.raises(RuntimeError, match='MI355X'):
    model.predict_topk(ids, 5)
  with torch.no_grad(), pytest.raises(RuntimeError, match='MI355X'):
    model.predict_topk(ids, 5, targets=ids, last_only=True)
