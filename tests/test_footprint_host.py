"""Proof that the footprint checks bite (tests/footprint.py, on the CPU): the two-fill runner over a small Python stand-in of a
kernel, written against the arena's views.  The honest stand-in passes every check; each planted defect fails exactly the check meant
for it, on the buffer it touches, and the message names the position.

The stand-in ("gather, column sum, transposed shadow"):
  ids int64 [M] (index-valued), x fp32 [V, d] (ld d + 8), ws 16 fp32 words of workspace ->
  out fp32 [M, d] (ld d + 8, pad = margin) = x[ids]; colsum fp32 [d] = sum of the rows of x;
  out_t fp32 [d, ld_t] = out^T in columns 0..M-1, columns M..ld_t documented as untouched."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402

M, V, D, LD_T = 10, 7, 12, 16


def rows_past(buf, extra):
  """The payload's rows plus `extra` rows of what lies behind it: what a kernel with a wrong row bound addresses."""
  t = buf.t if buf.t.dim() == 2 else buf.t.reshape(1, -1)
  if buf.flat:
    return t.as_strided((t.shape[1] + extra,), (1,), t.storage_offset())
  return t.as_strided((buf.rows + extra, buf.ld), (buf.ld, 1), t.storage_offset())


def standin(defect=None, zero_data=False):
  def case(ar):
    g = torch.Generator().manual_seed(3)
    xdata = torch.zeros(V, D) if zero_data else torch.randint(-8, 9, (V, D), generator=g).float()
    idata = torch.randint(0, V, (M,), generator=g)
    idata[0], idata[-1] = 0, V - 1
    ids = ar.inp('ids', idata, index_margin=(0, V - 1))
    x = ar.inp('x', xdata, ld=D + 8, misalign=True)
    ws = ar.ws('ws', 64, dtype=torch.float32)
    out = ar.out('out', torch.float32, M, D, ld=D + 8)
    colsum = ar.out('colsum', torch.float32, D)
    pad = torch.zeros(D, LD_T, dtype=torch.bool)
    pad[:, M:] = True
    out_t = ar.out('out_t', torch.float32, D, LD_T, untouched=pad)

    def launch():
      idx = ids.t.clone()
      if defect == 'index_overread':          # the last row takes the id one past the end of ids
        idx[M - 1] = rows_past(ids, 1)[M]
      res = x.t[idx]
      if defect == 'ws_word':                 # a result that adds one word of workspace
        res[0, 0] += ws.t[3]
      n = {'last_row_unwritten': M - 1, 'last_4_rows_unwritten': M - 4}.get(defect, M)
      out.t[:n] = res[:n]
      out_t.t[:, :M] = x.t[ids.t].t()
      if defect == 'masked_tail':             # rows V.. of a 4-row tile are "masked" by a weight of 0
        w = torch.zeros(V + 1, 1)
        w[:V] = 1
        colsum.t[:] = (rows_past(x, 1)[:, :D] * w).sum(0)
      else:
        colsum.t[:] = x.t.sum(0)
      if defect == 'store_past_last_row':
        rows_past(out, 1)[M, 0] = 1.0
      if defect == 'store16_across_row_end':  # 4 floats from column D - 2 of the last row: two of them are pad
        rows_past(out, 0)[M - 1, D - 2:D + 2] = torch.cat([res[M - 1, D - 2:], torch.zeros(2)])
      if defect == 'input_modified':
        x.t[1, 2] += 1
      if defect == 'untouched_written':
        out_t.t.as_strided((D, LD_T), (LD_T, 1), out_t.t.storage_offset())[:, M] = 0.0
    return launch
  return case


def test_honest_standin_is_clean():
  arenas = FP.run_case('standin', standin(), 'cpu')
  out = arenas[0].bufs[3]
  assert out.name == 'out' and out.t.data_ptr() % 16 == 0
  assert torch.equal(out.t, arenas[0].bufs[1].t[arenas[0].bufs[0].t])        # and it computes what it says
  assert FP.run_case('standin', standin(zero_data=True), 'cpu')


# defect -> (the one check that must fail, the buffer, a position the message must name)
DEFECTS = {
  'store_past_last_row': ('W', 'out', f'({M}, 0)'),
  'store16_across_row_end': ('W', 'out', f'({M - 1}, {D})'),
  'last_row_unwritten': ('C+R', 'out', f'({M - 1}, 0)'),
  'last_4_rows_unwritten': ('C+R', 'out', f'({M - 4}, 0)'),
  'masked_tail': ('C+R', 'colsum', '(0, 0)'),
  'index_overread': ('C+R', 'out', f'({M - 1}, '),
  'input_modified': ('I', 'x', '(1, 2)'),
  'ws_word': ('C+R', 'out', '(0, 0)'),
  'untouched_written': ('U', 'out_t', f'(0, {M})'),
}


@pytest.mark.parametrize('defect', sorted(DEFECTS))
def test_planted_defect_fails_its_own_check(defect):
  check, buf, pos = DEFECTS[defect]
  with pytest.raises(FP.FootprintError) as e:
    FP.run_case('standin', standin(defect), 'cpu')
  failed = {(c, b) for c, b, _ in e.value.failures}
  assert failed == {(check, buf)}, str(e.value)
  msg = [m for c, b, m in e.value.failures if (c, b) == (check, buf)][0]
  assert pos in msg, msg
  assert 'standin' in str(e.value) and buf in str(e.value) and f': {check}: ' in str(e.value)


def test_front_margin_is_reported_with_negative_rows():
  def case(ar):
    x = ar.inp('x', torch.ones(4, 8), misalign=True)
    out = ar.out('out', torch.float32, 4, 8)

    def launch():
      out.t.copy_(x.t)
      out.t.as_strided((1, 8), (8, 1), out.t.storage_offset() - 8)[0, 5] = 2.0   # row -1
    return launch
  with pytest.raises(FP.FootprintError) as e:
    FP.run_case('standin', case, 'cpu')
  assert e.value.checks == {'W'} and '(-1, 5)' in str(e.value)


@pytest.mark.parametrize('defect', ['last_row_unwritten', 'untouched_written'])
def test_a_result_equal_to_a_fill_is_still_caught(defect):
  """x = 0: every correct output is +0.0, the bits of the 0x00 fill.  The 0xFF run catches the unwritten row (and the zero written
  into the untouched column)."""
  check, buf, _ = DEFECTS[defect]
  with pytest.raises(FP.FootprintError) as e:
    FP.run_case('standin', standin(defect, zero_data=True), 'cpu')
  assert {(c, b) for c, b, _ in e.value.failures} == {(check, buf)}


def test_index_margins_stay_in_range():
  """The margins of an index-valued input hold two different values of the payload's range, never the fill bytes: the over-read id
  of 'index_overread' selects another row of x (the runs differ) and no address outside x."""
  seen = []
  for run in range(2):
    ar = FP.Arena('cpu', run)
    standin('index_overread')(ar)
    ids = ar.bufs[0]
    assert ids.full.min() >= 0 and ids.full.max() < V
    seen.append(int(ids.full[0]))
    assert int(ids.full[0]) == int(ids.full[-1]) == int(rows_past(ids, 1)[M])
  assert seen[0] != seen[1]


def test_layout_rules():
  ar = FP.Arena('cpu', 1)
  a = ar.out('a', torch.bfloat16, 5, 40, ld=48)
  b = ar.out('b', torch.float32, 3, misalign=True)
  c = ar.inp('mask', torch.ones(4, 4, dtype=torch.bool))
  for buf in (a, b, c):
    item = buf.full.element_size()
    assert buf.front * item >= FP.GUARD_BYTES and buf.t.data_ptr() % 16 == 0
  assert a.front >= FP.GUARD_ROWS * 48 and a.t.stride(0) == 48 and tuple(a.t.shape) == (5, 40)
  assert a.t.data_ptr() % 128 == 0 and b.t.data_ptr() % 128 == 16
  assert torch.isnan(a.t.float()).all() and torch.isnan(b.t).all()      # 0xFF.. is a NaN in bf16 and fp32
  assert bool(c.t.all()) and int(c.full[0]) == 0xFF                     # and "may attend" in a mask byte
