"""Footprint checks: where a launch reads and writes, as opposed to what it computes.

Every buffer of a launch is a view into the middle of a larger allocation (an ``Arena``), and the launch runs twice.  The two runs are
identical except for one fill byte, 0x00 then 0xFF, written into every margin, every output, every workspace and every part of an
in-place buffer that the header says is not read.  0xFF.. is a NaN in bf16, fp32, e4m3 and E8M0 and "may attend" in a mask.  Checks,
all bit equality:

  W    after each run every margin still holds its fill (outputs, in-place buffers, workspaces and inputs alike);
  I    after each run every const operand equals its pre-launch clone;
  C+R  after both runs every extent documented as written is bit-identical between the runs: an element that was never written keeps
       two different fills, a result that took in a margin or uninitialised workspace byte differs (usually as NaN);
  U    extents documented as untouched keep each run's fill.

Index-valued inputs (ids, targets, doc_start, plan words) get margins of two different IN-RANGE values in place of the fill bytes
(``index_margin``), so that an over-read index changes a result but never an address.

Margins: at least GUARD_ROWS rows of the buffer and at least 4096 bytes on each side; a flat buffer counts 16 bytes (one vector
access) as its row.  With ld > cols the pad columns are margin unless a ``written`` / ``untouched`` mask claims them.  Payload bases
are 16-byte aligned; ``misalign=True`` puts a base at 16 bytes past a 128-byte line.  Works on any torch device: the calibration in
tests/test_footprint_host.py runs it on the CPU over Python stand-ins of a kernel.

The tests/test_footprint_*gpu.py files hold the cases, one file per subject: each fills a module-level ``CASES`` dict (id -> (entry
points covered, case function, ...)) and runs its rows through ``run_on_gpu``.  ``L`` / ``P`` / ``call`` reach the library without the
ops wrappers, which allocate exact-size tensors - what these tests must not do."""

import ctypes as C

import pytest
import torch

GUARD_ROWS = 264      # as GUARD of tests/test_gemm_parity_gpu.py: more than one tile of rows
GUARD_BYTES = 4096
FILLS = (0x00, 0xFF)
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
SHOW = 6              # offending positions named in a failure message


def bits(t):
  """Same-size integer view (bit comparison: NaN == NaN, -0 != +0)."""
  if t.dtype == torch.bool:
    return t.view(torch.uint8)
  return t if not t.dtype.is_floating_point else t.view(_INT[t.element_size()])


def fill_value(dtype, fill):
  """The integer whose bytes are all `fill`, in the integer dtype of the same size as `dtype`."""
  size = torch.empty((), dtype=dtype).element_size()
  return 0 if fill == 0 else (0xFF if size == 1 else -1)


class FootprintError(AssertionError):
  """failures: list of (check, buffer name, message); checks: the set of check names that failed."""

  def __init__(self, entry, failures):
    self.entry, self.failures = entry, failures
    self.checks = {c for c, _, _ in failures}
    self.buffers = {b for _, b, _ in failures}
    super().__init__('\n'.join(f'{entry}: {b}: {c}: {m}' for c, b, m in failures))


class Buf:
  """One buffer of a launch inside its allocation.  `t` is the payload view ([rows, cols] with row stride ld, or [n] when flat);
  pass `t` (or ptr / ld) to the launch."""

  def __init__(self, name, role, dtype, rows, cols, ld, flat, device, fill, data, written, untouched, unread, index_margin, misalign,
               run):
    self.name, self.role, self.dtype, self.rows, self.cols, self.ld, self.flat = name, role, dtype, rows, cols, ld, flat
    item = torch.empty((), dtype=dtype).element_size()
    self.idt = _INT[item]
    row_bytes = 16 if flat else ld * item
    mbytes = max(GUARD_ROWS * row_bytes, GUARD_BYTES)
    mbytes = (mbytes + 15) // 16 * 16
    self.front = mbytes // item                       # margin elements on each side
    n_el = 2 * self.front + rows * ld
    raw = torch.empty(n_el * item + 256, dtype=torch.uint8, device=device)
    want = 16 if misalign else 0
    off = (want - (raw.data_ptr() + self.front * item)) % 128
    assert off % 16 == 0, 'allocator returned a base that is not 16-byte aligned'
    self.raw = raw
    self.full = raw[off:off + n_el * item].view(self.idt)        # integer view of margins + payload rows (pad included)
    if index_margin is not None:
      self.margin_value = int(index_margin[run])
    else:
      self.margin_value = fill_value(dtype, fill)
    self.full.fill_(self.margin_value)
    body = self.full[self.front:self.front + rows * ld].view(rows, ld)
    self.body = body                                             # integer view [rows, ld]
    self.t = self.full.view(dtype)[self.front:self.front + rows * ld].view(rows, ld)[:, :cols]
    if flat:
      self.t = self.t.reshape(-1)
    assert self.t.data_ptr() % 16 == 0 and (self.t.data_ptr() % 128 != 0) == bool(misalign)
    # --- extents over [rows, ld]
    payload = torch.zeros(rows, ld, dtype=torch.bool, device=device)
    payload[:, :cols] = True
    as_mask = lambda m: None if m is None else torch.as_tensor(m, dtype=torch.bool).to(device).reshape(rows, -1)  # noqa: E731

    def widen(m):
      m = as_mask(m)
      if m is None or m.shape[1] == ld:
        return m
      w = torch.zeros(rows, ld, dtype=torch.bool, device=device)
      w[:, :m.shape[1]] = m
      return w
    self.untouched = widen(untouched)
    self.unread = widen(unread)
    if role in ('out', 'inout'):
      self.written = widen(written) if written is not None else payload.clone()
      if self.untouched is not None:
        self.written &= ~self.untouched
    else:
      assert written is None and untouched is None and unread is None
      self.written = None
    claimed = payload.clone()
    for m in (self.written, self.untouched):
      if m is not None:
        claimed |= m
    self.pad_margin = ~claimed                                   # pad columns nobody claims: margin
    # --- contents
    if role in ('in', 'inout'):
      assert data is not None, f'{name}: an input needs data'
      self.t.copy_(torch.as_tensor(data).to(device=device, dtype=dtype).reshape(self.t.shape))
      if self.unread is not None:
        body[self.unread] = fill_value(dtype, fill)
    else:
      assert data is None
      body[payload] = fill_value(dtype, fill)
    if self.untouched is not None:
      body[self.untouched] = fill_value(dtype, fill)
    self.fill_int = fill_value(dtype, fill)
    self.before = body.clone() if role == 'in' else None

  @property
  def ptr(self):
    return self.t.data_ptr()

  def _pos(self, flat_idx):
    """First SHOW offending positions of a flat index tensor over `full`, as (row, col) relative to the payload."""
    out = []
    for i in flat_idx[:SHOW].tolist():
      rel = i - self.front
      out.append((0, rel) if self.flat else (rel // self.ld, rel % self.ld))
    return out

  def _body_pos(self, mask):
    idx = mask.reshape(-1).nonzero().reshape(-1) + self.front
    return int(mask.sum()), self._pos(idx)

  def check_run(self, fails):
    f, n = self.front, self.rows * self.ld
    bad = self.full != self.margin_value
    bad[f:f + n] = False
    pad_bad = (self.body != self.margin_value) & self.pad_margin
    bad[f:f + n] |= pad_bad.reshape(-1)
    if bool(bad.any()):
      idx = bad.nonzero().reshape(-1)
      fails.append(('W', self.name, f'{idx.numel()} margin elements changed, first at (row, col) {self._pos(idx)}'))
    if self.role == 'in':
      diff = (self.body != self.before) & ~self.pad_margin
      if bool(diff.any()):
        k, pos = self._body_pos(diff)
        fails.append(('I', self.name, f'{k} elements of a const operand changed, first at (row, col) {pos}'))
    if self.untouched is not None:
      diff = (self.body != self.fill_int) & self.untouched
      if bool(diff.any()):
        k, pos = self._body_pos(diff)
        fails.append(('U', self.name, f'{k} elements of an extent documented as untouched were written, first at (row, col) {pos}'))

  def check_pair(self, other, fails):
    if self.written is None:
      return
    diff = (self.body != other.body) & self.written
    if bool(diff.any()):
      k, pos = self._body_pos(diff)
      fails.append(('C+R', self.name, f'{k} elements differ between the 0x00 and the 0xFF run (never written, or computed from a '
                    f'margin / uninitialised byte), first at (row, col) {pos}'))


class Arena:
  """The buffers of one run of one case."""

  def __init__(self, device, run):
    self.device, self.run, self.fill = device, run, FILLS[run]
    self.bufs = []

  def _add(self, name, role, dtype, rows, cols, ld, flat, **kw):
    b = Buf(name, role, dtype, rows, cols, cols if ld is None else ld, flat, self.device, self.fill, kw.pop('data', None),
            kw.pop('written', None), kw.pop('untouched', None), kw.pop('unread', None), kw.pop('index_margin', None),
            kw.pop('misalign', False), self.run)
    assert not kw, kw
    self.bufs.append(b)
    return b

  # 2-D buffers [rows, cols] with row stride ld; flat buffers [n]
  def inp(self, name, data, ld=None, **kw):
    data = torch.as_tensor(data)
    if data.dim() == 1:
      return self._add(name, 'in', data.dtype, 1, data.numel(), None, True, data=data, **kw)
    data = data.reshape(-1, data.shape[-1])
    return self._add(name, 'in', data.dtype, data.shape[0], data.shape[1], ld, False, data=data, **kw)

  def inout(self, name, data, ld=None, **kw):
    data = torch.as_tensor(data)
    if data.dim() == 1:
      return self._add(name, 'inout', data.dtype, 1, data.numel(), None, True, data=data, **kw)
    data = data.reshape(-1, data.shape[-1])
    return self._add(name, 'inout', data.dtype, data.shape[0], data.shape[1], ld, False, data=data, **kw)

  def out(self, name, dtype, rows, cols=None, ld=None, **kw):
    if cols is None:
      return self._add(name, 'out', dtype, 1, rows, None, True, **kw)
    return self._add(name, 'out', dtype, rows, cols, ld, False, **kw)

  def ws(self, name, nbytes, dtype=torch.uint8):
    item = torch.empty((), dtype=dtype).element_size()
    return self._add(name, 'ws', dtype, 1, max(int(nbytes) // item, 16 // item), None, True)


def run_case(entry, case, device, sync=None):
  """case(arena) declares the buffers of one launch in `arena` and returns a callable that launches.  Runs it under both fills and
  raises FootprintError naming every failed check."""
  fails, arenas = [], []
  for run in range(2):
    ar = Arena(device, run)
    launch = case(ar)
    assert any(b.t.data_ptr() % 128 != 0 for b in ar.bufs), f'{entry}: no buffer off a 128-byte line'
    if sync:
      sync()
    launch()
    if sync:
      sync()
    for b in ar.bufs:
      b.check_run(fails)
    arenas.append(ar)
  for b0, b1 in zip(arenas[0].bufs, arenas[1].bufs):
    assert b0.name == b1.name
    b0.check_pair(b1, fails)
  if fails:
    seen, uniq = set(), []
    for f in fails:                      # the same W / I / U failure in both runs is reported once
      if f not in seen:
        seen.add(f)
        uniq.append(f)
    raise FootprintError(entry, uniq)
  return arenas


# ---- what the GPU case files share
def L():
  from plainlm_amd import _lib
  return _lib.load()


def P(b, offset=0):
  """Device pointer of an arena buffer or of a tensor (plus a byte offset), NULL for None."""
  if b is None:
    return C.c_void_p(0)
  return C.c_void_p((b.ptr if isinstance(b, Buf) else b.data_ptr()) + offset)


def call(name, *args):
  from plainlm_amd import _lib, ops
  _lib.check(getattr(L(), name)(*args, ops._stream()), name)


def run_on_gpu(cid, entries, fn, env=None):
  """run_case on the GPU for one row of a CASES table, under the row's environment switches; returns the two arenas."""
  if not torch.cuda.is_available():
    pytest.skip('no GPU')
  from plainlm_amd import ops
  with pytest.MonkeyPatch.context() as mp:
    for k, v in (env or {}).items():
      mp.setenv(k, v)
    if env:
      ops.reload_env()
    try:
      return run_case(f'{entries[0]} [{cid}]', fn, 'cuda', sync=torch.cuda.synchronize)
    except RuntimeError as e:
      if 'rc=-1' in str(e) or 'rc=-4' in str(e):   # a refused argument: an ordinary failure of this case
        raise
      pytest.exit(f'{cid}: {e}: a launch failed on the device, nothing more is started on it', returncode=3)
    finally:
      if env:
        mp.undo()
        ops.reload_env()
