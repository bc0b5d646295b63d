"""Where every launch of the C ABI reads and writes, on a real MI355X (tests/footprint.py: every buffer between margins, two runs that differ
in one fill byte; W / I / C+R / U are bit equality).  One table row per case, at the smallest ragged shapes at which an edge exists; each
case asserts the path it takes before it launches.  The calls go through _lib.load() and ops._p / ops._stream(): the ops wrappers
allocate exact-size tensors, which is what these tests must not do.  Values are checked elsewhere (the parity files); tests/
test_footprint_host.py shows on the CPU that each check fails for the defect it is meant for.  profiles/footprint.md has the outcome
per entry point.  Not here: plm_comm_* (several ranks), the two probes (already exact)."""
import ctypes as C
import functools
import glob
import importlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint as FP  # noqa: E402
from footprint import L, P, call  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8
CASES = {}      # id -> (entry points covered, case function, environment switches)


def case(cid, entries, env=None):
  def deco(fn):
    assert cid not in CASES, cid
    CASES[cid] = (tuple(entries.split()), fn, env or {})
    return fn
  return deco


def gen(seed):
  return torch.Generator().manual_seed(seed)


def rnd(seed, *shape, dtype=F32, scale=1.0):
  return (torch.randn(*shape, generator=gen(seed)) * scale).to(dtype)


def ints(seed, *shape, lo=-4, hi=5, dtype=F32):
  """Small integers: fp32 sums of them are exact in any order (the entry points that are not bit-reproducible)."""
  return torch.randint(lo, hi, shape, generator=gen(seed)).to(dtype)


def cols_from(rows, ld, c0):
  m = torch.zeros(rows, ld, dtype=torch.bool)
  m[:, c0:] = True
  return m


# ======================================================================================================================================
# flat element-wise kernels and small reductions
# ======================================================================================================================================
FLAT_N = (1, 7, 1003, 2051)   # below one vector; a vector tail; off vector x block; past one 8-wide 256-thread block


def _flat_cases():
  for n in FLAT_N:
    @case(f'cast_f32_bf16-n{n}', 'plm_cast_f32_bf16')
    def _(ar, n=n):
      src = ar.inp('src', rnd(1, n), misalign=True)
      dst = ar.out('dst', BF16, n)
      return lambda: call('plm_cast_f32_bf16', P(src), P(dst), n)

    @case(f'scale_bf16-n{n}', 'plm_scale_bf16')
    def _(ar, n=n):
      x = ar.inout('x', rnd(2, n, dtype=BF16))
      alpha = ar.inp('alpha', torch.tensor([0.37]), misalign=True)
      return lambda: call('plm_scale_bf16', P(x), n, P(alpha))

    for acc in (0, 1):
      @case(f'axpy_f32-n{n}-acc{acc}', 'plm_axpy_f32')
      def _(ar, n=n, acc=acc):
        out = ar.inout('out', rnd(3, n)) if acc else ar.out('out', F32, n)
        x = ar.inp('x', rnd(4, n), misalign=True)
        alpha = ar.inp('alpha', torch.tensor([1.7])) if acc else None   # NULL = 1.0 without accumulate
        return lambda: call('plm_axpy_f32', P(out), P(x), n, P(alpha), acc)

    @case(f'lerp_f32-n{n}', 'plm_lerp_f32')
    def _(ar, n=n):
      p = ar.inout('p', rnd(5, n), misalign=True)
      z = ar.inp('z', rnd(6, n))
      return lambda: call('plm_lerp_f32', P(p), P(z), n, 0.1)

    @case(f'mean_f32-n{n}', 'plm_mean_f32')
    def _(ar, n=n):
      x = ar.inp('x', rnd(7, n), misalign=True)
      out = ar.out('out', F32, 1)
      return lambda: call('plm_mean_f32', P(x), P(out), n)

    @case(f'sumsq_f32-n{n}', 'plm_sumsq_f32')
    def _(ar, n=n):
      x = ar.inp('x', rnd(8, n))
      scratch = ar.ws('scratch', 4096 * 4, dtype=F32)
      out = ar.out('out', F32, 1, misalign=True)
      return lambda: call('plm_sumsq_f32', P(x), n, P(scratch), P(out))


_flat_cases()


def _act_cases():
  for M, h in ((57, 72), (3, 2816)):   # partial 256-thread blocks: 513 and 1056 16-byte items
    assert (M * h // 8) % 256 != 0 and (h // 8) % 256 != 0
    for kind in (0, 1):
      @case(f'act_fwd-{M}x{h}-kind{kind}', 'plm_act_fwd')
      def _(ar, M=M, h=h, kind=kind):
        u = ar.inp('u', rnd(11, M, h, dtype=BF16), misalign=True)
        out = ar.out('out', BF16, M, h)
        return lambda: call('plm_act_fwd', P(u), P(out), M * h, kind)

      @case(f'act_bwd-{M}x{h}-kind{kind}', 'plm_act_bwd')
      def _(ar, M=M, h=h, kind=kind):
        dout = ar.inp('dout', rnd(12, M, h, dtype=BF16))
        u = ar.inp('u', rnd(11, M, h, dtype=BF16), misalign=True)
        du = ar.out('du', BF16, M, h)
        return lambda: call('plm_act_bwd', P(dout), P(u), P(du), M * h, kind)

    @case(f'swiglu_fwd-{M}x{h}', 'plm_swiglu_fwd')
    def _(ar, M=M, h=h):
      u = ar.inp('u', rnd(13, M, 2 * h, dtype=BF16), misalign=True)
      out = ar.out('out', BF16, M, h)
      return lambda: call('plm_swiglu_fwd', P(u), P(out), M, h)

    @case(f'swiglu_bwd-{M}x{h}', 'plm_swiglu_bwd')
    def _(ar, M=M, h=h):
      dout = ar.inp('dout', rnd(14, M, h, dtype=BF16), misalign=True)
      u = ar.inp('u', rnd(13, M, 2 * h, dtype=BF16))
      du = ar.out('du', BF16, M, 2 * h)
      return lambda: call('plm_swiglu_bwd', P(dout), P(u), P(du), M, h)


_act_cases()


# ======================================================================================================================================
# RMSNorm, column sums
# ======================================================================================================================================
def _rms_template(d):
  return 1 if d <= 256 else 3 if d <= 768 else 4 if d <= 1024 else 8


def _rms_cases():
  M = 67   # 17 blocks of 4 rows, the last with 3
  for d, tmpl in ((4, 1), (260, 3), (772, 4), (1028, 8), (2044, 8)):
    for full in (0, 1):
      @case(f'rmsnorm_fwd-d{d}-{"branch-xout" if full else "plain"}', 'plm_rmsnorm_fwd')
      def _(ar, d=d, tmpl=tmpl, full=full):
        assert _rms_template(d) == tmpl and d % (256 * 4) != 0, 'template / partly filled chunk'
        x = ar.inp('x', rnd(21, M, d), misalign=True)
        branch = ar.inp('branch', rnd(22, M, d, dtype=BF16)) if full else None
        xout = ar.out('xout', F32, M, d) if full else None
        w = ar.inp('w', rnd(23, d))
        y = ar.out('y', BF16, M, d)
        rstd = ar.out('rstd', F32, M)
        return lambda: call('plm_rmsnorm_fwd', P(x), P(branch), P(xout), P(w), P(y), P(rstd), M, d, 1e-6)

      @case(f'rmsnorm_bwd-d{d}-{"gin-bf16" if full else "plain"}', 'plm_rmsnorm_bwd plm_rmsnorm_bwd_blocks')
      def _(ar, d=d, tmpl=tmpl, full=full):
        nblk = int(L().plm_rmsnorm_bwd_blocks(M))
        assert _rms_template(d) == tmpl and nblk == 17
        dy = ar.inp('dy', rnd(24, M, d, dtype=BF16))
        x = ar.inp('x', rnd(21, M, d), misalign=True)
        w = ar.inp('w', rnd(23, d))
        rstd = ar.inp('rstd', rnd(25, M).abs() + 0.5)
        gin = ar.inp('gin', rnd(26, M, d)) if full else None
        dx = ar.out('dx', F32, M, d)
        dxb = ar.out('dx_bf16', BF16, M, d) if full else None
        part = ar.out('dw_partial', F32, nblk, d)
        return lambda: call('plm_rmsnorm_bwd', P(dy), P(x), P(w), P(rstd), P(gin), P(dx), P(dxb), P(part), M, d)

    for acc in (0, 1):
      @case(f'colsum_f32-d{d}-acc{acc}', 'plm_colsum_f32')
      def _(ar, d=d, acc=acc):
        part = ar.inp('part', rnd(27, 17, d), misalign=True)
        out = ar.inout('out', rnd(28, d)) if acc else ar.out('out', F32, d)
        return lambda: call('plm_colsum_f32', P(part), P(out), 17, d, acc)

    @case(f'colsum_f32_multi-d{d}', 'plm_colsum_f32_multi')
    def _(ar, d=d):
      from plainlm_amd import _lib
      parts = [ar.inp(f'part{i}', rnd(30 + i, 17, d), misalign=(i == 1)) for i in range(3)]
      outs = [ar.inout(f'out{i}', rnd(40 + i, d)) if i == 1 else ar.out(f'out{i}', F32, d) for i in range(3)]
      arr = (_lib.ColsumItem * 3)(*[_lib.ColsumItem(p.ptr, o.ptr, int(i == 1)) for i, (p, o) in enumerate(zip(parts, outs))])
      return lambda: call('plm_colsum_f32_multi', arr, 3, 17, d)


_rms_cases()


# ======================================================================================================================================
# embedding
# ======================================================================================================================================
EM, EV, ED = 1000, 300, 72


def _embed_ids(ends_used):
  ids = torch.randint(1, EV - 1, (EM,), generator=gen(51))
  ids[ids % 7 == 3] = 5            # unused rows and one heavily repeated id
  ids[100:140] = 17
  if ends_used:
    ids[0], ids[EM - 1], ids[500] = EV - 1, 0, 0
  return ids


def _embed_cases():
  for ends in (0, 1):
    tag = 'ends-used' if ends else 'ends-unused'

    @case(f'embed_fwd-{tag}', 'plm_embed_fwd')
    def _(ar, ends=ends):
      ids = ar.inp('ids', _embed_ids(ends), index_margin=(0, EV - 1))
      W = ar.inp('W', rnd(52, EV, ED), misalign=True)
      out = ar.out('out', F32, EM, ED)
      return lambda: call('plm_embed_fwd', P(ids), P(W), P(out), EM, ED, EV)

    @case(f'embed_bwd-{tag}', 'plm_embed_bwd')
    def _(ar, ends=ends):
      """Atomic adds: not bit-reproducible on real data, so small integers (fp32 sums exact in any order)."""
      idv = _embed_ids(ends)
      unused = torch.ones(EV, dtype=torch.bool)
      unused[idv] = False
      ids = ar.inp('ids', idv, index_margin=(0, EV - 1))
      dout = ar.inp('dout', ints(53, EM, ED), misalign=True)
      dW = ar.inout('dW', ints(54, EV, ED), untouched=unused[:, None].expand(EV, ED))
      return lambda: call('plm_embed_bwd', P(ids), P(dout), P(dW), EM, ED, EV)

    for acc in (0, 1):
      @case(f'embed_bwd_sorted-{tag}-acc{acc}', 'plm_embed_bwd_sorted plm_embed_bwd_workspace_bytes')
      def _(ar, ends=ends, acc=acc):
        nbytes = int(L().plm_embed_bwd_workspace_bytes(EM, EV))
        assert nbytes > 0 and EV >= 256, 'the sorted path, two radix passes'
        idv = _embed_ids(ends)
        unused = torch.ones(EV, dtype=torch.bool)
        unused[idv] = False
        ids = ar.inp('ids', idv, index_margin=(0, EV - 1))
        dout = ar.inp('dout', rnd(53, EM, ED), misalign=True)
        if acc:   # rows without tokens are documented as untouched
          dW = ar.inout('dW', rnd(54, EV, ED), untouched=unused[:, None].expand(EV, ED))
        else:     # every row is written (zeros for rows without tokens); dW need not be cleared
          dW = ar.out('dW', F32, EV, ED)
        ws = ar.ws('workspace', nbytes)
        return lambda: call('plm_embed_bwd_sorted', P(ids), P(dout), P(dW), EM, ED, EV, acc, P(ws), nbytes)


_embed_cases()


# ======================================================================================================================================
# casts with the transposed shadow, optimizer tail
# ======================================================================================================================================
SHADOW_ITEMS = ((40, 200, 48), (200, 40, 256), (8, 8, 8))   # (rows, cols, ld_t): ragged 64x64 tiles both ways; ld_t > rows; one quad
LONG_LIST = 58                                               # > 56 items: two launches


def _shadow_bufs(ar, i, rows, cols, ld_t):
  dst = ar.out(f'dst{i}', BF16, rows, cols)
  dst_t = ar.out(f'dst_t{i}', BF16, cols, ld_t, untouched=cols_from(cols, ld_t, rows)) if ld_t > rows else ar.out(f'dst_t{i}', BF16, cols, rows)
  return dst, dst_t


def _cast_t_cases():
  for rows, cols, ld_t in SHADOW_ITEMS:
    @case(f'cast_f32_bf16_t-{rows}x{cols}-ldt{ld_t}', 'plm_cast_f32_bf16_t')
    def _(ar, rows=rows, cols=cols, ld_t=ld_t):
      src = ar.inp('src', rnd(61, rows, cols), misalign=True)
      dst, dst_t = _shadow_bufs(ar, '', rows, cols, ld_t)
      return lambda: call('plm_cast_f32_bf16_t', P(src), P(dst), P(dst_t), rows, cols, ld_t)

  @case(f'cast_f32_bf16_t_multi-{LONG_LIST}items', 'plm_cast_f32_bf16_t_multi')
  def _(ar):
    from plainlm_amd import _lib
    assert LONG_LIST > 56
    arr = (_lib.CastItem * LONG_LIST)()
    for i in range(LONG_LIST):
      rows, cols, ld_t = SHADOW_ITEMS[i % 3]
      src = ar.inp(f'src{i}', rnd(62 + i, rows, cols), misalign=(i == 0))
      dst, dst_t = _shadow_bufs(ar, i, rows, cols, ld_t)
      arr[i] = _lib.CastItem(src.ptr, dst.ptr, dst_t.ptr, rows, cols, ld_t)
    return lambda: call('plm_cast_f32_bf16_t_multi', arr, LONG_LIST)


_cast_t_cases()

# kind -> (name, has m, has v, has a `first` step that does not read the state it creates)
OPTIM_KINDS = {5: ('adamw', 1, 1, 0), 1: ('nadamw', 1, 1, 0), 2: ('sgd', 1, 0, 1), 3: ('signsgd', 1, 0, 1), 4: ('sfo_adamw', 1, 1, 1)}


def _hparams(kind, first):
  from plainlm_amd import ops
  hp = ops.optim_hparams(kind, lr=0.01, weight_decay=0.1, first=bool(first), beta1=0.9, beta2=0.95, eps=1e-8, momentum=0.9, dampening=0.1,
                         bc2=0.0975, coef_grad=0.002, coef_avg=0.009, ckp1=0.25, bc1=0.19)
  assert hp.kind == kind
  return hp


def _state(ar, name, data, has, unread):
  """A state buffer: read and written (first = 0) or only written (first = 1: pre-filled with the fill byte, it must not reach a result)."""
  if not has:
    return None
  return ar.inout(name, data, unread=torch.ones(data.shape, dtype=torch.bool).reshape(-1, data.shape[-1]) if unread else None)


def _optim_cases():
  for kind, (name, has_m, has_v, has_first) in OPTIM_KINDS.items():
    for first in ((0, 1) if has_first else (0,)):
      @case(f'optim_f32-{name}-first{first}', 'plm_optim_f32')
      def _(ar, kind=kind, has_m=has_m, has_v=has_v, first=first):
        n = 1003
        hp = _hparams(kind, first)
        p = ar.inout('p', rnd(71, n), misalign=True)
        g = ar.inp('g', rnd(72, n))
        m = _state(ar, 'm', rnd(73, n), has_m, first)
        v = _state(ar, 'v', rnd(74, n).abs(), has_v, first)
        clip = ar.inp('clip_coef', torch.tensor([0.8]))
        return lambda: call('plm_optim_f32', C.byref(hp), P(p), P(g), P(m), P(v), n, P(clip))

      count = LONG_LIST if (kind, first) in ((5, 0), (4, 1)) else 3

      @case(f'optim_cast_multi-{name}-first{first}-{count}items', 'plm_optim_cast_multi')
      def _(ar, kind=kind, has_m=has_m, has_v=has_v, first=first, count=count):
        from plainlm_amd import _lib
        hp = _hparams(kind, first)
        arr = (_lib.OptimItem * count)()
        clip = ar.inp('clip_coef', torch.tensor([0.8]), misalign=True)
        for i in range(count):
          rows, cols, ld_t = SHADOW_ITEMS[i % 3]
          p = ar.inout(f'p{i}', rnd(75 + i, rows, cols))
          g = ar.inp(f'g{i}', rnd(175 + i, rows, cols))
          m = _state(ar, f'm{i}', rnd(275 + i, rows, cols), has_m, first)
          v = _state(ar, f'v{i}', rnd(375 + i, rows, cols).abs(), has_v, first)
          dst, dst_t = _shadow_bufs(ar, i, rows, cols, ld_t)
          arr[i] = _lib.OptimItem(p.ptr, g.ptr, m.ptr if m else None, v.ptr if v else None, dst.ptr, dst_t.ptr, rows, cols, ld_t)
        return lambda: call('plm_optim_cast_multi', C.byref(hp), arr, count, P(clip))

  @case('optim_f32-sgd-no-momentum', 'plm_optim_f32')
  def _(ar):
    hp = _hparams(2, 0)
    hp.momentum = 0.0   # m is neither read nor written and may be NULL
    p = ar.inout('p', rnd(71, 1003), misalign=True)
    g = ar.inp('g', rnd(72, 1003))
    return lambda: call('plm_optim_f32', C.byref(hp), P(p), P(g), P(None), P(None), 1003, P(None))


_optim_cases()


# ======================================================================================================================================
# cross entropy, scoring head
# ======================================================================================================================================
def _ce_cases():
  for V, ld, path in ((8200, 8208, 'fast<2>'), (777, 800, 'generic')):
    @case(f'ce_fwd_bwd-V{V}-{path}', 'plm_ce_fwd_bwd')
    def _(ar, V=V, ld=ld, path=path):
      M = 5
      fast = V % 8 == 0 and ld % 8 == 0 and V <= 1024 * 8 * 8
      nch = -(-(V // 8) // 1024)
      assert (path == 'generic') == (not fast) and (not fast or (nch == 2 and (V // 8) % 1024 < 8)), 'fast template with a nearly empty last chunk'
      whole = torch.ones(M, ld, dtype=torch.bool)   # the pad columns V..ld are written as zeros: part of the contract
      logits = ar.inout('logits', rnd(81, M, V, dtype=BF16, scale=3.0), ld=ld, written=whole, unread=cols_from(M, ld, V), misalign=True)
      targets = ar.inp('targets', torch.tensor([0, V - 1, -100, 17, V // 2]), index_margin=(0, V - 1))
      loss = ar.out('loss_rows', F32, M)
      return lambda: call('plm_ce_fwd_bwd', P(logits), P(targets), P(loss), M, V, ld, 0.2)


_ce_cases()


def _head_score_cases():
  for M, V, K, path in ((520, 264, 64, 'persistent'), (136, 777, 64, '128x128')):
    for want_lse in (1, 0):
      @case(f'head_score-{M}x{V}x{K}-{path}-lse{want_lse}', 'plm_head_score_bf16 plm_head_score_workspace_bytes')
      def _(ar, M=M, V=V, K=K, path=path, want_lse=want_lse):
        # the header's condition: shapes plm_gemm_bf16_nt serves with a 128x128 kernel (M < 512, V % 8 != 0) go through that kernel
        assert (path == '128x128') == (M < 512 or V % 8 != 0)
        assert V % 192 != 0 and V % 128 != 0 and M % 128 != 0, 'ragged last tile'
        nbytes = int(L().plm_head_score_workspace_bytes(M, V, K))
        assert nbytes > 0
        Y = ar.inp('Y', rnd(85, M, K, dtype=BF16), ld=K + 8, misalign=True)
        W = ar.inp('W', rnd(86, V, K, dtype=BF16), ld=K + 8)
        t = torch.randint(0, V, (M,), generator=gen(87))
        t[0], t[1], t[2], t[M - 1] = 0, V - 1, -100, V      # both ends, two ignored rows
        targets = ar.inp('targets', t, index_margin=(0, V - 1))
        nll = ar.out('nll', F32, M)
        lse = ar.out('lse', F32, M) if want_lse else None
        ws = ar.ws('workspace', nbytes)
        return lambda: call('plm_head_score_bf16', P(Y), K + 8, P(W), K + 8, P(targets), P(nll), P(lse), M, V, K, P(ws), nbytes)


_head_score_cases()


# ======================================================================================================================================
# bf16 GEMMs
# ======================================================================================================================================
def _nt_bufs(ar, M, N, K, dtype=BF16, c0=False):
  A = ar.inp('A', rnd(91, M, K, dtype=BF16), ld=K + 8, misalign=True)   # rows past M and columns K..ld are margin
  B = ar.inp('B', rnd(92, N, K, dtype=BF16), ld=K + 8)
  Cb = ar.inout('C', rnd(93, M, N), ld=N + 8) if c0 else ar.out('C', dtype, M, N, ld=N + 8)
  alpha = ar.inp('alpha', torch.tensor([0.7]))
  return A, B, Cb, alpha


def _nt_cases():
  # variant -> (M, N, K): one tile + 8 in M and in N; K a multiple of 64 where the kernel needs it, 200 where it does not
  shapes = {1: (136, 72, 200), 2: (136, 136, 128), 3: (264, 264, 128), 4: (264, 264, 128), 5: (264, 200, 128), 6: (264, 136, 128),
            7: (136, 200, 128)}
  for variant, (M, N, K) in shapes.items():
    @case(f'gemm_nt-v{variant}-{M}x{N}x{K}', 'plm_gemm_bf16_nt_ex')
    def _(ar, variant=variant, M=M, N=N, K=K):
      assert variant <= 1 or K % 64 == 0      # an explicit variant IS the path
      A, B, Cb, alpha = _nt_bufs(ar, M, N, K)
      return lambda: call('plm_gemm_bf16_nt_ex', P(A), K + 8, P(B), K + 8, P(Cb), N + 8, M, N, K, 0, 0, P(alpha), variant)

  for M, N, K, dt, acc, path in ((136, 72, 200, BF16, 0, 'reg128'), (136, 72, 200, F32, 1, 'reg128'), (136, 136, 128, BF16, 0, 'dma128'),
                                 (136, 136, 128, F32, 0, 'dma128')):
    @case(f'gemm_nt-auto-{M}x{N}x{K}-{"f32" if dt == F32 else "bf16"}-acc{acc}-{path}', 'plm_gemm_bf16_nt')
    def _(ar, M=M, N=N, K=K, dt=dt, acc=acc, path=path):
      # gemm_plan.h: the automatic choice needs M >= 512 for a persistent tile; K % 64 != 0 leaves only the register-staged kernel
      assert M < 512 and (path == 'reg128') == (K % 64 != 0)
      A, B, Cb, alpha = _nt_bufs(ar, M, N, K, dt, c0=bool(acc))
      return lambda: call('plm_gemm_bf16_nt', P(A), K + 8, P(B), K + 8, P(Cb), N + 8, M, N, K, int(dt == F32), acc, P(alpha))

  @case('gemm_nt-hybrid-2056x7432x1024', 'plm_gemm_bf16_nt_ws plm_gemm_nt_workspace_bytes', env={'PLM_NT_HYBRID_MIN_K': '64'})
  def _(ar):
    M, N, K = 2056, 7432, 1024    # 9 x 30 tiles of 256x256 on 256 workgroups: one full round + a stream-K remainder of one ragged tile row
    nbytes = int(L().plm_gemm_nt_workspace_bytes(M, N, K))
    assert nbytes > 0, 'shape does not take the hybrid schedule'
    A, B, Cb, alpha = _nt_bufs(ar, M, N, K)
    ws = ar.ws('workspace', nbytes)
    return lambda: call('plm_gemm_bf16_nt_ws', P(A), K + 8, P(B), K + 8, P(Cb), N + 8, M, N, K, 0, 0, P(alpha), 0, P(ws), nbytes)


_nt_cases()


def _tn_bufs(ar, i, M, N, K, acc):
  A = ar.inp(f'A{i}', rnd(95 + i, K, M, dtype=BF16), ld=M + 8, misalign=(i == 0))   # rows past K and columns M..ld are margin
  B = ar.inp(f'B{i}', rnd(96 + i, K, N, dtype=BF16), ld=N + 8)
  Cb = ar.inout(f'C{i}', rnd(97 + i, M, N), ld=N + 8) if acc else ar.out(f'C{i}', F32, M, N, ld=N + 8)
  return A, B, Cb


def _tn_cases():
  for M, N, K, split, kernel in ((136, 72, 200, 0, '128 reg'), (136, 72, 1024, 1, '128 dma'), (264, 264, 64, 0, 'persistent'),
                                 (264, 264, 1024, 1, 'persistent')):
    for acc in (0, 1):
      @case(f'gemm_tn-{M}x{N}x{K}-{"split" if split else "wholeK"}-acc{acc}', 'plm_gemm_bf16_tn plm_gemm_tn_workspace_bytes')
      def _(ar, M=M, N=N, K=K, split=split, kernel=kernel, acc=acc):
        nbytes = int(L().plm_gemm_tn_workspace_bytes(M, N, K))
        assert (nbytes > 0) == bool(split), 'whole-K / split-K'
        assert (kernel == 'persistent') == (K % 64 == 0 and M >= 256 and N >= 256) and (kernel != '128 reg' or K % 64 != 0)
        A, B, Cb = _tn_bufs(ar, 0, M, N, K, acc)
        alpha = ar.inp('alpha', torch.tensor([0.7]))
        ws = ar.ws('workspace', nbytes) if nbytes else None
        return lambda: call('plm_gemm_bf16_tn', P(A), M + 8, P(B), N + 8, P(Cb), N + 8, M, N, K, acc, P(alpha), P(ws), nbytes)

  @case('gemm_tn_grouped-3problems-K1024', 'plm_gemm_bf16_tn_grouped plm_gemm_tn_grouped_workspace_bytes')
  def _(ar):
    from plainlm_amd import _lib
    shapes, K = ((136, 72), (264, 264), (520, 264)), 1024
    n = len(shapes)
    Ms, Ns = (C.c_int64 * n)(*[s[0] for s in shapes]), (C.c_int64 * n)(*[s[1] for s in shapes])
    nbytes = int(L().plm_gemm_tn_grouped_workspace_bytes(Ms, Ns, n, K))
    assert nbytes > 16, 'shapes cannot be grouped, or nothing is split'
    alpha = ar.inp('alpha', torch.tensor([0.7]))
    arr = (_lib.TnProblem * n)()
    for i, (M, N) in enumerate(shapes):
      A, B, Cb = _tn_bufs(ar, i, M, N, K, acc=(i == 1))
      arr[i] = _lib.TnProblem(A.ptr, M + 8, B.ptr, N + 8, Cb.ptr, N + 8, M, N, int(i == 1), alpha.ptr)
    ws = ar.ws('workspace', nbytes)
    return lambda: call('plm_gemm_bf16_tn_grouped', arr, n, K, P(ws), nbytes)


_tn_cases()


# ---- the fused NT epilogues: one launch (M = 520, K = 64, the smallest N that qualifies) and the two-launch fallback (136, 200, 72) ----
def _rope_tables(T, hd, seed=101):
  ang = torch.rand(T, hd // 2, generator=gen(seed)) * 6.28
  return torch.cos(ang), torch.sin(ang)


def _fused_cases():
  for B_, T, K, fused in ((2, 260, 64, 1), (2, 68, 200, 0)):
    @case(f'qkv_rope-{B_ * T}x192x{K}-{"one-launch" if fused else "fallback"}', 'plm_qkv_rope_bf16')
    def _(ar, B_=B_, T=T, K=K, fused=fused):
      M, nh, hd = B_ * T, 1, 64
      N = 3 * nh * hd
      assert bool(fused) == (K % 64 == 0 and M >= 512 and hd == 64), 'the header\'s condition for the one-launch path'
      X = ar.inp('X', rnd(102, M, K, dtype=BF16), ld=K + 8, misalign=True)
      W = ar.inp('W', rnd(103, N, K, dtype=BF16, scale=0.2), ld=K + 8)
      cs, sn = _rope_tables(T, hd)
      rc, rs = ar.inp('rope_cos', cs), ar.inp('rope_sin', sn)      # exactly T rows
      Q = ar.out('QKV', BF16, M, N)
      return lambda: call('plm_qkv_rope_bf16', P(X), K + 8, P(W), K + 8, P(Q), N, M, K, P(rc), P(rs), B_, T, nh, hd)

  for M, K, h, fused in ((520, 64, 128, 1), (136, 200, 72, 0)):
    @case(f'fc1_swiglu-{M}x{2 * h}x{K}-{"one-launch" if fused else "fallback"}', 'plm_fc1_swiglu_bf16')
    def _(ar, M=M, K=K, h=h, fused=fused):
      assert bool(fused) == ((2 * h) % 256 == 0 and K % 64 == 0 and M >= 512)
      X = ar.inp('X', rnd(104, M, K, dtype=BF16), ld=K + 8, misalign=True)
      W = ar.inp('W', rnd(105, 2 * h, K, dtype=BF16, scale=0.2), ld=K + 8)
      U = ar.out('U', BF16, M, 2 * h)
      ACT = ar.out('ACT', BF16, M, h)
      return lambda: call('plm_fc1_swiglu_bf16', P(X), K + 8, P(W), K + 8, P(U), P(ACT), M, h, K)

  for M, K, h, fused in ((520, 64, 256, 1), (136, 200, 72, 0)):
    @case(f'fc2_dx_swiglu_bwd-{M}x{h}x{K}-{"one-launch" if fused else "fallback"}', 'plm_fc2_dx_swiglu_bwd_bf16')
    def _(ar, M=M, K=K, h=h, fused=fused):
      assert bool(fused) == (h % 256 == 0 and K % 64 == 0 and M >= 512)
      dY = ar.inp('dY', rnd(106, M, K, dtype=BF16), ld=K + 8, misalign=True)
      W2T = ar.inp('W2T', rnd(107, h, K, dtype=BF16, scale=0.2), ld=K + 8)
      U = ar.inp('U', rnd(108, M, 2 * h, dtype=BF16))
      DU = ar.out('DU', BF16, M, 2 * h)
      scratch = None if fused else ar.ws('scratch', M * h * 2, dtype=BF16)   # the one-launch path takes NULL (it would answer PLM_E_WORKSPACE otherwise)
      return lambda: call('plm_fc2_dx_swiglu_bwd_bf16', P(dY), K + 8, P(W2T), K + 8, P(U), P(DU), P(scratch), M, h, K)


_fused_cases()


# ======================================================================================================================================
# attention
# ======================================================================================================================================
AB, ANH = 2, 2                 # "rows beyond T" is the next sequence for b = 0 and the margin for b = 1
AT = (68, 260, 392)            # 4 rows past one 64-row tile; 4 rows past a 128- and a 256-row tile; a partial 64-key tile after full 128-row tiles
AHD = (32, 64, 128)


def _rope_cases():
  for hd in AHD:
    @case(f'rope_qk-hd{hd}', 'plm_rope_qk')
    def _(ar, hd=hd):
      B_, T, nh = 3, 20, 1
      assert (B_ * T * (2 * nh * hd // 8)) % 256 != 0, 'a partial last block'
      ld = 3 * nh * hd
      vblock = cols_from(B_ * T, ld, 2 * nh * hd)    # the v block is neither read nor written
      qkv = ar.inout('qkv', rnd(111, B_ * T, ld, dtype=BF16), untouched=vblock, misalign=True)
      cs, sn = _rope_tables(T, hd)
      rc, rs = ar.inp('rope_cos', cs), ar.inp('rope_sin', sn)
      return lambda: call('plm_rope_qk', P(qkv), P(rc), P(rs), B_, T, nh, hd)


_rope_cases()


def _doc_start(T):
  """Documents that end on a 64 / 128 / 256-row tile edge (b = 0) and one row past it (b = 1)."""
  ds = torch.zeros(AB, T, dtype=I32)
  for b, bounds in enumerate(((0, 64, 128, 256, 384), (0, 65, 129, 257, 385))):
    for s in bounds:
      if s < T:
        ds[b, s:] = s
  return ds


@functools.lru_cache(maxsize=None)
def _attn_setup(T, hd, doc):
  """Inputs of the forward and (from one real forward) of the backward, on the CPU."""
  from plainlm_amd import ops
  qkv = rnd(121, AB * T, 3 * ANH * hd, dtype=BF16, scale=0.7)
  dout = rnd(122, AB * T, ANH * hd, dtype=BF16)
  cs, sn = _rope_tables(T, hd)
  ds = _doc_start(T) if doc else None
  plan = None
  dsd = ds.cuda() if doc else None
  if doc:
    nints = int(L().plm_attn_doc_plan_bytes(AB, T)) // 4
    pl = torch.zeros(nints, dtype=I32, device='cuda')
    call('plm_attn_doc_plan', P(dsd), P(pl), AB, T, ANH)
    plan = pl.cpu()
  out, lse = ops.attn_fwd(qkv.cuda(), AB, T, ANH, doc_start=dsd, plan=plan.cuda() if doc else None)
  return qkv, dout, cs, sn, ds, plan, out.cpu(), lse.cpu()


def _attn_path(hd, doc):
  return 'attn_generic.hip' if hd != 64 else ('attn_doc.hip' if doc else 'attn_causal.hip')


def _attn_cases():
  for doc in (0, 1):
    for hd in AHD:
      for T in AT:
        tag = f'{"doc" if doc else "causal"}-hd{hd}-T{T}'

        @case(f'attn_fwd-{tag}', 'plm_attn_fwd')
        def _(ar, doc=doc, hd=hd, T=T):
          assert T % 4 == 0 and T % 64 in (4, 8) and _attn_path(hd, doc)
          qkv_, _, _, _, ds_, plan_, _, _ = _attn_setup(T, hd, doc)
          qkv = ar.inp('qkv', qkv_, misalign=True)
          ds = ar.inp('doc_start', ds_, index_margin=(0, 4)) if doc else None
          plan = ar.inp('doc_plan', plan_, index_margin=(0, 1)) if doc and hd == 64 else None
          out = ar.out('out', BF16, AB * T, ANH * hd)
          lse = ar.out('lse', F32, AB * ANH, T)
          return lambda: call('plm_attn_fwd', P(qkv), P(ds), P(plan), P(out), P(lse), AB, T, ANH, hd)

        @case(f'attn_bwd-{tag}', 'plm_attn_bwd')
        def _(ar, doc=doc, hd=hd, T=T):
          qkv_, dout_, cs, sn, ds_, plan_, out_, lse_ = _attn_setup(T, hd, doc)
          qkv = ar.inp('qkv', qkv_, misalign=True)
          out = ar.inp('out', out_)
          dout = ar.inp('dout', dout_)
          lse = ar.inp('lse', lse_.reshape(AB * ANH, T))
          rc, rs = ar.inp('rope_cos', cs), ar.inp('rope_sin', sn)   # exactly T rows
          ds = ar.inp('doc_start', ds_, index_margin=(0, 4)) if doc else None
          plan = ar.inp('doc_plan', plan_, index_margin=(0, 1)) if doc and hd == 64 else None
          dqkv = ar.out('dqkv', BF16, AB * T, 3 * ANH * hd)
          delta = ar.out('delta', F32, AB * ANH, T)
          return lambda: call('plm_attn_bwd', P(qkv), P(out), P(dout), P(lse), P(rc), P(rs), P(ds), P(plan), P(dqkv), P(delta), AB, T, ANH, hd)

  for T in AT:
    @case(f'attn_doc_plan-T{T}', 'plm_attn_doc_plan plm_attn_doc_plan_bytes')
    def _(ar, T=T):
      nints = int(L().plm_attn_doc_plan_bytes(AB, T)) // 4
      n = AB * ((T + 127) // 128)
      pq = (8 + AB * T + 3) // 4 * 4
      cap = n + n // 4
      assert nints == pq + 8 * cap
      # written for certain: the header, doc_end[B, T] and the first n items of each list (every tile is an item; halves of split tiles follow,
      # their number is in the header); the alignment gap and the unused item slots are undefined
      w = torch.zeros(1, nints, dtype=torch.bool)
      w[0, :8 + AB * T] = True
      w[0, pq:pq + 4 * n] = True
      w[0, pq + 4 * cap:pq + 4 * cap + 4 * n] = True
      ds = ar.inp('doc_start', _doc_start(T), index_margin=(0, 4), misalign=True)
      plan = ar.out('plan', I32, nints, written=w)
      return lambda: call('plm_attn_doc_plan', P(ds), P(plan), AB, T, ANH)

    @case(f'attn_doc_start_from_mask-T{T}', 'plm_attn_doc_start_from_mask')
    def _(ar, T=T):
      ds = _doc_start(T).long()
      pos = torch.arange(T)
      m = (pos[None, None, :] >= ds[:, :, None]) & (pos[None, None, :] <= pos[None, :, None])
      mask = ar.inp('mask', m, misalign=True)
      out = ar.out('doc_start', I32, AB, T)
      status = ar.inout('status', torch.zeros(1, dtype=I32))      # caller-zeroed
      return lambda: call('plm_attn_doc_start_from_mask', P(mask), P(out), P(status), AB, T)


_attn_cases()


# ---- dense masks ----
def _dense_mask(Mm, T):
  """Bernoulli(1/2) with empty rows, one empty 128 x 64 tile and (T >= 260) one full tile."""
  m = torch.rand(Mm, T, T, generator=gen(131)) < 0.5
  m[:, 3, :] = False
  m[:, T - 1, :] = False
  m[:, 0:128, 64:128] = False
  if T >= 260:
    m[:, 128:256, 0:64] = True
  return m


def _mask_layout(Mm, T):
  W, NQT = (T + 63) // 64, (T + 127) // 128
  nb, ncls = Mm * T * W * 8, Mm * NQT * W
  total = int(L().plm_attn_mask_bytes(Mm, T))
  assert total == (nb + ncls + 15) // 16 * 16 and nb % 16 == 0     # the documented offsets: bits, then tile_class
  return nb, ncls, total


@functools.lru_cache(maxsize=None)
def _masked_setup(T, hd, bs):
  from plainlm_amd import ops
  Mm = AB if bs else 1
  mask = _dense_mask(Mm, T)
  nb, ncls, total = _mask_layout(Mm, T)
  packed = torch.zeros(total, dtype=U8, device='cuda')
  md = mask.cuda()
  call('plm_attn_mask_pack', P(md), bs, P(packed), C.c_void_p(packed.data_ptr() + nb), AB, T)
  qkv = rnd(132, AB * T, 3 * ANH * hd, dtype=BF16, scale=0.7)
  dout = rnd(133, AB * T, ANH * hd, dtype=BF16)
  cs, sn = _rope_tables(T, hd)
  out = torch.empty(AB * T, ANH * hd, dtype=BF16, device='cuda')
  lse = torch.empty(AB * ANH, T, dtype=F32, device='cuda')
  qd = qkv.cuda()
  call('plm_attn_fwd_masked', P(qd), P(packed), C.c_void_p(packed.data_ptr() + nb), bs, P(out), P(lse), AB, T, ANH, hd)
  torch.cuda.synchronize()
  return qkv, dout, cs, sn, packed.cpu(), out.cpu(), lse.cpu()


def _masked_cases():
  for bs in (0, 1):
    for T in AT:
      @case(f'attn_mask_pack-bs{bs}-T{T}', 'plm_attn_mask_pack plm_attn_mask_bytes')
      def _(ar, bs=bs, T=T):
        Mm = AB if bs else 1
        nb, ncls, total = _mask_layout(Mm, T)
        w = torch.zeros(1, total, dtype=torch.bool)
        w[0, :nb + ncls] = True
        mask = ar.inp('mask', _dense_mask(Mm, T), misalign=True)
        packed = ar.out('bits+tile_class', U8, total, written=w)      # both views of one allocation
        return lambda: call('plm_attn_mask_pack', P(mask), bs, P(packed), C.c_void_p(packed.ptr + nb), AB, T)

      for hd in AHD:
        tag = f'hd{hd}-bs{bs}-T{T}'

        @case(f'attn_fwd_masked-{tag}', 'plm_attn_fwd_masked')
        def _(ar, bs=bs, T=T, hd=hd):
          qkv_, _, _, _, packed_, _, _ = _masked_setup(T, hd, bs)
          nb = _mask_layout(AB if bs else 1, T)[0]
          qkv = ar.inp('qkv', qkv_, misalign=True)
          packed = ar.inp('bits+tile_class', packed_)
          out = ar.out('out', BF16, AB * T, ANH * hd)
          lse = ar.out('lse', F32, AB * ANH, T)
          return lambda: call('plm_attn_fwd_masked', P(qkv), P(packed), C.c_void_p(packed.ptr + nb), bs, P(out), P(lse), AB, T, ANH, hd)

        @case(f'attn_bwd_masked-{tag}', 'plm_attn_bwd_masked')
        def _(ar, bs=bs, T=T, hd=hd):
          qkv_, dout_, cs, sn, packed_, out_, lse_ = _masked_setup(T, hd, bs)
          nb = _mask_layout(AB if bs else 1, T)[0]
          qkv = ar.inp('qkv', qkv_, misalign=True)
          out = ar.inp('out', out_)
          dout = ar.inp('dout', dout_)
          lse = ar.inp('lse', lse_)
          rc, rs = ar.inp('rope_cos', cs), ar.inp('rope_sin', sn)
          packed = ar.inp('bits+tile_class', packed_)
          dqkv = ar.out('dqkv', BF16, AB * T, 3 * ANH * hd)
          delta = ar.out('delta', F32, AB * ANH, T)
          return lambda: call('plm_attn_bwd_masked', P(qkv), P(out), P(dout), P(lse), P(rc), P(rs), P(packed), C.c_void_p(packed.ptr + nb), bs,
                              P(dqkv), P(delta), AB, T, ANH, hd)


_masked_cases()


# ======================================================================================================================================
# MXFP8
# ======================================================================================================================================
def _mx_quant_bufs(ar, i, rows, cols, ld, rowwise, colwise):
  kq, kt = (cols + 127) // 128 * 128, (rows + 127) // 128 * 128
  x = ar.inp(f'x{i}', rnd(141 + i, rows, cols, dtype=BF16, scale=5.0), ld=ld, misalign=(i == 0))
  # the whole padded width is written (padding elements zero with scale byte 0)
  q = ar.out(f'q{i}', U8, rows, kq) if rowwise else None
  s = ar.out(f's{i}', U8, rows, kq // 32) if rowwise else None
  qt = ar.out(f'qt{i}', U8, cols, kt) if colwise else None
  st = ar.out(f'st{i}', U8, cols, kt // 32) if colwise else None
  return x, q, s, qt, st


def _mx_cases():
  rows, cols, ld = 77, 200, 264
  for rowwise, colwise in ((1, 1), (1, 0), (0, 1)):
    @case(f'mx_quant-{rows}x{cols}-rows{rowwise}-cols{colwise}', 'plm_mx_quant')
    def _(ar, rowwise=rowwise, colwise=colwise):
      x, q, s, qt, st = _mx_quant_bufs(ar, 0, rows, cols, ld, rowwise, colwise)
      return lambda: call('plm_mx_quant', P(x), ld, rows, cols, P(q), P(s), P(qt), P(st))

  @case('mx_quant_multi-3items', 'plm_mx_quant_multi')
  def _(ar):
    from plainlm_amd import _lib
    arr = (_lib.MxQuantItem * 3)()
    for i, (rw, cw) in enumerate(((1, 1), (0, 1), (1, 0))):
      x, q, s, qt, st = _mx_quant_bufs(ar, i, rows, cols, ld, rw, cw)
      pp = lambda b: b.ptr if b is not None else None  # noqa: E731
      arr[i] = _lib.MxQuantItem(x.ptr, ld, rows, cols, pp(q), pp(s), pp(qt), pp(st))
    return lambda: call('plm_mx_quant_multi', arr, 3)

  for mode, name in ((0, 'bf16'), (1, 'f32'), (2, 'f32-acc')):
    @case(f'gemm_mx_nt-200x160x512-{name}', 'plm_gemm_mx_nt')
    def _(ar, mode=mode):
      M, N, Kp = 200, 160, 512
      assert M % 128 != 0 and N % 128 != 0 and Kp % 128 == 0

      def e4m3(seed, r):   # finite e4m3fn bytes (0x7F / 0xFF are NaN) and scale bytes near 2^0
        d = torch.randint(0, 0x78, (r, Kp), generator=gen(seed)) | (torch.randint(0, 2, (r, Kp), generator=gen(seed + 1)) << 7)
        return d.to(U8), torch.randint(124, 131, (r, Kp // 32), generator=gen(seed + 2)).to(U8)
      a, as_ = e4m3(151, M)
      b, bs_ = e4m3(161, N)
      A, As = ar.inp('A', a, misalign=True), ar.inp('As', as_)
      B, Bs = ar.inp('B', b), ar.inp('Bs', bs_)
      if mode == 2:
        Cb = ar.inout('C', rnd(171, M, N), ld=N + 8)
      else:
        Cb = ar.out('C', BF16 if mode == 0 else F32, M, N, ld=N + 8)
      return lambda: call('plm_gemm_mx_nt', P(A), P(As), P(B), P(Bs), P(Cb), N + 8, M, N, Kp, mode)


_mx_cases()


# ======================================================================================================================================
# the test
# ======================================================================================================================================
@pytest.mark.parametrize('cid', list(CASES))
def test_footprint(cid):
  FP.run_on_gpu(cid, *CASES[cid])


NOT_HERE = ('plm_comm_', 'plm_probe_', 'plm_version', 'plm_last_error_string', 'plm_reload_env', 'plm_set_cu_reserve')


def test_every_entry_point_has_a_footprint_case():
  """Every function of include/plainlm_hip.h that launches something, or sizes what a launch needs, has a row in the CASES of some
  tests/test_footprint_*gpu.py (the comm entry points need several ranks, the probes are exact already).  The files are found by
  glob: a new entry point brings a case file of its own."""
  from plainlm_amd import _lib
  here = os.path.dirname(os.path.abspath(__file__))
  files = sorted(glob.glob(os.path.join(here, 'test_footprint_*gpu.py')))
  assert os.path.abspath(__file__) in files, files
  covered = set()
  for f in files:
    mod = importlib.import_module(os.path.splitext(os.path.basename(f))[0])
    covered |= {e for row in mod.CASES.values() for e in row[0]}
  want = {f for f in _lib.header_functions() if not f.startswith(NOT_HERE)}
  assert want - covered == set(), sorted(want - covered)
  assert covered - want == set(), sorted(covered - want)
