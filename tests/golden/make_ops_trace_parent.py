"""What every wrapper of plainlm_amd/ops.py hands to the C ABI, recorded BEFORE ops.py got one operand contract, one workspace arena and
one launch bracket (commit 2afedcd), for tests/test_ops_trace_host.py, which replays the same scenarios on the working tree.

Nothing runs on a GPU and the library is not loaded: ``_lib.load`` returns a fake whose ``plm_*`` attributes record their arguments,
``ops._stream`` returns a constant, and operands are CPU tensors seen through a torch.Tensor subclass whose ``is_cuda`` is True.

A library call is recorded as [entry point, argument ...], decoded with _lib.SIGNATURES: scalars as given; a pointer as 'NULL', 'stream',
'<operand name>+<byte offset>', 'ret<k>' (+<offset>: the k-th tensor the wrapper returned) or 'scratch' (neither - its identity is
deliberately not recorded, its size argument is a scalar and is); ctypes item tables and structs as lists of their fields, pointers
encoded the same way.  Pure queries (``*_bytes``, ``plm_rmsnorm_bwd_blocks``) are answered but not recorded: memoising them may change
their count.  The size queries answer a deterministic function of their arguments and of the reserve last given to the fake
``plm_set_cu_reserve``, so a stale memo, or a query asked before the launch hook, shows as a wrong size in the launch's arguments.

Per scenario:
  'calls':   the library calls with ops.LAUNCH_HOOK and ops.PROFILE unset, and ['attn_flops', masked?] wherever ops.attn_flops ran
  'ret':     dtype[shape]s[strides] of every tensor returned (None / bool / int as they are)
  'inst':    the same call with a hook and a profile list set (torch.cuda.Event faked): the sequence of ['hook', family, work],
             ['event'] (an event recorded), ['attn_flops', masked?] and entry-point names - the calls' arguments are those of 'calls',
             or the scenario holds 'inst_calls' in full
  'profile': the (family, work) pairs ops.PROFILE received
  'raised':  [exception type, message] in place of all of the above; 'launches' is then the number of library calls made (0)
The 'hook-reserve' scenarios run with a hook that raises the CU reserve at its first call.

Every base case is also run once per tensor argument and mutation (other dtype, one more dim, non-unit inner stride, padded rows,
off the GPU, one row less, one column less): what the parent refuses is recorded as 'raised', what it accepts with its calls.

Only names that exist on both sides of the change are used, so this one file runs on the parent and on the working tree alike.

Run from a checkout of commit 2afedcd (no GPU, no built library needed):
  python tests/golden/make_ops_trace_parent.py [output .json]
"""
import contextlib
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch  # noqa: E402

from plainlm_amd import _lib, ops  # noqa: E402

BF16, F32, I64, I32, U8 = torch.bfloat16, torch.float32, torch.int64, torch.int32, torch.uint8
STREAM = 0x57AE00
QUERIES = ('plm_rmsnorm_bwd_blocks',)


class Gpu(torch.Tensor):
  is_cuda = True


def gpu(t):
  return t.as_subclass(Gpu)


def span_bytes(t):
  if t.numel() == 0:
    return 0
  return (sum((n - 1) * s for n, s in zip(t.shape, t.stride())) + 1) * t.element_size()


def query_answer(name, a, reserve):
  """The fake size queries: deterministic in their arguments and the CU reserve; 0 where the library refuses or needs nothing."""
  if name == 'plm_rmsnorm_bwd_blocks':
    return (a[0] + 63) // 64
  if name == 'plm_attn_doc_plan_bytes':
    return a[0] * a[1] * 16
  if name == 'plm_attn_mask_bytes':
    M, T = a
    return M * T * ((T + 63) // 64) * 8 + (M * ((T + 127) // 128) * ((T + 63) // 64) + 15) // 16 * 16
  if name == 'plm_gemm_nt_workspace_bytes':
    M, N, K = a
    return 0 if M < 8 else 256 * (1 + (M + 3 * N + 5 * K) % 5) + 64 * reserve
  if name == 'plm_gemm_tn_workspace_bytes':
    M, N, K = a
    return 0 if K < 16 else 128 * (1 + (M + 3 * N + 5 * K) % 7) + 64 * reserve
  if name == 'plm_gemm_tn_grouped_workspace_bytes':
    Ms, Ns, n, K = a
    return 0 if K % 2 else 512 + 32 * sum(Ms[i] + Ns[i] for i in range(n)) + 64 * reserve
  if name in ('plm_head_score_workspace_bytes', 'plm_head_predict_workspace_bytes'):
    M, V, K = a
    return 0 if M == 1 else 64 * (1 + (M + V + K) % 9) + 32 * reserve + (8 if 'predict' in name else 0)
  if name in ('plm_attn_decode_workspace_bytes', 'plm_attn_extend_workspace_bytes'):
    B, n, nh, hd, Tmax, splits = a if 'extend' in name else (a[0], 1) + tuple(a[1:])
    if hd not in (64, 128) or not 0 <= splits <= 64 or n < 1 or B < 1 or nh < 1 or Tmax < 1:
      return 0
    return 16 + 256 * (B * n * nh + splits) + Tmax
  if name == 'plm_embed_bwd_workspace_bytes':
    M, V = a
    return 0 if V >= 65536 else 16 * M + 4 * V
  raise AssertionError(f'no fake answer for {name}')


class Recorder:
  def __init__(self):
    self.entries, self.operands, self.reserve, self.fc2_refusals, self.sizes = [], [], 0, 0, []
    self.lib = FakeLib(self)

  def operand(self, name, t):
    if isinstance(t, torch.Tensor):
      self.operands.append((name, t.data_ptr(), t.data_ptr() + span_bytes(t), t))

  def ptr(self, v):
    v = v.value if isinstance(v, C.c_void_p) else v
    if not v:
      return 'NULL'
    if v == STREAM:
      return 'stream'
    for name, lo, hi, _ in self.operands:
      if lo <= v < hi:
        return f'{name}+{v - lo}'
    return int(v)  # a returned tensor or scratch: decided when the wrapper has returned

  def struct(self, s):
    return [self.ptr(getattr(s, f)) if ty is C.c_void_p else getattr(s, f) for f, ty in s._fields_]

  def arg(self, a, ty):
    if ty is C.c_void_p:
      return self.ptr(a)
    if isinstance(a, C.Array):
      return [self.struct(x) if isinstance(x, C.Structure) else x for x in a]
    if hasattr(a, '_obj'):  # ctypes.byref
      return self.struct(a._obj)
    if isinstance(a, C.Structure):
      return self.struct(a)
    return a

  def call(self, name, args):
    if name == 'plm_set_cu_reserve':
      self.reserve = int(args[0])
    if name.endswith('_bytes') or name in QUERIES:
      return query_answer(name, args, self.reserve)
    types = _lib.SIGNATURES[name][1]
    assert len(types) == len(args), f'{name}: {len(args)} arguments for {len(types)} parameters'
    self.entries.append([name] + [self.arg(a, ty) for a, ty in zip(args, types)])
    self.sizes += [int(a) for a, ty in zip(args, types) if ty is C.c_size_t]
    if name == 'plm_fc2_dx_swiglu_bwd_bf16' and self.fc2_refusals:
      self.fc2_refusals -= 1
      return -4
    return None if _lib.SIGNATURES[name][0] is None else 0

  def launches(self):
    return sum(1 for e in self.entries if e[0].startswith('plm_') and e[0] not in ('plm_set_cu_reserve', 'plm_reload_env'))

  def finish(self, result):
    """Entries with the pointers that were left open resolved against what the wrapper returned; the returned values' signatures."""
    flat = []

    def walk(v):
      if isinstance(v, torch.Tensor):
        flat.append(v)
        return f'{str(v.dtype)[6:]}{list(v.shape)}s{list(v.stride())}'
      if isinstance(v, ops.MxTensor):
        return ['mx', list(v.shape), walk(v.data), walk(v.scales)]
      if isinstance(v, (C.Array, C.Structure)):
        return type(v).__name__
      if isinstance(v, (list, tuple)):
        return [walk(x) for x in v]
      return v
    ret = walk(result)
    ranges = [(k, t.data_ptr(), t.data_ptr() + span_bytes(t)) for k, t in enumerate(flat)]

    def fix(v):
      if isinstance(v, list):
        return [fix(x) for x in v]
      if isinstance(v, int) and not isinstance(v, bool) and v >= 1 << 32:  # an open pointer (no scalar here comes near)
        for k, lo, hi in ranges:
          if lo <= v < hi:
            return f'ret{k}' + (f'+{v - lo}' if v > lo else '')
        return 'scratch'
      return v
    return [fix(e) for e in self.entries], ret


class FakeLib:
  def __init__(self, rec):
    self._rec = rec

  def __getattr__(self, name):
    if not name.startswith('plm_'):
      raise AttributeError(name)
    return lambda *args: self._rec.call(name, args)


class FakeEvent:
  rec = None

  def __init__(self, enable_timing=False):
    pass

  def record(self):
    FakeEvent.rec.entries.append(['event'])


@contextlib.contextmanager
def faked(rec):
  """ops against the recorder: the library, the stream, torch.cuda.Event and a recording attn_flops; hook, profile and reserve reset."""
  saved = (_lib.load, ops._stream, torch.cuda.Event, ops.attn_flops, ops.LAUNCH_HOOK, ops.PROFILE)
  flops = ops.attn_flops

  def attn_flops(B, T, nh, hd, doc_start=None):
    rec.entries.append(['attn_flops', doc_start is not None])
    return flops(B, T, nh, hd, doc_start)
  FakeEvent.rec = rec
  _lib.load, ops._stream, torch.cuda.Event, ops.attn_flops = (lambda: rec.lib), (lambda: C.c_void_p(STREAM)), FakeEvent, attn_flops
  ops.LAUNCH_HOOK = ops.PROFILE = None
  ops.set_cu_reserve(0)
  rec.entries.clear()
  try:
    yield rec
  finally:
    ops.set_cu_reserve(0)
    _lib.load, ops._stream, torch.cuda.Event, ops.attn_flops, ops.LAUNCH_HOOK, ops.PROFILE = saved


# ---- the cases: name -> (operands(), call(**operands)) ---------------------------------------------------------------------------
def z(shape, dtype, ld=None):
  """Zeros on the fake GPU; ld: the row stride of a 2-D tensor (a column slice of a wider buffer)."""
  if ld is None:
    return gpu(torch.zeros(tuple(shape), dtype=dtype))
  return gpu(torch.zeros((shape[0], ld), dtype=dtype))[:, :shape[1]]


def mx(rows, k):
  kp = ops.mx_pad(k)
  return ops.MxTensor(z((rows, kp), U8), z((rows, kp // 32), U8), (rows, k))


B_, T_, NH, HD, TMAX, NCH = 2, 8, 2, 64, 8, 3  # attention: batch, seq, heads, head_dim, cache rows, chunk width
DM = NH * HD
CASES = {}


def case(name, operands, call, **opts):
  CASES[name] = (operands, call, opts)


def rope():
  return dict(rope_cos=z((TMAX, HD // 2), F32), rope_sin=z((TMAX, HD // 2), F32))


def attn_saved():
  return dict(qkv=z((B_ * T_, 3 * DM), BF16), out=z((B_ * T_, DM), BF16), dout=z((B_ * T_, DM), BF16), lse=z((B_, NH, T_), F32), **rope())


def packed_mask():
  return dict(bits=z((B_, T_, 1), I64), tile_class=z((B_, 1, 1), U8))


case('cast_bf16', lambda: dict(src=z((5, 7), F32)), lambda src: ops.cast_bf16(src))
case('cast_bf16:out', lambda: dict(src=z((5, 7), F32), out=z((5, 7), BF16)), lambda src, out: ops.cast_bf16(src, out=out))
case('cast_bf16_t', lambda: dict(src=z((5, 7), F32)), lambda src: ops.cast_bf16_t(src))
case('cast_bf16_t:out', lambda: dict(src=z((5, 7), F32), out=z((5, 7), BF16), out_t=z((7, 5), BF16, ld=8)),
     lambda src, out, out_t: ops.cast_bf16_t(src, out=out, out_t=out_t))
case('cast_bf16_t_multi', lambda: dict(src=z((5, 7), F32), out=z((5, 7), BF16), out_t=z((7, 5), BF16, ld=8), src2=z((3, 4), F32),
                                       out2=z((3, 4), BF16), out_t2=z((4, 3), BF16)),
     lambda src, out, out_t, src2, out2, out_t2: ops.cast_bf16_t_multi([(src, out, out_t), (src2, out2, out_t2)]))
case('cast_bf16_t_multi:empty', dict, lambda: ops.cast_bf16_t_multi([]))
case('mx_quant', lambda: dict(x=z((5, 40), BF16, ld=48)), lambda x: ops.mx_quant(x))
case('mx_quant:rows', lambda: dict(x=z((5, 40), BF16)), lambda x: ops.mx_quant(x, cols=False))
case('mx_quant:cols', lambda: dict(x=z((5, 40), BF16)), lambda x: ops.mx_quant(x, rows=False))
case('mx_quant:neither', lambda: dict(x=z((5, 40), BF16)), lambda x: ops.mx_quant(x, rows=False, cols=False))
case('mx_quant_multi', lambda: dict(x=z((5, 40), BF16), x2=z((3, 33), BF16, ld=40)), lambda x, x2: ops.mx_quant_multi([x, x2], cols=False))
case('mx_quant_multi:empty', dict, lambda: ops.mx_quant_multi([]))
case('gemm_mx_nt', lambda: dict(a=mx(5, 40), b=mx(6, 40)), lambda a, b: ops.gemm_mx_nt(a, b))
case('gemm_mx_nt:f32', lambda: dict(a=mx(5, 40), b=mx(6, 40)), lambda a, b: ops.gemm_mx_nt(a, b, out_dtype=F32))
case('gemm_mx_nt:acc', lambda: dict(a=mx(5, 40), b=mx(6, 40), out=z((5, 6), F32, ld=8)),
     lambda a, b, out: ops.gemm_mx_nt(a, b, out=out, accumulate=True))
case('gemm_mx_nt:out-bf16', lambda: dict(a=mx(5, 40), b=mx(6, 40), out=z((5, 6), BF16)), lambda a, b, out: ops.gemm_mx_nt(a, b, out=out))
case('gemm_mx_nt:acc-bf16', lambda: dict(a=mx(5, 40), b=mx(6, 40), out=z((5, 6), BF16)),
     lambda a, b, out: ops.gemm_mx_nt(a, b, out=out, accumulate=True))
case('gemm_mx_nt:acc-no-out', lambda: dict(a=mx(5, 40), b=mx(6, 40)), lambda a, b: ops.gemm_mx_nt(a, b, accumulate=True))
case('gemm_mx_nt:k-differs', lambda: dict(a=mx(5, 40), b=mx(6, 41)), lambda a, b: ops.gemm_mx_nt(a, b))
case('gemm_mx_nt:not-mx', lambda: dict(a=z((5, 40), BF16), b=mx(6, 40)), lambda a, b: ops.gemm_mx_nt(a, b))
case('embed_fwd', lambda: dict(ids=z((2, 6), I64), W=z((20, 8), F32)), lambda ids, W: ops.embed_fwd(ids, W))
case('embed_bwd', lambda: dict(ids=z((12,), I64), dout=z((12, 8), F32), dW=z((20, 8), F32)), lambda ids, dout, dW: ops.embed_bwd(ids, dout, dW))
case('embed_bwd_sorted', lambda: dict(ids=z((2, 6), I64), dout=z((12, 8), F32), dW=z((20, 8), F32)),
     lambda ids, dout, dW: ops.embed_bwd_sorted(ids, dout, dW, False))
case('embed_bwd_sorted:acc', lambda: dict(ids=z((12,), I64), dout=z((12, 8), F32), dW=z((20, 8), F32)),
     lambda ids, dout, dW: ops.embed_bwd_sorted(ids, dout, dW, True))
case('embed_bwd_sorted:big-V', lambda: dict(ids=z((12,), I64), dout=z((12, 1), F32), dW=z((65536, 1), F32)),
     lambda ids, dout, dW: ops.embed_bwd_sorted(ids, dout, dW, True))
case('embed_bwd_sorted:sliced', lambda: dict(ids=z((2 * 65536 + 10,), I64), dout=z((2 * 65536 + 10, 2), F32), dW=z((20, 2), F32)),
     lambda ids, dout, dW: ops.embed_bwd_sorted(ids, dout, dW, False), mutate=False)
case('embed_bwd_sorted:sliced-big-V', lambda: dict(ids=z((65536 + 10,), I64), dout=z((65536 + 10, 1), F32), dW=z((65536, 1), F32)),
     lambda ids, dout, dW: ops.embed_bwd_sorted(ids, dout, dW, False), mutate=False)
case('rmsnorm_fwd', lambda: dict(x=z((5, 16), F32), w=z((16,), F32)), lambda x, w: ops.rmsnorm_fwd(x, w, 1e-6))
case('rmsnorm_fwd:branch', lambda: dict(x=z((5, 16), F32), w=z((16,), F32), branch=z((5, 16), BF16)),
     lambda x, w, branch: ops.rmsnorm_fwd(x, w, 1e-5, branch=branch))
case('rmsnorm_fwd:xout', lambda: dict(x=z((5, 16), F32), w=z((16,), F32)), lambda x, w: ops.rmsnorm_fwd(x, w, 1e-6, write_xout=True))
case('rmsnorm_bwd', lambda: dict(dy=z((70, 16), BF16), x=z((70, 16), F32), w=z((16,), F32), rstd=z((70,), F32)),
     lambda dy, x, w, rstd: ops.rmsnorm_bwd(dy, x, w, rstd))
case('rmsnorm_bwd:gin-bf16-dw', lambda: dict(dy=z((70, 16), BF16), x=z((70, 16), F32), w=z((16,), F32), rstd=z((70,), F32), gin=z((70, 16), F32),
                                             dw_out=z((16,), F32)),
     lambda dy, x, w, rstd, gin, dw_out: ops.rmsnorm_bwd(dy, x, w, rstd, gin=gin, want_bf16=True, dw_out=dw_out, dw_accumulate=True))
case('rmsnorm_bwd:defer', lambda: dict(dy=z((70, 16), BF16), x=z((70, 16), F32), w=z((16,), F32), rstd=z((70,), F32)),
     lambda dy, x, w, rstd: ops.rmsnorm_bwd(dy, x, w, rstd, dw_accumulate=True, defer_dw=True))
case('colsum_multi', lambda: dict(part=z((2, 16), F32), out=z((16,), F32), part2=z((2, 16), F32), out2=z((16,), F32)),
     lambda part, out, part2, out2: ops.colsum_multi([(part, out, False), (part2, out2, True)]))
case('colsum_multi:empty', dict, lambda: ops.colsum_multi([]))
case('swiglu_fwd', lambda: dict(u=z((5, 16), BF16)), lambda u: ops.swiglu_fwd(u))
case('swiglu_bwd', lambda: dict(dout=z((5, 8), BF16), u=z((5, 16), BF16)), lambda dout, u: ops.swiglu_bwd(dout, u))
case('act_fwd', lambda: dict(u=z((5, 16), BF16)), lambda u: ops.act_fwd(u, 'silu'))
case('act_fwd:relu_sq', lambda: dict(u=z((5, 16), BF16)), lambda u: ops.act_fwd(u, 'relu_sq'))
case('act_fwd:bad-kind', lambda: dict(u=z((5, 16), BF16)), lambda u: ops.act_fwd(u, 'gelu'))
case('act_bwd', lambda: dict(dout=z((5, 16), BF16), u=z((5, 16), BF16)), lambda dout, u: ops.act_bwd(dout, u, 'relu_sq'))
case('reserve-and-env', dict, lambda: (ops.set_cu_reserve(5), ops.cu_reserve(), ops.reload_env(), ops.set_cu_reserve(0), ops.cu_reserve()))
case('gemm_nt', lambda: dict(A=z((24, 32), BF16), B=z((16, 32), BF16)), lambda A, B: ops.gemm_nt(A, B))
case('gemm_nt:strided-out-alpha', lambda: dict(A=z((24, 32), BF16, ld=40), B=z((16, 32), BF16, ld=48), out=z((24, 16), BF16, ld=24),
                                               alpha=z((), F32)),
     lambda A, B, out, alpha: ops.gemm_nt(A, B, out=out, alpha=alpha))
case('gemm_nt:f32-acc', lambda: dict(A=z((24, 32), BF16), B=z((16, 32), BF16), out=z((24, 16), F32)),
     lambda A, B, out: ops.gemm_nt(A, B, out=out, accumulate=True))
case('gemm_nt:out_dtype', lambda: dict(A=z((24, 32), BF16), B=z((16, 32), BF16)), lambda A, B: ops.gemm_nt(A, B, out_dtype=F32))
case('gemm_nt:variant', lambda: dict(A=z((24, 32), BF16), B=z((16, 32), BF16)), lambda A, B: ops.gemm_nt(A, B, variant=3))
case('gemm_nt:no-workspace', lambda: dict(A=z((4, 32), BF16), B=z((16, 32), BF16)), lambda A, B: ops.gemm_nt(A, B))
case('gemm_nt:k-differs', lambda: dict(A=z((24, 32), BF16), B=z((16, 31), BF16)), lambda A, B: ops.gemm_nt(A, B))
case('gemm_tn', lambda: dict(A=z((32, 24), BF16), B=z((32, 16), BF16)), lambda A, B: ops.gemm_tn(A, B))
case('gemm_tn:out-acc-alpha', lambda: dict(A=z((32, 24), BF16, ld=40), B=z((32, 16), BF16), out=z((24, 16), F32, ld=24), alpha=z((), F32)),
     lambda A, B, out, alpha: ops.gemm_tn(A, B, out=out, accumulate=True, alpha=alpha))
case('gemm_tn:acc-without-out', lambda: dict(A=z((32, 24), BF16), B=z((32, 16), BF16)), lambda A, B: ops.gemm_tn(A, B, accumulate=True))
case('gemm_tn:no-workspace', lambda: dict(A=z((8, 24), BF16), B=z((8, 16), BF16)), lambda A, B: ops.gemm_tn(A, B))
case('gemm_tn:k-differs', lambda: dict(A=z((32, 24), BF16), B=z((31, 16), BF16)), lambda A, B: ops.gemm_tn(A, B))


def grouped(K=32, K2=None):
  return lambda: dict(A=z((K, 24), BF16), B=z((K, 16), BF16), out=z((24, 16), F32), A2=z((K2 or K, 8), BF16, ld=16), B2=z((K2 or K, 12), BF16),
                      out2=z((8, 12), F32, ld=16), alpha=z((), F32))


def call_grouped(A, B, out, A2, B2, out2, alpha):
  return ops.gemm_tn_grouped([(A, B, out, False, None), (A2, B2, out2, True, alpha)])


case('gemm_tn_grouped', grouped(), call_grouped)
case('gemm_tn_grouped:refused-by-the-library', grouped(K=31), call_grouped, mutate=False)
case('gemm_tn_grouped:k-differs', grouped(K2=30), call_grouped, mutate=False)
case('gemm_tn_grouped:none', dict, lambda: ops.gemm_tn_grouped([]))
case('gemm_tn_grouped:oversize', lambda: dict(A=z((32, 24), BF16), B=z((32, 16), BF16), out=z((24, 16), F32)),
     lambda A, B, out: ops.gemm_tn_grouped([(A, B, out, False, None)] * (ops.TN_GROUP_MAX + 1)), mutate=False)
case('fc1_swiglu', lambda: dict(x=z((5, 32), BF16), w=z((16, 32), BF16)), lambda x, w: ops.fc1_swiglu(x, w))
case('fc1_swiglu:odd-h', lambda: dict(x=z((5, 32), BF16), w=z((24, 32), BF16)), lambda x, w: ops.fc1_swiglu(x, w))
case('fc2_dx_swiglu_bwd', lambda: dict(dy=z((5, 32), BF16), w2t=z((8, 32), BF16), u=z((5, 16), BF16)),
     lambda dy, w2t, u: ops.fc2_dx_swiglu_bwd(dy, w2t, u))
case('fc2_dx_swiglu_bwd:retry', lambda: dict(dy=z((5, 32), BF16), w2t=z((8, 32), BF16), u=z((5, 16), BF16)),
     lambda dy, w2t, u: ops.fc2_dx_swiglu_bwd(dy, w2t, u), fc2_refusals=1, mutate=False)
case('fc2_dx_swiglu_bwd:refused-twice', lambda: dict(dy=z((5, 32), BF16), w2t=z((8, 32), BF16), u=z((5, 16), BF16)),
     lambda dy, w2t, u: ops.fc2_dx_swiglu_bwd(dy, w2t, u), fc2_refusals=2, mutate=False)
case('rope_qk_', lambda: dict(qkv=z((B_ * T_, 3 * DM), BF16), **rope()),
     lambda qkv, rope_cos, rope_sin: ops.rope_qk_(qkv, rope_cos, rope_sin, B_, T_, NH))
case('rope_qk_:short-table', lambda: dict(qkv=z((B_ * T_, 3 * DM), BF16), **rope()),
     lambda qkv, rope_cos, rope_sin: ops.rope_qk_(qkv, rope_cos, rope_sin, B_, T_ + 1, NH), mutate=False)
case('qkv_rope', lambda: dict(x=z((B_ * T_, 32), BF16), w=z((3 * DM, 32), BF16), **rope()),
     lambda x, w, rope_cos, rope_sin: ops.qkv_rope(x, w, rope_cos, rope_sin, B_, T_, NH))
case('doc_start_from_mask', lambda: dict(mask=z((B_, T_, T_), torch.bool)), lambda mask: ops.doc_start_from_mask(mask))
case('attn_doc_plan', lambda: dict(doc_start=z((B_, T_), I32)), lambda doc_start: ops.attn_doc_plan(doc_start, NH))
case('attn_flops', dict, lambda: ops.attn_flops(B_, T_, NH, HD))
case('attn_fwd', lambda: dict(qkv=z((B_ * T_, 3 * DM), BF16)), lambda qkv: ops.attn_fwd(qkv, B_, T_, NH))
case('attn_fwd:doc', lambda: dict(qkv=z((B_ * T_, 3 * DM), BF16), doc_start=z((B_, T_), I32)),
     lambda qkv, doc_start: ops.attn_fwd(qkv, B_, T_, NH, doc_start=doc_start))
case('attn_fwd:doc-plan', lambda: dict(qkv=z((B_ * T_, 3 * DM), BF16), doc_start=z((B_, T_), I32), plan=z((64,), I32)),
     lambda qkv, doc_start, plan: ops.attn_fwd(qkv, B_, T_, NH, doc_start=doc_start, plan=plan))
case('attn_bwd', attn_saved, lambda qkv, out, dout, lse, rope_cos, rope_sin: ops.attn_bwd(qkv, out, dout, lse, rope_cos, rope_sin, B_, T_, NH))
case('attn_bwd:doc-delta', lambda: dict(doc_start=z((B_, T_), I32), **attn_saved()),
     lambda doc_start, qkv, out, dout, lse, rope_cos, rope_sin: ops.attn_bwd(qkv, out, dout, lse, rope_cos, rope_sin, B_, T_, NH,
                                                                            doc_start=doc_start, return_delta=True))
case('attn_bwd:doc-plan', lambda: dict(doc_start=z((B_, T_), I32), plan=z((64,), I32), **attn_saved()),
     lambda doc_start, plan, qkv, out, dout, lse, rope_cos, rope_sin: ops.attn_bwd(qkv, out, dout, lse, rope_cos, rope_sin, B_, T_, NH,
                                                                                  doc_start=doc_start, plan=plan))
case('attn_bwd:delta-hd128', lambda: dict(qkv=z((B_ * T_, 3 * 128), BF16), out=z((B_ * T_, 128), BF16), dout=z((B_ * T_, 128), BF16),
                                          lse=z((B_, 1, T_), F32), rope_cos=z((T_, 64), F32), rope_sin=z((T_, 64), F32)),
     lambda qkv, out, dout, lse, rope_cos, rope_sin: ops.attn_bwd(qkv, out, dout, lse, rope_cos, rope_sin, B_, T_, 1, return_delta=True))
case('attn_mask_pack', lambda: dict(mask=z((B_, T_, T_), torch.bool)), lambda mask: ops.attn_mask_pack(mask))
case('attn_mask_pack:2d', lambda: dict(mask=z((T_, T_), torch.bool)), lambda mask: ops.attn_mask_pack(mask))
case('attn_mask_pack:T-not-4', lambda: dict(mask=z((6, 6), torch.bool)), lambda mask: ops.attn_mask_pack(mask))
case('attn_mask_pack:not-square', lambda: dict(mask=z((B_, T_, 4), torch.bool)), lambda mask: ops.attn_mask_pack(mask))
case('attn_mask_pack:not-a-tensor', dict, lambda: ops.attn_mask_pack([[True]]))
case('attn_fwd_masked', lambda: dict(qkv=z((B_ * T_, 3 * DM), BF16), **packed_mask()),
     lambda qkv, bits, tile_class: ops.attn_fwd_masked(qkv, bits, tile_class, B_, T_, NH))
case('attn_fwd_masked:shared-mask', lambda: dict(qkv=z((B_ * T_, 3 * DM), BF16), bits=z((1, T_, 1), I64), tile_class=z((1, 1, 1), U8)),
     lambda qkv, bits, tile_class: ops.attn_fwd_masked(qkv, bits, tile_class, B_, T_, NH))
case('attn_bwd_masked', lambda: dict(**attn_saved(), **packed_mask()),
     lambda qkv, out, dout, lse, rope_cos, rope_sin, bits, tile_class: ops.attn_bwd_masked(qkv, out, dout, lse, rope_cos, rope_sin, bits,
                                                                                          tile_class, B_, T_, NH))
case('attn_bwd_masked:delta', lambda: dict(**attn_saved(), **packed_mask()),
     lambda qkv, out, dout, lse, rope_cos, rope_sin, bits, tile_class: ops.attn_bwd_masked(qkv, out, dout, lse, rope_cos, rope_sin, bits,
                                                                                          tile_class, B_, T_, NH, return_delta=True),
     mutate=False)


def cached(rows, width, lens='lens', ld=None, **more):
  return lambda: dict(**{'qkv' if width == 3 else 'q': z((rows, width * DM), BF16, ld=ld), 'kv': z((B_, TMAX, 2 * DM), BF16),
                         lens: z((B_,), I32)}, **more)


case('kv_append_rope', lambda: dict(**cached(B_, 3, 'pos', ld=3 * DM + 8)(), **rope()),
     lambda qkv, kv, pos, rope_cos, rope_sin: ops.kv_append_rope(qkv, pos, rope_cos, rope_sin, kv, NH))
case('kv_append_rope:outputs', lambda: dict(**cached(B_, 3, 'pos')(), **rope(), q_out=z((B_, DM), BF16), status=z((1,), I32)),
     lambda qkv, kv, pos, rope_cos, rope_sin, q_out, status: ops.kv_append_rope(qkv, pos, rope_cos, rope_sin, kv, NH, q_out=q_out,
                                                                               status=status))
case('attn_decode_workspace', dict, lambda: ops.attn_decode_workspace(B_, NH, HD, TMAX, 0, 'cpu'))
case('attn_decode_workspace:refused', dict, lambda: ops.attn_decode_workspace(B_, NH, 48, TMAX, 0, 'cpu'))
case('attn_decode', cached(B_, 1), lambda q, kv, lens: ops.attn_decode(q, kv, lens, NH))
case('attn_decode:splits-lse', cached(B_, 1), lambda q, kv, lens: ops.attn_decode(q, kv, lens, NH, splits=4, want_lse=True), mutate=False)
case('attn_decode:bad-splits', cached(B_, 1), lambda q, kv, lens: ops.attn_decode(q, kv, lens, NH, splits=65), mutate=False)
case('attn_decode:workspace', cached(B_, 1, ws=z((4096,), U8)),
     lambda q, kv, lens, ws: ops.attn_decode(q, kv, lens, NH, workspace=(ws, 4000)), mutate=False)
case('attn_decode:padded-cache', lambda: dict(q=z((B_, DM), BF16), kv=gpu(torch.zeros((B_, TMAX, 2 * DM + 8), dtype=BF16))[:, :, :2 * DM],
                                              lens=z((B_,), I32)),
     lambda q, kv, lens: ops.attn_decode(q, kv, lens, NH), mutate=False)
case('kv_append_rope_rows', lambda: dict(**cached(B_ * NCH, 3, 'lens0')(), **rope()),
     lambda qkv, kv, lens0, rope_cos, rope_sin: ops.kv_append_rope_rows(qkv, lens0, rope_cos, rope_sin, kv, NH))
case('kv_append_rope_rows:n_new-outputs', lambda: dict(**cached(B_ * NCH, 3, 'lens0', ld=3 * DM + 8)(), **rope(), n_new=z((B_,), I32),
                                                       q_out=z((B_ * NCH, DM), BF16), status=z((1,), I32)),
     lambda qkv, kv, lens0, rope_cos, rope_sin, n_new, q_out, status: ops.kv_append_rope_rows(qkv, lens0, rope_cos, rope_sin, kv, NH,
                                                                                             n_new=n_new, q_out=q_out, status=status))
case('kv_append_rope_rows:ragged', lambda: dict(**cached(B_ * NCH + 1, 3, 'lens0')(), **rope()),
     lambda qkv, kv, lens0, rope_cos, rope_sin: ops.kv_append_rope_rows(qkv, lens0, rope_cos, rope_sin, kv, NH), mutate=False)
case('attn_extend_workspace', dict, lambda: ops.attn_extend_workspace(B_, NCH, NH, HD, TMAX, 2, 'cpu'))
case('attn_extend_workspace:refused', dict, lambda: ops.attn_extend_workspace(B_, 0, NH, HD, TMAX, 0, 'cpu'))
case('attn_extend', cached(B_ * NCH, 1, 'lens0'), lambda q, kv, lens0: ops.attn_extend(q, kv, lens0, NH))
case('attn_extend:n_new-splits-lse', cached(B_ * NCH, 1, 'lens0', n_new=z((B_,), I32)),
     lambda q, kv, lens0, n_new: ops.attn_extend(q, kv, lens0, NH, n_new=n_new, splits=2, want_lse=True))
case('attn_extend:workspace', cached(B_ * NCH, 1, 'lens0', ws=z((8192,), U8)),
     lambda q, kv, lens0, ws: ops.attn_extend(q, kv, lens0, NH, workspace=(ws, 8000)), mutate=False)
case('attn_extend:bad-splits', cached(B_ * NCH, 1, 'lens0'), lambda q, kv, lens0: ops.attn_extend(q, kv, lens0, NH, splits=-1), mutate=False)
case('sample_logits', lambda: dict(logits=z((3, 50), BF16, ld=56), u=z((3,), F32)), lambda logits, u: ops.sample_logits(logits, u))
case('sample_logits:stats', lambda: dict(logits=z((1, 50), BF16), u=z((1,), F32)),
     lambda logits, u: ops.sample_logits(logits, u, temperature=0.7, top_k=5, top_p=0.9, want_stats=True), mutate=False)


def spec(k=2, B=2, V=50):
  return lambda: dict(target_logits=z((B * (k + 1), V), BF16, ld=V + 6), draft_logits=z((k * B, V), BF16), draft_tokens=z((k, B), I64),
                      target_cutoff=z((B * (k + 1),), F32), draft_cutoff=z((k * B,), F32), target_tokens=z((B * (k + 1),), I64),
                      u_accept=z((k, B), F32), u_resid=z((B,), F32))


case('spec_verify', spec(), lambda **kw: ops.spec_verify(temperature=0.5, **kw))
case('ce_fwd_bwd_', lambda: dict(logits=z((5, 56), BF16), targets=z((5,), I64)), lambda logits, targets: ops.ce_fwd_bwd_(logits, targets, 0.2))
case('ce_fwd_bwd_:V', lambda: dict(logits=z((5, 56), BF16), targets=z((5,), I64)),
     lambda logits, targets: ops.ce_fwd_bwd_(logits, targets, 0.2, V=50), mutate=False)
case('head_score', lambda: dict(y=z((5, 32), BF16, ld=40), w=z((50, 32), BF16), targets=z((5,), I64)),
     lambda y, w, targets: ops.head_score(y, w, targets))
case('head_score:lse', lambda: dict(y=z((5, 32), BF16), w=z((50, 32), BF16, ld=48), targets=z((5,), I64)),
     lambda y, w, targets: ops.head_score(y, w, targets, want_lse=True), mutate=False)
case('head_score:no-workspace', lambda: dict(y=z((1, 32), BF16), w=z((50, 32), BF16), targets=z((1,), I64)),
     lambda y, w, targets: ops.head_score(y, w, targets), mutate=False)
case('head_predict', lambda: dict(y=z((5, 32), BF16, ld=40), w=z((50, 32), BF16)), lambda y, w: ops.head_predict(y, w))
case('head_predict:targets-lse', lambda: dict(y=z((5, 32), BF16), w=z((50, 32), BF16, ld=48), targets=z((5,), I64)),
     lambda y, w, targets: ops.head_predict(y, w, targets=targets, want_entropy=False, want_lse=True))
case('head_predict:no-workspace', lambda: dict(y=z((1, 32), BF16), w=z((50, 32), BF16)), lambda y, w: ops.head_predict(y, w), mutate=False)
case('mean', lambda: dict(x=z((5, 7), F32)), lambda x: ops.mean(x))
case('scale_bf16_', lambda: dict(x=z((5, 7), BF16), alpha=z((), F32)), lambda x, alpha: ops.scale_bf16_(x, alpha))
case('axpy_f32_', lambda: dict(out=z((35,), F32), x=z((5, 7), F32)), lambda out, x: ops.axpy_f32_(out, x))
case('axpy_f32_:alpha-store', lambda: dict(out=z((35,), F32), x=z((35,), F32), alpha=z((), F32)),
     lambda out, x, alpha: ops.axpy_f32_(out, x, alpha=alpha, accumulate=False))
case('sumsq', lambda: dict(x=z((35,), F32)), lambda x: ops.sumsq(x))
case('sumsq:scratch', lambda: dict(x=z((35,), F32), scratch=z((4096,), F32)), lambda x, scratch: ops.sumsq(x, scratch=scratch), mutate=False)


def hparams(kind):
  return ops.optim_hparams(kind, 0.25, weight_decay=0.5, first=True, beta1=0.5, beta2=0.75, eps=0.125, momentum=0.5, dampening=0.25, bc2=0.5,
                           coef_grad=0.25, coef_avg=0.5, ckp1=0.25, bc1=0.5)


case('optim_', lambda: dict(p=z((35,), F32), g=z((35,), F32), m=z((35,), F32), v=z((35,), F32), clip=z((), F32)),
     lambda p, g, m, v, clip: ops.optim_(hparams('adamw'), p, g, m, v, clip_coef=clip))
case('optim_:sgd', lambda: dict(p=z((35,), F32), g=z((35,), F32)), lambda p, g: ops.optim_(hparams('sgd'), p, g, None, None), mutate=False)


def optim_items():
  return dict(p=z((5, 7), F32), g=z((5, 7), F32), m=z((5, 7), F32), v=z((5, 7), F32), dst=z((5, 7), BF16), dst_t=z((7, 5), BF16, ld=8),
              p2=z((3, 4), F32), g2=z((3, 4), F32), dst2=z((3, 4), BF16), dst_t2=z((4, 3), BF16))


def call_optim_cast(p, g, m, v, dst, dst_t, p2, g2, dst2, dst_t2):
  table = ops.optim_cast_multi_(hparams('sfo_adamw'), [(p, g, m, v, dst, dst_t), (p2, g2, None, None, dst2, dst_t2)])
  return table, ops.optim_cast_multi_(hparams(ops._lib.OPTIM_NADAMW), None, clip_coef=g2, table=table)


case('optim_cast_multi_', optim_items, call_optim_cast)
case('lerp_', lambda: dict(p=z((35,), F32), z=z((35,), F32)), lambda p, z: ops.lerp_(p, z, 0.25))  # noqa: F811

RESERVE_CASES = ('gemm_nt', 'gemm_tn', 'gemm_tn_grouped', 'head_score', 'head_predict', 'gemm_mx_nt', 'fc1_swiglu', 'attn_fwd')
# the hook-reserve runs of the cached size queries use shapes of their own: the parent's head caches are not keyed by the reserve
RESERVE_SHAPES = {
  'gemm_nt': lambda: dict(A=z((40, 32), BF16), B=z((16, 32), BF16)),
  'head_score': lambda: dict(y=z((6, 32), BF16), w=z((50, 32), BF16), targets=z((6,), I64)),
  'head_predict': lambda: dict(y=z((6, 32), BF16), w=z((50, 32), BF16)),
}


def mutations(t):
  """(tag, the tensor changed in one respect) for every mutation that applies to t."""
  other = {BF16: F32, F32: BF16, I64: I32, I32: I64, U8: torch.int8, torch.bool: U8}[t.dtype]
  plain = t.as_subclass(torch.Tensor)
  yield 'dtype', gpu(plain.to(other))
  yield 'rank', gpu(plain.unsqueeze(0))
  yield 'cpu', plain
  if t.dim() >= 1:
    last = t.shape[-1]
    yield 'inner', gpu(torch.zeros(tuple(t.shape[:-1]) + (2 * last,), dtype=t.dtype))[..., ::2]
    if t.shape[0] > 1:
      yield 'short', gpu(plain[:-1])
  if t.dim() >= 2:
    yield 'rows', gpu(torch.zeros(tuple(t.shape[:-1]) + (last + 8,), dtype=t.dtype))[..., :last]
    yield 'narrow', gpu(torch.zeros(tuple(t.shape[:-1]) + (last - 1,), dtype=t.dtype))


def run(call, operands, fc2_refusals=0, instrumented=False, reserve_hook=False):
  """One call against a fresh recorder: {'raised', 'launches'} or {'calls', 'ret'} (+ 'profile' when instrumented)."""
  rec = Recorder()
  rec.fc2_refusals = fc2_refusals
  for name, t in operands.items():
    if isinstance(t, ops.MxTensor):
      rec.operand(name + '.data', t.data)
      rec.operand(name + '.scales', t.scales)
    else:
      rec.operand(name, t)
  with faked(rec):
    if instrumented or reserve_hook:
      fired = []

      def hook(family, work):
        rec.entries.append(['hook', family, work])
        if reserve_hook and not fired:
          ops.set_cu_reserve(3)
        fired.append(family)
      ops.LAUNCH_HOOK = hook
    if instrumented:
      ops.PROFILE = []
    try:
      result = call(**operands)
    except Exception as e:  # noqa: BLE001 - the type is what is recorded
      return {'raised': [type(e).__name__, str(e)], 'launches': rec.launches()}
    calls, ret = rec.finish(result)
    out = {'calls': calls, 'ret': ret}
    if instrumented:
      out['profile'] = [[fam, work] for fam, work, _, _ in ops.PROFILE]
  return out


def scenario(operands, call, opts, **how):
  return run(call, operands(), fc2_refusals=opts.get('fc2_refusals', 0), **how)


def record_all():
  out = {}
  for name, (operands, call, opts) in CASES.items():
    plain = scenario(operands, call, opts)
    if 'raised' not in plain:
      inst = scenario(operands, call, opts, instrumented=True)
      plain['inst'] = [e if e[0] in ('hook', 'event', 'attn_flops') else e[0] for e in inst['calls']]
      plain['profile'] = inst['profile']
      if [e for e in inst['calls'] if e[0].startswith('plm_')] != [e for e in plain['calls'] if e[0].startswith('plm_')] or inst['ret'] != plain['ret']:
        plain['inst_calls'], plain['inst_ret'] = inst['calls'], inst['ret']
    out[name] = plain
    if ':' in name and name.split(':')[0] in CASES:
      skip = set(CASES[name.split(':')[0]][0]())
    else:
      skip = set()
    if not opts.get('mutate', True):
      continue
    for arg in operands():
      if arg in skip:
        continue
      base = operands()
      ts = [('', base[arg])] if isinstance(base[arg], torch.Tensor) else [('.data', base[arg].data), ('.scales', base[arg].scales)]
      for part, t in ts:
        for tag, changed in mutations(t):
          ops_ = operands()
          if part:
            setattr(ops_[arg], part[1:], changed)
          else:
            ops_[arg] = changed
          out[f'{name}/{arg}{part}/{tag}'] = run(call, ops_, fc2_refusals=opts.get('fc2_refusals', 0))
  for name in RESERVE_CASES:
    operands, call, opts = CASES[name]
    out[f'hook-reserve/{name}'] = run(call, RESERVE_SHAPES.get(name, operands)(), reserve_hook=True)
  return json.loads(json.dumps(out))  # tuples -> lists: exactly what the file holds


def main():
  out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'ops_trace_parent.json')
  scenarios = record_all()
  with open(out, 'w') as f:
    json.dump({'commit': '2afedcd', 'scenarios': scenarios}, f, separators=(',', ':'))
    f.write('\n')
  refused = sum('raised' in s for s in scenarios.values())
  print(f'{out}: {len(scenarios)} scenarios, {refused} refusals, {os.path.getsize(out)} bytes')


if __name__ == '__main__':
  main()
