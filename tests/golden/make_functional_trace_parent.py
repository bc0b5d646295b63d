"""The ops calls of the block-linear autograd Functions BEFORE the bf16 / mxfp8 pairs of plainlm_amd/functional.py became one family
(commit c4c2987), recorded for tests/test_functional_trace_host.py, which replays the same scenarios on the working tree and requires
equal traces.  Equal traces mean: the same kernels in the same order with operands of the same dtype, shape and strides and the same
scalars, the same calls skipped when an input needs no gradient, the same tensors kept alive between forward and backward, and the
same weight gradients entering the GradSink's queue in the same order and leaving it in the same launches.

Nothing runs on a GPU and the library is not loaded: every ops function these Functions reach is replaced by a fake on CPU tensors that
appends one entry [name, signature of every argument ...] and returns zeros of the right shape and dtype (mx_quant: ops.MxTensor.empty).
Signatures: a tensor is 'dtype[shape]s[strides]' (+ '@name' for a weight or its main_grad), an MxTensor 'mx[rows,K]', scalars and keywords
as given.  Around the ops entries a pass records
  'saved':  the signature of every tensor a forward packs (torch.autograd.graph.saved_tensors_hooks),
  'alive':  which tensors RETURNED by the fakes during forward still exist after it ('<entry index>:<op>.<output index>'; the module's
            own output is held by the caller and so listed) - this is what sees the MX copies a Function keeps as plain attributes, and
            that the row-blocked copies and the bf16 activation of the MX path are dropped,
  'grads':  the signatures of x.grad and of every weight's .grad after backward (None: went to the sink, or not needed),
and a GradSink in use adds the entries ['defer_dw', dy, x, weight name] and ['flush', bytes queued, [[weight name, accumulate] ...]].

Only names that exist on both sides of the change are used (the modules of transformer.py, GradSink, ops), so this one file runs on
the parent and on the working tree alike.

functional_trace_parent.json: {'commit', 'scenarios': {name: {'modules': {...}, 'passes': [{'ops', 'saved', 'alive', 'grads'} ...]}}}

Run from a checkout of commit c4c2987 (no GPU, no built library needed):
  python tests/golden/make_functional_trace_parent.py [output .json]
"""
import contextlib
import json
import os
import sys
import weakref

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

D, HIDDEN, M, HEADS, B, T = 64, 128, 24, 2, 2, 12  # M = B * T = 24 rows: ragged against every tile size
PRECISIONS = ('bf16', 'mxfp8')
MODULES = ('linear', 'attention', 'glu', 'mlp', 'mlp_relu_sq')
GRAD_PATTERNS = ('all', 'no_x', 'no_w')


class Recorder:
  """The fakes and what they recorded."""

  def __init__(self, torch, ops):
    self.torch, self.ops = torch, ops
    self.entries, self.outputs, self.names = [], [], {}
    self.group_ok = True  # gemm_tn_grouped's answer

  def name(self, t, name):
    self.names[t.data_ptr()] = name

  def sig(self, v):
    torch = self.torch
    if isinstance(v, torch.Tensor):
      s = f'{str(v.dtype)[6:]}{list(v.shape)}s{list(v.stride())}'
      return s + '@' + self.names[v.data_ptr()] if v.data_ptr() in self.names else s
    if isinstance(v, self.ops.MxTensor):
      return f'mx{list(v.shape)}'
    if isinstance(v, (list, tuple)):
      return [self.sig(e) for e in v]
    if v is None or isinstance(v, (bool, int, float, str)):
      return v
    if isinstance(v, torch.dtype):
      return str(v)
    return type(v).__name__

  def call(self, op, args, kwargs, outs):
    self.entries.append([op] + [self.sig(a) for a in args] + [{k: self.sig(v) for k, v in kwargs.items()}] * bool(kwargs))
    for j, o in enumerate(outs):
      t = o.data if isinstance(o, self.ops.MxTensor) else o
      self.outputs.append((f'{len(self.entries) - 1}:{op}.{j}', weakref.ref(t)))

  def alive(self):  # reference counts decide (nothing here sits in a cycle): no collection needed
    return [label for label, ref in self.outputs if ref() is not None]

  def take(self):
    e, self.entries, self.outputs = self.entries, [], []
    return e

  def fakes(self):
    torch, ops, rec = self.torch, self.ops, self
    bf16, f32 = torch.bfloat16, torch.float32

    def zeros(shape, dtype):
      return torch.zeros(tuple(shape), dtype=dtype)

    def cast_bf16_t(src, out=None, out_t=None):
      out = zeros(src.shape, bf16) if out is None else out
      out_t = zeros((src.shape[1], src.shape[0]), bf16) if out_t is None else out_t
      rec.call('cast_bf16_t', (src,), dict(out=out, out_t=out_t), ())
      return out, out_t

    def gemm_nt(A, Bm, *args, **kw):
      names = ('out', 'out_dtype', 'accumulate', 'alpha', 'variant')
      full = dict(zip(names, args), **kw)
      out = full.get('out')
      made = out is None
      if made:
        out = zeros((A.shape[0], Bm.shape[0]), full.get('out_dtype', bf16))
      rec.call('gemm_nt', (A, Bm) + args, kw, (out,) if made else ())
      return out

    def gemm_tn(A, Bm, *args, **kw):
      full = dict(zip(('out', 'accumulate', 'alpha'), args), **kw)
      out = full.get('out')
      made = out is None
      if made:
        out = zeros((A.shape[1], Bm.shape[1]), f32)
      rec.call('gemm_tn', (A, Bm) + args, kw, (out,) if made else ())
      return out

    def gemm_tn_grouped(problems):
      rec.call('gemm_tn_grouped', (problems,), {}, ())
      return rec.group_ok

    def gemm_mx_nt(a, b, *args, **kw):
      full = dict(zip(('out', 'accumulate', 'out_dtype'), args), **kw)
      out = full.get('out')
      made = out is None
      if made:
        out = zeros((a.shape[0], b.shape[0]), full.get('out_dtype', bf16))
      rec.call('gemm_mx_nt', (a, b) + args, kw, (out,) if made else ())
      return out

    def mx_quant(x, *args, **kw):
      full = dict(zip(('rows', 'cols'), args), **kw)
      R, Cc = x.shape
      r = ops.MxTensor.empty(R, Cc, x.device) if full.get('rows', True) else None
      c = ops.MxTensor.empty(Cc, R, x.device) if full.get('cols', True) else None
      rec.call('mx_quant', (x,) + args, kw, [o for o in (r, c) if o is not None])
      return r, c

    def fc1_swiglu(x, w):
      u, act = zeros((x.shape[0], w.shape[0]), bf16), zeros((x.shape[0], w.shape[0] // 2), bf16)
      rec.call('fc1_swiglu', (x, w), {}, (u, act))
      return u, act

    def fc2_dx_swiglu_bwd(dy, w2t, u):
      du = zeros(u.shape, bf16)
      rec.call('fc2_dx_swiglu_bwd', (dy, w2t, u), {}, (du,))
      return du

    def swiglu_fwd(u):
      out = zeros((u.shape[0], u.shape[1] // 2), bf16)
      rec.call('swiglu_fwd', (u,), {}, (out,))
      return out

    def swiglu_bwd(dout, u):
      du = zeros(u.shape, bf16)
      rec.call('swiglu_bwd', (dout, u), {}, (du,))
      return du

    def act_fwd(u, *args, **kw):
      out = zeros(u.shape, bf16)
      rec.call('act_fwd', (u,) + args, kw, (out,))
      return out

    def act_bwd(dout, u, *args, **kw):
      du = zeros(u.shape, bf16)
      rec.call('act_bwd', (dout, u) + args, kw, (du,))
      return du

    def qkv_rope(x, w, *args, **kw):
      out = zeros((x.shape[0], w.shape[0]), bf16)
      rec.call('qkv_rope', (x, w) + args, kw, (out,))
      return out

    def rope_qk_(qkv, *args, **kw):
      rec.call('rope_qk_', (qkv,) + args, kw, ())
      return qkv

    # not block-linear ops: Attention.forward is the one public way to QKVRopeFn that both sides share, and it goes on through AttnFn
    def attn_fwd(qkv, Bn, Tn, nh, *args, **kw):
      out, lse = zeros((Bn * Tn, qkv.shape[1] // 3), bf16), zeros((Bn, nh, Tn), f32)
      rec.call('attn_fwd', (qkv, Bn, Tn, nh) + args, kw, (out, lse))
      return out, lse

    def attn_bwd(qkv, *args, **kw):
      dqkv = zeros(qkv.shape, bf16)
      rec.call('attn_bwd', (qkv,) + args, kw, (dqkv,))
      return dqkv

    return {f.__name__: f for f in (cast_bf16_t, gemm_nt, gemm_tn, gemm_tn_grouped, gemm_mx_nt, mx_quant, fc1_swiglu, fc2_dx_swiglu_bwd,
                                    swiglu_fwd, swiglu_bwd, act_fwd, act_bwd, qkv_rope, rope_qk_, attn_fwd, attn_bwd)}

  @contextlib.contextmanager
  def patched(self):
    fakes = self.fakes()
    saved = {k: getattr(self.ops, k) for k in fakes}
    for k, f in fakes.items():
      setattr(self.ops, k, f)
    try:
      yield self
    finally:
      for k, f in saved.items():
        setattr(self.ops, k, f)


def linears_of(torch, mod):
  from plainlm_amd.transformer import HipLinear
  return [(n or 'lin', m) for n, m in mod.named_modules() if isinstance(m, HipLinear)]


def prepare(torch, rec, mods, precision, sink):
  """Zero weights (their values never matter), precision and sink wired as Transformer does; the names the signatures use."""
  for tag, mod in mods:
    for n, lin in linears_of(torch, mod):
      with torch.no_grad():
        lin.weight.zero_()
      lin.mx = precision == 'mxfp8'
      rec.name(lin.weight, f'{tag}.{n}.w')
      if sink is not None:
        lin.sink = sink
        lin.weight.main_grad = torch.zeros_like(lin.weight)
        rec.name(lin.weight.main_grad, f'{tag}.{n}.g')


def traced_sink(rec, Fn):
  """A real GradSink whose defer_dw calls and flushes are recorded in line with the ops entries."""
  sink = Fn.GradSink()
  sink.enabled = True
  defer, flush = sink.defer_dw, sink._flush_linear_dw

  def pname(p):
    return rec.names.get(p.data_ptr(), '?')

  def defer_dw(dy, x, p):
    rec.entries.append(['defer_dw', rec.sig(dy), rec.sig(x), pname(p)])
    return defer(dy, x, p)

  def _flush_linear_dw():
    if sink.dw_queue:
      rec.entries.append(['flush', sink.dw_queue_bytes, [[pname(p), acc] for _, _, p, acc in sink.dw_queue]])
    return flush()
  sink.defer_dw, sink._flush_linear_dw = defer_dw, _flush_linear_dw
  return sink


def one_pass(torch, rec, run, x_grad, mods, sink):
  """Forward + backward (+ the sink's final flush, as the embedding's backward does): what the fakes, the hooks and the sink saw."""
  x = torch.zeros((M, D), dtype=torch.bfloat16, requires_grad=x_grad)
  saved = []

  def pack(t):
    saved.append(rec.sig(t))
    return t
  with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
    y = run(x)
  alive = rec.alive()
  if y.requires_grad:
    y.backward(torch.ones_like(y))
  if sink is not None:
    sink.flush_dw()
  grads = {'x': rec.sig(x.grad)}
  for tag, mod in mods:
    for n, lin in linears_of(torch, mod):
      grads[f'{tag}.{n}'] = rec.sig(lin.weight.grad)
      lin.weight.grad = None
  del y
  return {'ops': rec.take(), 'saved': saved, 'alive': alive, 'grads': grads}


def build(torch, kind):
  """(module, run(x)) of one module scenario."""
  from plainlm_amd import transformer as Tr
  if kind == 'linear':
    mod = Tr.HipLinear(D, D)
    return mod, mod
  if kind == 'attention':
    cfg = Tr.ModelConfig(vocab_size=64, seq_len=T, dim=D, expand=2.0, n_layers=1, n_heads=HEADS)
    mod = Tr.Attention(cfg)
    rope = Tr.rope_tables(D // HEADS, T)
    return mod, lambda x: mod(x, rope, None, B, T)
  mod = Tr.MLP_CLASSES[kind](dim=D, hidden_dim=HIDDEN - 28, multiple_of=HIDDEN)  # 100 rounds up to 128
  return mod, mod.apply_fn


def describe(mod, attrs=()):
  out = {'class': type(mod).__name__, 'state_dict': {k: list(v.shape) for k, v in mod.state_dict().items()}}
  out.update({a: getattr(mod, a) for a in attrs})
  return out


MODULE_ATTRS = {'glu': ('hidden_dim',), 'mlp': ('hidden_dim', 'kind'), 'mlp_relu_sq': ('hidden_dim', 'kind')}  # what other code reads


def module_scenario(torch, Fn, ops, kind, precision, with_sink, pattern):
  """Three passes through one module: fresh weights (the shadows are cast, the MX copies quantized), again without a weight change (no
  cast and no quantize call may appear; with a sink the window goes on, so the gradients accumulate), and after invalidate() in a new
  window (the calls reappear)."""
  rec = Recorder(torch, ops)
  with rec.patched():
    sink = traced_sink(rec, Fn) if with_sink else None
    mod, run = build(torch, kind)
    mods = [(kind, mod)]
    prepare(torch, rec, mods, precision, sink)
    if pattern == 'no_w':
      for p in mod.parameters():
        p.requires_grad_(False)
    passes = []
    for i in range(3):
      if i == 2:
        for _, lin in linears_of(torch, mod):
          lin.invalidate()
      if sink is not None and i != 1:
        sink.begin_window()
      passes.append(one_pass(torch, rec, run, pattern != 'no_x', mods, sink))
  return {'modules': {kind: describe(mod, MODULE_ATTRS.get(kind, ()))}, 'passes': passes}


def chain_scenario(torch, Fn, ops, widths, mx_at=(), group_local=None, group_ok=True, passes=1):
  """HipLinears applied one after the other with one sink: backward queues their gradients last to first."""
  from plainlm_amd import transformer as Tr
  rec = Recorder(torch, ops)
  rec.group_ok = group_ok
  with rec.patched():
    sink = traced_sink(rec, Fn)
    if group_local is not None:
      sink.dw_group_local = group_local
    lins = [Tr.HipLinear(a, b) for a, b in zip(widths[:-1], widths[1:])]
    mods = [(f'l{i}', lin) for i, lin in enumerate(lins)]
    prepare(torch, rec, mods, 'bf16', sink)
    for i in mx_at:
      lins[i].mx = True

    def run(x):
      for lin in lins:
        x = lin(x)
      return x
    sink.begin_window()
    out = [one_pass(torch, rec, run, True, mods, sink) for _ in range(passes)]
  return {'modules': {t: describe(m) for t, m in mods}, 'passes': out}


def record_all():
  import torch
  from plainlm_amd import functional as Fn
  from plainlm_amd import ops
  out = {}
  for precision in PRECISIONS:
    for kind in MODULES:
      for with_sink in (False, True):
        for pattern in GRAD_PATTERNS:
          out[f'{precision}-{kind}-{"sink" if with_sink else "autograd"}-{pattern}'] = module_scenario(torch, Fn, ops, kind, precision,
                                                                                                       with_sink, pattern)
  # the sink's queue: a flush in mid-queue (five gradients, groups of three); one MX and two bf16 gradients in one flush (the second bf16
  # Linear is 60 wide: its transposed shadow is padded to 64 columns and sliced); a single bf16 gradient (gemm_tn, never the grouped
  # launch); a grouped launch that is refused (gemm_tn each); two passes in one window (the second accumulates)
  out['sink-five-linears-groups-of-three'] = chain_scenario(torch, Fn, ops, [D] * 6, group_local=3)
  out['sink-one-mx-two-bf16'] = chain_scenario(torch, Fn, ops, [D, D, 60, D], mx_at=(0,))
  out['sink-single-bf16'] = chain_scenario(torch, Fn, ops, [D, D])
  out['sink-grouping-refused'] = chain_scenario(torch, Fn, ops, [D, D, 60, D], group_ok=False)
  out['sink-two-passes-one-window'] = chain_scenario(torch, Fn, ops, [D, D, D], mx_at=(1,), passes=2)
  return json.loads(json.dumps(out))  # tuples -> lists: exactly what the file holds


def main():
  out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'functional_trace_parent.json')
  scenarios = record_all()
  with open(out, 'w') as f:
    json.dump({'commit': 'c4c2987', 'scenarios': scenarios}, f, separators=(',', ':'))
    f.write('\n')
  print(f'{out}: {len(scenarios)} scenarios, {sum(len(p["ops"]) for s in scenarios.values() for p in s["passes"])} entries')


if __name__ == '__main__':
  main()
