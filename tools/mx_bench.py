"""MXFP8 vs bf16 on the GEMMs of the block linears, random operands (never zeros: zero
operands read high).  Per step shape (forward Y = X W^T, dX = dY W, dW = dY^T X of w_qkv, w_out, fc1, fc2): the bf16 kernel the step uses
(gemm_nt; gemm_tn for dW) vs the MX NT GEMM, ms and TFLOP/s, quantization excluded; then the quantizer (both orientations of the
activation-side operand, one read) in ms and TB/s of algorithmic bytes, and the grouped
quantization of every block weight; with --step, the whole training step (fwd + bwd of the model's loss) with linear_precision bf16
and mxfp8, alternating in one process.
Usage: python tools/mx_bench.py [--config 160m|420m] [--iters 20] [--step] [--no-gemm] [--json out.jsonl]"""
import time
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from plainlm_amd import ops  # noqa: E402

BF = torch.bfloat16
CFG = {'160m': dict(B=32, T=1024, d=768, h=2048, nh=12, layers=12, V=50280), '420m': dict(B=8, T=2048, d=1024, h=2816, nh=16, layers=24, V=50280)}


def timeit(fn, iters, warmup=10):
  for _ in range(warmup):
    fn()
  torch.cuda.synchronize()
  s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  s.record()
  for _ in range(iters):
    fn()
  e.record()
  torch.cuda.synchronize()
  return s.elapsed_time(e) / iters


def gemm_rows(c, iters, out):
  M, d, h = c['B'] * c['T'], c['d'], c['h']
  lin = {'qkv': (3 * d, d), 'out': (d, d), 'fc1': (2 * h, d), 'fc2': (d, h)}
  rows = []
  for name, (nout, nin) in lin.items():
    for kind, (m, n, k) in (('fwd', (M, nout, nin)), ('dX', (M, nin, nout)), ('dW', (nout, nin, M))):
      g = torch.Generator(device='cuda').manual_seed(m + n + k)
      a = torch.randn(m, k, device='cuda', dtype=BF, generator=g)
      b = torch.randn(n, k, device='cuda', dtype=BF, generator=g) * 0.02
      if kind == 'dW':  # the bf16 step runs dW as TN over [tokens, *] operands
        at, bt = a.t().contiguous(), b.t().contiguous()
        acc = torch.zeros(m, n, device='cuda')
        t_bf = timeit(lambda: ops.gemm_tn(at, bt, out=acc, accumulate=True), iters)
      else:
        t_bf = timeit(lambda: ops.gemm_nt(a, b), iters)
      qa, _ = ops.mx_quant(a, cols=False)
      qb, _ = ops.mx_quant(b, cols=False)
      if kind == 'dW':
        acc = torch.zeros(m, n, device='cuda')
        t_mx = timeit(lambda: ops.gemm_mx_nt(qa, qb, out=acc, accumulate=True), iters)
      else:
        t_mx = timeit(lambda: ops.gemm_mx_nt(qa, qb), iters)
      fl = 2.0 * m * n * k
      r = dict(linear=name, gemm=kind, M=m, N=n, K=k, bf16_ms=round(t_bf, 4), mx_ms=round(t_mx, 4), bf16_tflops=round(fl / t_bf / 1e9, 1),
               mx_tflops=round(fl / t_mx / 1e9, 1), speedup=round(t_bf / t_mx, 3))
      rows.append(r)
      print('%-4s %-3s (%6d, %5d, %6d)  bf16 %7.3f ms %6.0f TF | mx %7.3f ms %6.0f TF | x%.2f' % (name, kind, m, n, k, t_bf, r['bf16_tflops'], t_mx,
                                                                                              r['mx_tflops'], r['speedup']), flush=True)
      if out:
        out.write(json.dumps(r) + '\n')
      del a, b, qa, qb
  return rows


def quant_rows(c, iters, out):
  M, d, h = c['B'] * c['T'], c['d'], c['h']
  for cols in sorted({d, 2 * h, h, 3 * d}):
    x = torch.randn(M, cols, device='cuda', dtype=BF)
    for rows_, cols_ in ((True, True), (True, False)):
      t = timeit(lambda: ops.mx_quant(x, rows=rows_, cols=cols_), iters)
      nbytes = 2 * x.numel() + 1.03125 * x.numel() * (int(rows_) + int(cols_))
      r = dict(quant=f'[{M}, {cols}]', orientations='both' if cols_ else 'rows', ms=round(t, 4), tbps=round(nbytes / t / 1e9, 2))
      print('quant [%6d, %5d] %-5s %7.3f ms %5.2f TB/s' % (M, cols, r['orientations'], t, r['tbps']), flush=True)
      if out:
        out.write(json.dumps(r) + '\n')
  items = [torch.randn(o, i, device='cuda', dtype=BF) for _ in range(c['layers']) for o, i in ((3 * d, d), (d, d), (2 * h, d), (d, h))]
  t = timeit(lambda: ops.mx_quant_multi(items), iters)
  n = sum(x.numel() for x in items)
  print('quant_multi: %d weights, %.3f ms, %.2f TB/s' % (len(items), t, (2 + 2 * 1.03125) * n / t / 1e9), flush=True)


def step_rows(c, iters, out):
  from plainlm_amd.transformer import ModelConfig, Transformer
  models = {}
  for prec in ('bf16', 'mxfp8'):
    torch.manual_seed(0)
    models[prec] = Transformer(ModelConfig(vocab_size=c['V'], seq_len=c['T'], dim=c['d'], expand=8 / 3, n_layers=c['layers'], n_heads=c['nh'],
                                           mlp='glu', linear_precision=prec)).cuda()
  g = torch.Generator(device='cuda').manual_seed(0)
  ids = torch.randint(0, c['V'], (c['B'], c['T']), device='cuda', generator=g)
  tgt = torch.randint(0, c['V'], (c['B'], c['T']), device='cuda', generator=g)

  def step(m):
    m.zero_grad(set_to_none=True)
    m.loss(ids, tgt).backward()

  for m in models.values():
    for _ in range(3):
      step(m)
  times = {p: [] for p in models}
  for _ in range(iters):
    for p, m in models.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      step(m)
      torch.cuda.synchronize()
      times[p].append((time.perf_counter() - t0) * 1e3)
  for p, ts in times.items():
    ts.sort()
    r = dict(step=p, median_ms=round(ts[len(ts) // 2], 3), min_ms=round(ts[0], 3), tok_per_s=round(c['B'] * c['T'] / ts[len(ts) // 2] * 1e3))
    print('step %-6s median %8.3f ms  min %8.3f ms  %9d tok/s' % (p, r['median_ms'], r['min_ms'], r['tok_per_s']), flush=True)
    if out:
      out.write(json.dumps(r) + '\n')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', default='160m', choices=sorted(CFG))
  ap.add_argument('--iters', type=int, default=20)
  ap.add_argument('--step', action='store_true', help='also the whole training step, bf16 vs mxfp8')
  ap.add_argument('--no-gemm', action='store_true', help='skip the per-shape GEMM and quantizer rows')
  ap.add_argument('--json', default='')
  a = ap.parse_args()
  if not torch.cuda.is_available():
    sys.exit('mx_bench.py measures the GPU kernels: no GPU found')
  c = CFG[a.config]
  out = open(a.json, 'a') if a.json else None
  if not a.no_gemm:
    gemm_rows(c, a.iters, out)
    quant_rows(c, a.iters, out)
  if a.step:
    step_rows(c, max(a.iters, 10), out)


if __name__ == '__main__':
  main()
