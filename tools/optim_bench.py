"""Optimizer tail on its own: the flat optimizer's clip_and_step (||g||^2 sweep + the update, with and without the bf16 shadows written by the
update launch) and the stand-alone weight cast it replaces, 160M model; for sfo_adamw also the train / eval swap (one lerp over the flat
parameters + the shadow invalidation; the re-cast is the stand-alone cast).
Usage (GPU box): python tools/optim_bench.py [--optim adamw|nadamw|sgd|signSGD|sfo_adamw ...]   (default: adamw)
                 python tools/optim_bench.py --muon   the Muon tail: FlatMuon, its torch twin and FlatAdamW at the 160M
                                                      shape in one process, sides alternating, HIP events, median of 20 with [min max]; the
                                                      Newton-Schulz part alone with its TFLOP/s; the Muon group's launch count"""
import argparse, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
import plainlm_amd as P
from plainlm_amd import optim as O

OPTIMS = {
  'adamw': lambda m, g: O.FlatAdamW(m, g, lr=1e-4, betas=[0.9, 0.95], eps=1e-8, weight_decay=0.1),
  'nadamw': lambda m, g: O.FlatNAdamW(m, g, lr=1e-4, betas=[0.9, 0.95], eps=1e-8, weight_decay=0.1),
  'sgd': lambda m, g: O.FlatSGD(m, g, lr=1e-4, momentum=0.9, dampening=0.0, weight_decay=0.1),
  'signSGD': lambda m, g: O.FlatSignSGD(m, g, lr=1e-4, momentum=0.9, dampening=0.0, weight_decay=0.1),
  'sfo_adamw': lambda m, g: O.FlatAdamWScheduleFree(m, g, lr=1e-4, betas=[0.9, 0.95], weight_decay=0.1, warmup_steps=0),
}


def t(fn, it=20):
  for _ in range(5): fn()
  torch.cuda.synchronize()
  s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  s.record()
  for _ in range(it): fn()
  e.record(); torch.cuda.synchronize()
  return s.elapsed_time(e) / it


def muon_bench(rounds=20, warmup=3, headline_ms=30.0):
  import statistics
  from plainlm_amd import ops
  dev = torch.device('cuda')
  kw = dict(lr=1e-4, betas=[0.9, 0.95], eps=1e-8, weight_decay=0.1)
  gen = torch.Generator(device='cuda').manual_seed(0)

  def flat(cls, groups_of):
    m = bench.build_model(bench.CONFIGS['160m'], dev)
    m.enable_main_grad()
    opt = cls(m, groups_of(m), **kw)
    opt.flat_g.normal_(generator=gen)
    return m, opt
  muon_groups = lambda m: O.muon_param_groups(m, P.get_param_groups(m, 0.1))  # noqa: E731
  m1, fm = flat(O.FlatMuon, muon_groups)
  m2, fa = flat(O.FlatAdamW, lambda m: P.get_param_groups(m, 0.1))
  m3 = bench.build_model(bench.CONFIGS['160m'], dev)
  tw = O.Muon(muon_groups(m3), **kw)
  params3 = list(m3.parameters())
  for p in params3:
    p.grad = torch.randn(p.shape, device=dev, generator=gen)

  def twin_step():
    torch.nn.utils.clip_grad_norm_(params3, 1.0)
    tw.step()
  shapes = [tuple(p.shape) for p in fm.param_groups[0]['params']]
  steps = fm.param_groups[0]['ns_steps']
  ws = ops.muon_workspace(shapes, dev)
  table, _ = ops.muon_items([(None, p.main_grad, torch.zeros_like(p), None, None) for p in fm.param_groups[0]['params']])
  ops.muon_prepare(table, shapes, 0.0, False, torch.zeros(len(shapes), device=dev), workspace=ws)
  sides = {'FlatMuon clip_and_step': lambda: fm.clip_and_step(1.0), 'optim.Muon twin (clip_grad_norm_ + step)': twin_step,
           'FlatAdamW clip_and_step': lambda: fa.clip_and_step(1.0),
           'Newton-Schulz alone (ops.muon_orthogonalize)': lambda: ops.muon_orthogonalize(shapes, steps, dev, workspace=ws)}
  times = {k: [] for k in sides}
  for r in range(warmup + rounds):
    for k, fn in sides.items():   # sides alternating inside one process
      s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      s.record()
      fn()
      e.record()
      torch.cuda.synchronize()
      if r >= warmup:
        times[k].append(s.elapsed_time(e))
  print(f'# tools/optim_bench.py --muon: 160M shape, {len(shapes)} block matrices {sorted(set(shapes))}, one process, sides alternating, HIP events,')
  print(f'# median of {rounds} [min max] ms after {warmup} warm-up rounds; workspace {ws[1] / 1e6:.1f} MB')
  med = {}
  for k, v in times.items():
    med[k] = statistics.median(v)
    print(f'{k:48s} {med[k]:8.3f} [{min(v):.3f} {max(v):.3f}] ms')
  fl = ops.muon_ns_flops(shapes, steps)
  ns = 'Newton-Schulz alone (ops.muon_orthogonalize)'
  print(f'Newton-Schulz: {fl / 1e12:.3f} TFLOP per step, {fl / med[ns] / 1e9:.1f} TFLOP/s at the median')
  n = len(shapes)
  g32, g56 = -(-n // ops.NT_BATCH_GROUP), -(-n // 56)
  print(f'Muon group launches per step: prepare {2 * g56} + Newton-Schulz {steps} x 3 x {g32} = {steps * 3 * g32} + apply {g56} = {2 * g56 + steps * 3 * g32 + g56}'
        f' (a loop over plm_gemm_bf16_nt would take {steps * 3 * n})')
  a, b = 'FlatMuon clip_and_step', 'optim.Muon twin (clip_grad_norm_ + step)'
  print(f'share of a {headline_ms:.0f} ms headline step: FlatMuon tail {100 * med[a] / headline_ms:.1f} %, FlatAdamW tail {100 * med["FlatAdamW clip_and_step"] / headline_ms:.1f} %')
  below = max(times[a]) < min(times[b])
  print(f"FlatMuon's range lies wholly below the twin's: {'yes' if below else 'NO'}")


ap = argparse.ArgumentParser()
ap.add_argument('--optim', nargs='+', choices=list(OPTIMS), default=['adamw'])
ap.add_argument('--muon', action='store_true')
args = ap.parse_args()
if args.muon:
  muon_bench()
  sys.exit(0)
for name in args.optim:
  for shadows in ('1', '0'):
    os.environ['PLM_ADAMW_SHADOWS'] = shadows
    model = bench.build_model(bench.CONFIGS['160m'], torch.device('cuda'))
    model.enable_main_grad()
    opt = OPTIMS[name](model, P.get_param_groups(model, 0.1))
    opt.flat_g.normal_()
    step = t(lambda: opt.clip_and_step(1.0))
    def cast():
      model.invalidate_shadows()
      model.refresh_shadows()
    swap = ''
    if hasattr(opt, 'eval'):
      swap = f', eval / train swap {t(lambda: (opt.eval(), opt.train())) / 2:.3f} ms each'
    print(f'{name} PLM_ADAMW_SHADOWS={shadows}: clip_and_step {step:.3f} ms, stand-alone cast of all weights {t(cast):.3f} ms{swap}', flush=True)
    del model, opt
