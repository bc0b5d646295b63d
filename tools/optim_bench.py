"""Optimizer tail on its own: the flat optimizer's clip_and_step (||g||^2 sweep + the update, with and without the bf16 shadows written by the
update launch) and the stand-alone weight cast it replaces, 160M model; for sfo_adamw also the train / eval swap (one lerp over the flat
parameters + the shadow invalidation; the re-cast is the stand-alone cast).
Usage (GPU box): python tools/optim_bench.py [--optim adamw|nadamw|sgd|signSGD|sfo_adamw ...]   (default: adamw)"""
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


ap = argparse.ArgumentParser()
ap.add_argument('--optim', nargs='+', choices=list(OPTIMS), default=['adamw'])
args = ap.parse_args()
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
