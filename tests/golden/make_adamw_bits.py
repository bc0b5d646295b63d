"""AdamW trajectories of the library BEFORE AdamW joined the plm_optim_* family (commit e28c6c9, ABI 111: plm_adamw_f32 and
plm_adamw_cast_multi, which formed decay = fma(-lr, wd, 1) and lr / bc1 on the device), frozen as bits for
tests/test_optim_gpu.py::test_adamw_bits_are_those_of_the_separate_adamw_kernels.

The inputs come from the seeded CPU generator below, which the test imports; adamw_bits.npz holds only the outputs.
  flat:   4099 elements, 3 steps, device clip coefficient 0.37, lr changing per step
  multi:  three matrices with partial 64 x 64 tiles and ld_t > rows, 2 steps, clip 0.61, with the shadows
each at an ordinary hyper-parameter set ('plain') and at lr = 0.826, wd = 0.71, beta1 = 0.9 ('sep', flat through step 3), where the
fused fp32 formation of decay (0.41354004 against 0.41354001) and the fp32 division lr / bc1 (step 3: 3.0479703 against 3.0479705)
differ from forming them in double and rounding once.  p, m, v and the shadows are kept as the LAST step leaves them: every earlier
step's bits feed them.

Keys: '<set>/flat/{p,m,v}', '<set>/multi/<i>/{p,m,v}', '<set>/multi/<i>/{dst,dst_t}' (bf16 bits as uint16).

Run on an MI355X, with a libplainlm_hip.so built from commit e28c6c9:
  python tests/golden/make_adamw_bits.py <path to that libplainlm_hip.so> [output .npz]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SETS = {'plain': dict(lr=1e-2, wd=0.1, b1=0.9, b2=0.95, eps=1e-8), 'sep': dict(lr=0.826, wd=0.71, b1=0.9, b2=0.95, eps=1e-8)}
FLAT_N, FLAT_STEPS, FLAT_CLIP = 4099, 3, 0.37
MULTI_SHAPES = [(72, 24, 80), (16, 72, 24), (8, 8, 16)]  # rows, cols, ld_t
MULTI_STEPS, MULTI_CLIP = 2, 0.61


def step_lr(hp, t):
  """learning rate of step t (1-based): the set's own at steps 1 and 3, half as much again at step 2"""
  return hp['lr'] * (1.5 if t == 2 else 1.0)


def flat_inputs():
  gen = torch.Generator().manual_seed(20261)
  p = torch.randn(FLAT_N, generator=gen)
  return p, [torch.randn(FLAT_N, generator=gen) for _ in range(FLAT_STEPS)]


def multi_inputs():
  """per matrix: (p, [g per step], m0, v0): the moments start non-zero"""
  gen = torch.Generator().manual_seed(20262)
  out = []
  for rows, cols, _ in MULTI_SHAPES:
    p = torch.randn(rows, cols, generator=gen)
    gs = [torch.randn(rows, cols, generator=gen) for _ in range(MULTI_STEPS)]
    out.append((p, gs, torch.randn(rows, cols, generator=gen) * 0.1, torch.rand(rows, cols, generator=gen) * 0.01))
  return out


class _Item(C.Structure):  # struct plm_adamw_item of ABI 111
  _fields_ = [(n, C.c_void_p) for n in ('p', 'g', 'm', 'v', 'dst', 'dst_t')] + [(n, C.c_int64) for n in ('rows', 'cols', 'ld_t')]


def main():
  lib = C.CDLL(sys.argv[1])
  out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, 'adamw_bits.npz')
  assert lib.plm_version() == 111, lib.plm_version()
  F, P = C.c_float, C.c_void_p
  lib.plm_adamw_f32.argtypes = [P, P, P, P, C.c_int64] + [F] * 7 + [P, P]
  lib.plm_adamw_cast_multi.argtypes = [C.POINTER(_Item), C.c_int] + [F] * 7 + [P, P]
  stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
  out = {}
  for name, hp in SETS.items():
    p0, gs = flat_inputs()
    p, m, v = p0.cuda(), torch.zeros(FLAT_N, device='cuda'), torch.zeros(FLAT_N, device='cuda')
    clip = torch.tensor([FLAT_CLIP], device='cuda')
    for t in range(1, FLAT_STEPS + 1):
      g = gs[t - 1].cuda()
      rc = lib.plm_adamw_f32(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), FLAT_N, step_lr(hp, t), hp['b1'], hp['b2'], hp['eps'],
                             hp['wd'], 1.0 - hp['b1'] ** t, 1.0 - hp['b2'] ** t, clip.data_ptr(), stream())
      assert rc == 0
    torch.cuda.synchronize()
    for k, x in (('p', p), ('m', m), ('v', v)):
      out[f'{name}/flat/{k}'] = x.cpu().numpy()
    mats = [(p.cuda(), [g.cuda() for g in gs], m.cuda(), v.cuda(), torch.empty(p.shape, dtype=torch.bfloat16, device='cuda'),
             torch.full((p.shape[1], ld_t), 7.0, dtype=torch.bfloat16, device='cuda'))
            for (p, gs, m, v), (_, _, ld_t) in zip(multi_inputs(), MULTI_SHAPES)]
    clip = torch.tensor([MULTI_CLIP], device='cuda')
    for t in range(1, MULTI_STEPS + 1):
      table = (_Item * len(mats))()
      for i, (p, gs, m, v, dst, dst_t) in enumerate(mats):
        table[i] = _Item(p.data_ptr(), gs[t - 1].data_ptr(), m.data_ptr(), v.data_ptr(), dst.data_ptr(), dst_t.data_ptr(), p.shape[0], p.shape[1],
                         dst_t.stride(0))
      rc = lib.plm_adamw_cast_multi(table, len(mats), step_lr(hp, t), hp['b1'], hp['b2'], hp['eps'], hp['wd'], 1.0 - hp['b1'] ** t,
                                    1.0 - hp['b2'] ** t, clip.data_ptr(), stream())
      assert rc == 0
    torch.cuda.synchronize()
    for i, (p, _, m, v, dst, dst_t) in enumerate(mats):
      for k, x in (('p', p), ('m', m), ('v', v)):
        out[f'{name}/multi/{i}/{k}'] = x.cpu().numpy()
      out[f'{name}/multi/{i}/dst'] = dst.view(torch.int16).cpu().numpy().view(np.uint16)
      out[f'{name}/multi/{i}/dst_t'] = dst_t.view(torch.int16).cpu().numpy().view(np.uint16)
  np.savez_compressed(out_path, **out)
  print(f'wrote {out_path}: {len(out)} arrays, {os.path.getsize(out_path)} bytes')


if __name__ == '__main__':
  main()
