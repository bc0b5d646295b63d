"""The four GEMM workspace queries of the library BEFORE the launch plans moved into csrc/gemm_plan.h (commit 0604155), recorded
for tests/test_gemm_plan_gpu.py: plm_gemm_nt_workspace_bytes, plm_gemm_tn_workspace_bytes, plm_gemm_tn_grouped_workspace_bytes and
plm_head_score_workspace_bytes are host calls whose answers are the plans' slab layouts (hybrid stream-K of the NT kernel, split-K /
hybrid of the TN kernels, split search of the grouped TN kernel), so equal numbers mean equal plans.

Shape table: every GEMM of the 160M (B = 32, T = 1024), 420M (B = 8, T = 2048) and document-mask (160M at B = 8) steps as
tools/kbench.py lists them, and one shape on each side of every threshold of the plan code (the thresholds that depend on the grid
are placed with the recording device's CU count).  Settings: CU reserves 0 / 8 / 13 / 16 with the default switches, and the whole chip
once each under PLM_NT_NO_HYBRID, PLM_TN_NO_BIG, PLM_GEMM_V1 and PLM_NT_HYBRID_MIN_K=64.

gemm_plan_parent.json: {'commit', 'cu_count', 'cases': [[query, args], ...], 'settings': [{'reserve', 'env', 'bytes': [...]}, ...]}
with bytes[i] the answer for cases[i]; query is 'nt' / 'tn' / 'head' with args [M, N, K] or 'tn_grouped' with args [Ms, Ns, K].

Run on an MI355X from a checkout of commit 0604155 with its library built:
  python tests/golden/make_gemm_plan_parent.py [output .json]
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

RESERVES = (0, 8, 13, 16)
SWITCHES = ({'PLM_NT_NO_HYBRID': '1'}, {'PLM_TN_NO_BIG': '1'}, {'PLM_GEMM_V1': '1'}, {'PLM_NT_HYBRID_MIN_K': '64'})
ALL_SWITCHES = sorted({k for s in SWITCHES for k in s})


def cases(cus):
  out = []
  for B, T, d, h, V in ((32, 1024, 768, 2048, 50280), (8, 2048, 1024, 2816, 50280), (8, 1024, 768, 2048, 50280)):
    M = B * T
    for m, n, k in ((M, 3 * d, d), (M, d, d), (M, 2 * h, d), (M, d, h), (M, V, d), (M, d, 3 * d), (M, d, 2 * h), (M, h, d), (M, d, 50304)):
      out.append(['nt', [m, n, k]])
    for m, n, k in ((3 * d, d, M), (d, d, M), (2 * h, d, M), (d, h, M), (V, d, M)):
      out.append(['tn', [m, n, k]])
    out.append(['head', [M, V, d]])
    block = [(d, h), (2 * h, d), (d, d), (3 * d, d)]
    for nb in (1, 3, 6, 12):
      out.append(['tn_grouped', [[m for m, _ in block * nb], [n for _, n in block * nb], M]])
  # NT: the hybrid's floors (M 2048, N 256, K 8192, K % 64, N % 8), the single-round and packing tests, the bounds of L
  for m, n, k in ((504, 768, 8192), (512, 768, 8192), (32768, 120, 8192), (32768, 128, 8192), (2040, 12288, 8192), (2048, 12288, 8192),
                  (98304, 248, 8192), (98304, 256, 8192), (32768, 768, 8128), (32768, 768, 8192), (32768, 772, 8192), (32768, 768, 8200),
                  (256 * cus, 256, 8192), (256 * (cus + 1), 256, 8192), (256 * (cus + cus // 2), 256, 8192), (128 * cus, 512, 16384),
                  (34560, 512, 8192), (34816, 512, 8192), (35072, 512, 8192), (32768, 768, 2048), (32768, 768, 4096), (16384, 1024, 50304)):
    out.append(['nt', [m, n, k]])
  # TN: the persistent kernel's floors (M, N 256, K % 64), fewer tiles than slots / whole rounds / a remainder, the split caps (K / 512, 32) and
  # the 128x128 kernels' 512-tile test
  for m, n, k in ((248, 256, 32768), (256, 248, 32768), (256, 256, 32768), (120, 768, 32768), (128, 768, 32768), (768, 772, 32768),
                  (768, 768, 32776), (768, 768, 32768), (256 * cus, 256, 8192), (256 * (cus + 1), 256, 8192), (256 * (cus - 1), 256, 8192),
                  (2048, 3968, 8192), (2048, 4096, 8192), (768, 768, 256), (768, 768, 512), (768, 768, 1024), (768, 768, 65536), (8, 8, 64)):
    out.append(['tn', [m, n, k]])
  # grouped TN: 1 and 48 problems, mixed M and N, what the plan refuses (49 problems, K % 64, K < 64, M % 8), tile counts around the grid
  for ms, ns, k in (([768], [768], 32768), ([768] * 48, [768] * 48, 8192), ([768] * 49, [768] * 49, 8192), ([8, 264, 768, 4096], [50280, 8, 2304, 520], 16384),
                    ([768, 2048], [768, 768], 32776), ([768], [768], 32), ([764], [768], 8192), ([256 * cus], [256], 8192), ([256 * cus, 256], [256, 256], 8192),
                    ([768, 768], [768, 768], 64), ([768, 768], [768, 768], 512), ([768, 768], [768, 768], 576)):
    out.append(['tn_grouped', [ms, ns, k]])
  # scoring head: device-independent bound; the rows / partials cross-over and ragged V
  for m, v, k in ((504, 50280, 768), (512, 50280, 768), (512, 120, 768), (512, 128, 768), (32768, 50281, 768), (1, 8, 64), (255, 256, 64), (257, 50304, 64)):
    out.append(['head', [m, v, k]])
  return out


def query(lib, kind, args):
  if kind == 'tn_grouped':
    ms, ns, k = args
    return int(lib.plm_gemm_tn_grouped_workspace_bytes((C.c_int64 * len(ms))(*ms), (C.c_int64 * len(ns))(*ns), len(ms), k))
  fn = {'nt': lib.plm_gemm_nt_workspace_bytes, 'tn': lib.plm_gemm_tn_workspace_bytes, 'head': lib.plm_head_score_workspace_bytes}[kind]
  return int(fn(*args))


def apply_setting(ops, reserve, env):
  for k in ALL_SWITCHES:
    os.environ.pop(k, None)
  os.environ.update(env or {})
  ops.reload_env()
  ops.set_cu_reserve(reserve)


def main():
  import torch
  from plainlm_amd import _lib, ops
  lib = _lib.load()
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  table = cases(cus)
  settings = []
  for reserve, env in [(r, None) for r in RESERVES] + [(0, s) for s in SWITCHES]:
    apply_setting(ops, reserve, env)
    settings.append({'reserve': reserve, 'env': env, 'bytes': [query(lib, kind, args) for kind, args in table]})
  apply_setting(ops, 0, None)
  out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'gemm_plan_parent.json')
  with open(out, 'w') as f:
    json.dump({'commit': '0604155', 'cu_count': cus, 'cases': table, 'settings': settings}, f, separators=(',', ':'))
    f.write('\n')
  print(f'{out}: {len(table)} cases x {len(settings)} settings on {cus} CUs; '
        f'{sum(b > 0 for s in settings for b in s["bytes"])} non-zero answers')


if __name__ == '__main__':
  main()
