"""The launch plans of the bf16 GEMMs (csrc/gemm_plan.h) pinned against the library before the plans were gathered there: the four
workspace queries are host calls whose answers are the plans' slab layouts, recorded from commit 0604155 on an MI355X by
tests/golden/make_gemm_plan_parent.py (shape table and settings: its docstring).  The plans depend on the CU count, so the test insists
on the recorded device instead of skipping."""

import ctypes as C
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gemm_plan_parent.json')
SWITCHES = ('PLM_NT_NO_HYBRID', 'PLM_TN_NO_BIG', 'PLM_GEMM_V1', 'PLM_NT_HYBRID_MIN_K')


def _query(lib, kind, args):
  if kind == 'tn_grouped':
    ms, ns, k = args
    return int(lib.plm_gemm_tn_grouped_workspace_bytes((C.c_int64 * len(ms))(*ms), (C.c_int64 * len(ns))(*ns), len(ms), k))
  fn = {'nt': lib.plm_gemm_nt_workspace_bytes, 'tn': lib.plm_gemm_tn_workspace_bytes, 'head': lib.plm_head_score_workspace_bytes}[kind]
  return int(fn(*args))


def test_workspace_queries_answer_as_before_the_plan_header(monkeypatch):
  from plainlm_amd import _lib, ops
  with open(GOLDEN) as f:
    rec = json.load(f)
  assert torch.cuda.get_device_properties(0).multi_processor_count == rec['cu_count'], 'recorded on another device'
  lib = _lib.load()
  cases = rec['cases']
  assert len(cases) >= 100 and len(rec['settings']) == 8
  wrong = []
  try:
    for st in rec['settings']:
      for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
      for k, v in (st['env'] or {}).items():
        monkeypatch.setenv(k, v)
      ops.reload_env()
      ops.set_cu_reserve(st['reserve'])
      assert len(st['bytes']) == len(cases)
      for (kind, args), want in zip(cases, st['bytes']):
        got = _query(lib, kind, args)
        if got != want:
          wrong.append((st['reserve'], st['env'], kind, args if kind != 'tn_grouped' else (len(args[0]), args[0][:4], args[1][:4], args[2]), got, want))
  finally:
    monkeypatch.undo()
    ops.reload_env()
    ops.set_cu_reserve(0)
  assert not wrong, (len(wrong), wrong[:10])
