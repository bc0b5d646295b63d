"""plainlm_amd/ops.py hands the C ABI what it handed it before its operand checks, workspaces and launch brackets were consolidated:
tests/golden/make_ops_trace_parent.py, run once on the commit before, wrote ops_trace_parent.json; the same code replays every
scenario here - CPU tensors that claim to be on the GPU, a recording fake in place of the library - and the traces must be equal as a
whole: the entry points and their order, every scalar, every pointer (operand + offset, returned tensor, scratch or NULL), every field
of an item table, what is returned, what LAUNCH_HOOK and PROFILE see and when, and for every refused input the exception and that
nothing was launched.  Then the workspace arena's own behaviour, against the same fakes."""
import collections
import ctypes as C
import functools
import importlib.util
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _load_generator():
  spec = importlib.util.spec_from_file_location('make_ops_trace_parent', os.path.join(GOLDEN, 'make_ops_trace_parent.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


GEN = _load_generator()
ops = GEN.ops
with open(os.path.join(GOLDEN, 'ops_trace_parent.json')) as f:
  PARENT = json.load(f)['scenarios']

# Every refusal whose type or message differs from the parent's, by scenario (<case>/<operand>/<mutation>).  The same inputs are refused.
OFF_GPU = "an operand off the GPU gets _need's RuntimeError('... no CPU path') like everywhere else; the parent raised the wrapper's ValueError"
SHADOWS = ('the (dst, dst_t) shadow-pair check is one helper with one wording, optim_cast_multi_\'s "[rows, cols]" / "[cols, >= rows]"; '
           'the type (ValueError) and the operand named are the parent\'s')
STRIDED = ("dtype, rank and inner stride are refused by _need's strided form, whose message does not repeat the wrapper's shape clause "
           '(which still guards the row stride and the row count); the type (ValueError) is the parent\'s')
QKV_COLS = 'a qkv width that is no multiple of 3 * nh is no stride fault: the message now says what is wrong; the type is the parent\'s'
ALLOWED = {
  **dict.fromkeys('''mx_quant/x/cpu mx_quant_multi/x/cpu mx_quant_multi/x2/cpu gemm_nt/A/cpu gemm_nt/B/cpu gemm_tn/A/cpu gemm_tn/B/cpu
    gemm_tn_grouped/A/cpu gemm_tn_grouped/B/cpu gemm_tn_grouped/A2/cpu gemm_tn_grouped/B2/cpu'''.split(), OFF_GPU),
  **dict.fromkeys('''cast_bf16_t:out/out_t/dtype cast_bf16_t:out/out_t/rank cast_bf16_t:out/out_t/inner cast_bf16_t:out/out_t/short
    cast_bf16_t:out/out_t/narrow cast_bf16_t_multi/src/short cast_bf16_t_multi/src/narrow cast_bf16_t_multi/out/dtype
    cast_bf16_t_multi/out/rank cast_bf16_t_multi/out/cpu cast_bf16_t_multi/out/inner cast_bf16_t_multi/out/short
    cast_bf16_t_multi/out/rows cast_bf16_t_multi/out/narrow cast_bf16_t_multi/out_t/dtype cast_bf16_t_multi/out_t/rank
    cast_bf16_t_multi/out_t/cpu cast_bf16_t_multi/out_t/inner cast_bf16_t_multi/out_t/short cast_bf16_t_multi/out_t/narrow
    cast_bf16_t_multi/src2/short cast_bf16_t_multi/src2/narrow cast_bf16_t_multi/out2/dtype cast_bf16_t_multi/out2/rank
    cast_bf16_t_multi/out2/cpu cast_bf16_t_multi/out2/inner cast_bf16_t_multi/out2/short cast_bf16_t_multi/out2/rows
    cast_bf16_t_multi/out2/narrow cast_bf16_t_multi/out_t2/dtype cast_bf16_t_multi/out_t2/rank cast_bf16_t_multi/out_t2/cpu
    cast_bf16_t_multi/out_t2/inner cast_bf16_t_multi/out_t2/short cast_bf16_t_multi/out_t2/narrow'''.split(), SHADOWS),
  **dict.fromkeys('''kv_append_rope/qkv/dtype kv_append_rope/qkv/rank kv_append_rope/qkv/inner kv_append_rope_rows/qkv/dtype
    kv_append_rope_rows/qkv/rank kv_append_rope_rows/qkv/inner sample_logits/logits/dtype sample_logits/logits/rank
    sample_logits/logits/inner spec_verify/target_logits/dtype spec_verify/target_logits/rank spec_verify/target_logits/inner
    spec_verify/draft_logits/dtype spec_verify/draft_logits/rank spec_verify/draft_logits/inner'''.split(), STRIDED),
  **dict.fromkeys('kv_append_rope/qkv/narrow kv_append_rope_rows/qkv/narrow'.split(), QKV_COLS),
}
NOT_TRACED = {'probe_ds_read_tr16', 'probe_mfma32',  # the two probes
              'mx_pad', 'optim_hparams', 'sfo_scalars', 'nadam_scalars',  # host arithmetic (optim_hparams is traced through its users)
              'release_workspaces', 'workspace_bytes'}  # new with the arena: tested below


@functools.lru_cache(maxsize=None)
def replayed():
  return GEN.record_all()


def test_every_wrapper_is_recorded_and_replayed():
  assert set(replayed()) == set(PARENT)
  cases = {name.split('/')[0].split(':')[0] for name in PARENT}
  public = {n for n, v in vars(ops).items() if callable(v) and not n.startswith('_') and getattr(v, '__module__', None) == ops.__name__
            and not isinstance(v, type)}
  assert public - NOT_TRACED <= cases | {'set_cu_reserve', 'cu_reserve', 'reload_env'}, sorted(public - NOT_TRACED - cases)
  assert 'reserve-and-env' in cases and len(PARENT) > 1000
  assert sum('raised' in s for s in PARENT.values()) > 700  # one scenario per operand and check


@pytest.mark.parametrize('case', sorted({name.split('/')[0] for name in PARENT}))
def test_trace_equals_the_parent(case):
  """The case itself, every mutation of its operands, and (as 'hook-reserve') the runs whose hook moves the CU reserve."""
  for name in [n for n in PARENT if n.split('/')[0] == case]:
    got, want = replayed()[name], PARENT[name]
    if name in ALLOWED:
      assert 'raised' in want and 'raised' in got and got['launches'] == 0, name
      assert got != want, f'{name} is listed in ALLOWED but equals the parent'
      continue
    assert set(got) == set(want), name
    for key in want:
      assert got[key] == want[key], f'{name}: {key} differ'


def test_refusals_launch_nothing():
  for name, s in replayed().items():
    if 'raised' in s and name != 'fc2_dx_swiglu_bwd:refused-twice':  # the library's own refusal, after two calls
      assert s['launches'] == 0, name
  assert set(ALLOWED) <= set(PARENT)


def test_the_recording_sees_what_it_is_there_for():
  """Guards the recording itself against going blind: the facts the scenarios were chosen to show are in the parent's file."""
  P = PARENT
  nt = P['gemm_nt']['calls'][0]
  assert nt[0] == 'plm_gemm_bf16_nt_ws' and nt[1:6] == ['A+0', 32, 'B+0', 32, 'ret0'] and nt[-3:] == ['scratch', 768, 'stream']
  assert P['gemm_nt:no-workspace']['calls'][0][-3:] == ['NULL', 0, 'stream']  # a 0 answer hands NULL and 0
  assert P['gemm_tn:no-workspace']['calls'][0][-3:] == ['NULL', 0, 'stream']
  assert P['head_score:no-workspace']['calls'][0][-3:] == ['scratch', 0, 'stream']  # the heads hand 16 bytes even then
  assert P['gemm_nt:strided-out-alpha']['calls'][0][1:7] == ['A+0', 40, 'B+0', 48, 'out+0', 24]  # row strides, the caller's out
  # the hook precedes the sized launch, and the size is the answer AFTER the hook moved the reserve (64 bytes per reserved CU here)
  for name, entry in (('gemm_nt', 'plm_gemm_bf16_nt_ws'), ('gemm_tn', 'plm_gemm_bf16_tn'), ('gemm_tn_grouped', 'plm_gemm_bf16_tn_grouped'),
                      ('head_score', 'plm_head_score_bf16'), ('head_predict', 'plm_head_predict_bf16')):
    calls = P[f'hook-reserve/{name}']['calls']
    assert [c[0] for c in calls] == ['hook', 'plm_set_cu_reserve', entry], name
  assert P['hook-reserve/gemm_tn_grouped']['calls'][2][-2] == P['gemm_tn_grouped']['calls'][0][-2] + 3 * 64
  assert P['hook-reserve/gemm_tn']['calls'][2][-2] == P['gemm_tn']['calls'][0][-2] + 3 * 64
  # the bracket: MFMA ops hook then time, HBM ops time without hooking, the masked pair hooks without timing
  assert P['gemm_nt']['inst'] == [['hook', 'gemm_nt', 2.0 * 24 * 16 * 32], ['event'], 'plm_gemm_bf16_nt_ws', ['event']]
  assert P['rmsnorm_fwd']['inst'] == [['event'], 'plm_rmsnorm_fwd', ['event']] and P['rmsnorm_fwd']['profile'][0][0] == 'hbm:rmsnorm_fwd'
  assert [e for e in P['attn_fwd_masked']['inst'] if e == ['event']] == [] and P['attn_fwd_masked']['inst'][1][0] == 'hook'
  assert P['attn_decode']['inst'] == ['plm_attn_decode'] and P['attn_decode']['profile'] == []
  # the masked pair count (a device reduction) is asked for only with PROFILE on, and after the hook got the causal estimate
  assert ['attn_flops', True] not in P['attn_fwd:doc']['calls']
  assert P['attn_fwd:doc']['inst'][1:4] == [['attn_flops', False], ['hook', 'attn_fwd', 36864.0], ['attn_flops', True]]
  # the -4 retry is two calls, the second with scratch; the sliced embedding is three launches over offsets of the same operands
  retry = P['fc2_dx_swiglu_bwd:retry']['calls']
  assert [c[7] for c in retry] == ['NULL', 'scratch'] and P['fc2_dx_swiglu_bwd:retry']['inst'].count('plm_fc2_dx_swiglu_bwd_bf16') == 2
  sliced = P['embed_bwd_sorted:sliced']['calls']
  assert [(c[1], c[4], c[7]) for c in sliced] == [('ids+0', 65536, 0), ('ids+524288', 65536, 1), ('ids+1048576', 10, 1)]
  assert P['embed_bwd_sorted:sliced-big-V'] == {**P['embed_bwd_sorted:sliced-big-V'], 'calls': [], 'ret': False}
  # grouped TN: accepted (an item table), refused by the library, by its contraction lengths, by its size
  assert len(P['gemm_tn_grouped']['calls'][0][1]) == 2 and P['gemm_tn_grouped']['ret'] is True
  for name in ('refused-by-the-library', 'k-differs', 'none', 'oversize'):
    assert P[f'gemm_tn_grouped:{name}']['calls'] == [] and P[f'gemm_tn_grouped:{name}']['ret'] is False
  # a caller's workspace goes through as it is; the automatic one is scratch at the size of the query's answer
  assert P['attn_decode:workspace']['calls'][0][-3:] == ['ws+0', 4000, 'stream'] and P['attn_decode']['calls'][0][-3:-1] == ['scratch', 1048]
  assert P['attn_decode:bad-splits']['raised'][0] == 'ValueError' and P['attn_extend_workspace:refused']['raised'][0] == 'ValueError'
  # refusals: every kind of exception the wrappers raise, and accepted mutations with their calls
  kinds = collections.Counter(s['raised'][0] for s in P.values() if 'raised' in s)
  assert set(kinds) == {'ValueError', 'RuntimeError', 'TypeError', 'KeyError'}
  assert 'calls' in P['gemm_nt/A/rows'] and 'raised' in P['rmsnorm_fwd/x/rows']


# ---- the workspace arena, against the same fakes -------------------------------------------------------------------------------
@pytest.fixture
def fake():
  rec = GEN.Recorder()
  with GEN.faked(rec):
    ops.release_workspaces()
    yield rec
    ops.release_workspaces()


def _every_workspace_user(i):
  """One call of every wrapper that takes a workspace, at the i-th of eight shapes."""
  z, BF16, F32, I64, I32 = GEN.z, torch.bfloat16, torch.float32, torch.int64, torch.int32
  M = 8 * (i + 1)
  ops.gemm_nt(z((M, 32), BF16), z((16, 32), BF16))
  ops.gemm_tn(z((32, M), BF16), z((32, 16), BF16))
  ops.gemm_tn_grouped([(z((32, M), BF16), z((32, 16), BF16), z((M, 16), F32), False, None)] * 2)
  ops.head_score(z((M, 32), BF16), z((50, 32), BF16), z((M,), I64))
  ops.head_predict(z((M, 32), BF16), z((50, 32), BF16))
  ops.embed_bwd_sorted(z((M,), I64), z((M, 8), F32), z((20, 8), F32), False)
  B = i + 1
  kv, lens = z((B, 8, 256), BF16), z((B,), I32)
  ops.attn_decode(z((B, 128), BF16), kv, lens, 2)
  ops.attn_extend(z((B * 3, 128), BF16), kv, lens, 2)


def test_arena_holds_the_largest_request_not_the_sum(fake):
  assert ops.workspace_bytes() == 0
  for i in range(8):
    _every_workspace_user(i)
  assert len(fake.sizes) == 8 * 8 and len(set(fake.sizes)) > 16  # many distinct requests ...
  assert ops.workspace_bytes() == max(fake.sizes) > 16  # ... one buffer, as large as the largest (the heads' floor of 16 is below it)
  for i in range(8):
    _every_workspace_user(i)
  assert ops.workspace_bytes() == max(fake.sizes)
  ops.release_workspaces()
  assert ops.workspace_bytes() == 0


def test_arena_reuses_its_storage_and_keeps_streams_apart(fake, monkeypatch):
  dev, s1, s2 = torch.device('cpu'), C.c_void_p(0x1000), C.c_void_p(0x2000)
  big = ops._workspace(dev, 4096, s1)
  assert big.dtype == torch.uint8 and big.numel() >= 4096
  for n in (1, 16, 4096):
    assert ops._workspace(dev, n, s1).data_ptr() == big.data_ptr()  # a request within the capacity: the same storage
  other = ops._workspace(dev, 64, s2)
  assert other.data_ptr() != big.data_ptr() and ops.workspace_bytes() == big.numel() + other.numel()
  assert ops._workspace(dev, 8192, s1).numel() >= 8192 and ops.workspace_bytes() == 8192 + other.numel()  # grown, the old one dropped
  # through a wrapper: the stream the launch gets is the stream whose arena it uses
  ops.release_workspaces()
  for handle in (0x1000, 0x2000):
    monkeypatch.setattr(ops, '_stream', lambda handle=handle: C.c_void_p(handle))
    ops.gemm_nt(GEN.z((24, 32), torch.bfloat16), GEN.z((16, 32), torch.bfloat16))
  assert len(ops._arenas) == 2 and {k[1] for k in ops._arenas} == {0x1000, 0x2000}


def test_workspace_functions_give_the_caller_a_buffer_of_their_own(fake):
  ws, nbytes = ops.attn_decode_workspace(2, 2, 64, 8, 0, 'cpu')
  ws2, _ = ops.attn_decode_workspace(2, 2, 64, 8, 0, 'cpu')
  assert ws.numel() == nbytes > 0 and ws.data_ptr() != ws2.data_ptr() and ops.workspace_bytes() == 0  # fresh, nothing registered
  ops.attn_decode(GEN.z((2, 128), torch.bfloat16), GEN.z((2, 8, 256), torch.bfloat16), GEN.z((2,), torch.int32), 2, workspace=(ws, nbytes))
  assert ops.workspace_bytes() == 0 and fake.entries[-1][-3] != 'NULL'  # a caller's workspace leaves the arena alone


def test_kv_caches_own_no_workspace(fake):
  from plainlm_amd.generate import KVCache
  _every_workspace_user(0)
  held = ops.workspace_bytes()
  for B in (1, 3, 8):
    cache = KVCache(2, B, 16, 2, 64, 'cpu')
    assert not hasattr(cache, 'workspace') and not hasattr(cache, 'extend_workspace')
    del cache
    assert ops.workspace_bytes() == held
