"""Pin the CPU oracle to the reference's own outputs (tests/golden/*.npz, produced
by tests/golden/make_golden.py from the imported reference).  fp32, tolerance 2e-6
relative to the tensor's max magnitude (torch CPU fp32 roundoff between two
orderings of the same arithmetic)."""

import os

import numpy as np
import pytest
import torch

from oracle import cpu_ref as O

TOL = 2e-6


def _load(golden_dir, name):
  z = np.load(os.path.join(golden_dir, name))
  return {k: torch.from_numpy(z[k]) for k in z.files}


def _close(a, b, tol=TOL):
  a, b = a.double(), b.double()
  scale = max(b.abs().max().item(), 1e-30)
  err = (a - b).abs().max().item()
  assert err <= tol * scale, f'max err {err:.3e} vs scale {scale:.3e}'


@pytest.fixture(scope='module')
def ops(golden_dir):
  return _load(golden_dir, 'ops.npz')


@pytest.fixture(scope='module')
def mdl(golden_dir):
  return _load(golden_dir, 'model.npz')


def test_rmsnorm_fwd_bwd(ops):
  x = ops['rms_x'].clone().requires_grad_(True)
  w = ops['rms_w'].clone().requires_grad_(True)
  y = O.rmsnorm(x, w)
  _close(y.detach(), ops['rms_y'])
  y.backward(ops['rms_dy'])
  _close(x.grad, ops['rms_dx'])
  _close(w.grad, ops['rms_dw'])


def test_rope_table_and_apply(ops):
  cos, sin = O.rope_table(64, 2048)
  rows = ops['rope_rows'].long()
  assert torch.equal(cos[rows], ops['rope_cos_rows'])
  assert torch.equal(sin[rows], ops['rope_sin_rows'])
  _close(O.rope_apply(ops['rope_q'], cos, sin), ops['rope_qr'])
  _close(O.rope_apply(ops['rope_k'], cos, sin), ops['rope_kr'])


def _docs(ops_or_mdl, key):
  return [[int(v) for v in row if v > 0] for row in ops_or_mdl[key]]


@pytest.mark.parametrize('tag', ['c', 'm'])
def test_attention_fwd_bwd(ops, tag):
  q, k, v = (ops[f'att{tag}_{n}'].clone().requires_grad_(True) for n in 'qkv')
  ds = O.doc_start_from_lengths(_docs(ops, 'attm_docs_lengths'), q.shape[1]) if tag == 'm' else None
  o = O.attention(q, k, v, ds)
  _close(o.detach(), ops[f'att{tag}_o'])
  o.backward(ops[f'att{tag}_do'])
  for n, t in zip('qkv', (q, k, v)):
    _close(t.grad, ops[f'att{tag}_d{n}'], 5e-6)


def test_doc_mask_matches_reference_mask(ops):
  ds = O.doc_start_from_lengths(_docs(ops, 'attm_docs_lengths'), 64)
  assert torch.equal(O.mask_from_doc_start(ds), ops['attm_mask'])
  # a single document is exactly the causal mask
  one = O.doc_start_from_lengths([[65]], 64)
  assert torch.equal(O.mask_from_doc_start(one)[0], torch.ones(64, 64, dtype=torch.bool).tril())
  with pytest.raises(ValueError):
    O.doc_start_from_lengths([[10, 10]], 64)


def test_glu_hidden_dim_and_fwd_bwd(ops):
  for d, ex, h in zip(ops['hid_dim'], ops['hid_expand'], ops['hid_out']):
    assert O.glu_hidden_dim(int(d), float(ex)) == int(h)
  assert O.parse_expand('8/3') == 8 / 3
  x = ops['glu_x'].clone().requires_grad_(True)
  w1 = ops['glu_w1'].clone().requires_grad_(True)
  w2 = ops['glu_w2'].clone().requires_grad_(True)
  y = O.swiglu(x @ w1.t(), w2.shape[1]) @ w2.t()
  _close(y.detach(), ops['glu_y'])
  y.backward(ops['glu_dy'])
  _close(x.grad, ops['glu_dx'])
  _close(w1.grad, ops['glu_dw1'])
  _close(w2.grad, ops['glu_dw2'])


def test_cross_entropy(ops):
  lg = ops['ce_logits'].clone().requires_grad_(True)
  loss = O.cross_entropy(lg, ops['ce_targets'])
  _close(loss.detach(), ops['ce_loss'])
  loss.backward()
  _close(lg.grad, ops['ce_dlogits'])


def test_embedding_repeated_ids(ops):
  w = ops['emb_w'].clone().requires_grad_(True)
  out = w[ops['emb_ids']]
  assert torch.equal(out.detach(), ops['emb_out'])
  out.backward(ops['emb_dout'])
  _close(w.grad, ops['emb_dw'])


def _model_cfg():
  return O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=2)


def _weights(mdl):
  return {k[2:]: v for k, v in mdl.items() if k.startswith('w:')}


def test_param_names_shapes_init(mdl):
  cfg = _model_cfg()
  w = _weights(mdl)
  assert list(w) == O.param_names(cfg)
  assert {n: tuple(t.shape) for n, t in w.items()} == O.param_shapes(cfg)
  # init distribution statistics of the reference (transformer.py:116-129)
  mine = O.init_params(cfg, seed=3)
  for i, n in enumerate(O.param_names(cfg)):
    ref_std = float(mdl['init_std'][i])
    if 'norm' in n:
      assert torch.equal(mine[n], torch.ones_like(mine[n])) and ref_std == 0.0
    else:
      assert abs(mine[n].std().item() - ref_std) < 0.06 * ref_std, n
      assert abs(mine[n].mean().item()) < 4 * ref_std / np.sqrt(mine[n].numel()) + 1e-4


def test_model_forward_backward(mdl):
  cfg = _model_cfg()
  w = _weights(mdl)
  tok = mdl['tokens']
  ids, tgt = tok[:, :64], tok[:, 1:65]
  _close(O.forward(w, cfg, ids), mdl['logits'])
  ds = O.doc_start_from_lengths(_docs(mdl, 'docs_lengths'), 64)
  _close(O.forward(w, cfg, ids, ds), mdl['logits_docmask'])
  loss, grads = O.loss_and_grads(w, cfg, ids, tgt)
  _close(loss, mdl['loss'])
  for n in O.param_names(cfg):
    _close(grads[n], mdl['g:' + n], 5e-6)


def test_engine_loss_sequence(mdl, golden_dir):
  """engine/engine.py:93-141 over 4 optimizer steps (accum 4, clip 1.0, AdamW, warmup-cosine)."""
  en = _load(golden_dir, 'engine.npz')
  cfg = _model_cfg()
  eng = O.OracleEngine(_weights(mdl), cfg, lr=3e-3, weight_decay=0.1, beta1=0.9, beta2=0.95, grad_clip=1.0,
                       accum=4, steps_budget=8, warmup_steps=2)
  losses, lrs, norms = [], [], []
  for i in range(en['tokens'].shape[0]):
    losses.append(eng.step({'input_ids': en['tokens'][i]}).item())
    if (i + 1) % 4 == 0:
      lrs.append(eng.lr)
      norms.append([eng.params[n].norm().item() for n in O.param_names(cfg)])
  np.testing.assert_allclose(losses, en['losses'].numpy(), rtol=2e-6)
  np.testing.assert_allclose(lrs, en['lrs'].numpy(), rtol=1e-12)
  np.testing.assert_allclose(norms, en['param_norms'].numpy(), rtol=5e-6)
  _close(eng.params['layers.1.mlp.fc2.weight'], en['final:layers.1.mlp.fc2.weight'], 5e-5)
  _close(eng.params['out_norm.weight'], en['final:out_norm.weight'], 5e-6)
  _close(eng.params['embed_tokens.weight'][:16], en['final:embed_rows'], 5e-5)


def _cfg1_checksums(params):
  return np.array([[float(p.double().sum()), float(p.double().abs().sum())] for p in params.values()])


def test_engine_cfg1_literal_shape(golden_dir):
  """BASELINE configs[0] / SURVEY section 8c at its literal shape - 2 layers, d = 128, 2 heads, seq 128, V = 50 280, micro-batch 1 x
  accumulation 4, 6 optimizer steps - as the REFERENCE engine ran it on the CPU (tests/golden/make_cfg1.py): the oracle engine reproduces the 24
  micro-step losses, the 6 learning rates, all parameter norms per step and the final-weight slices.  The initial weights are
  init_params(seed 7) on both sides; their checksums are part of the fixture."""
  z = _load(golden_dir, 'cfg1.npz')
  cfg = O.OracleConfig(vocab_size=50280, seq_len=128, dim=128, n_layers=2, n_heads=2)
  w = O.init_params(cfg, seed=7)
  np.testing.assert_allclose(_cfg1_checksums(w), z['init_checksums'].numpy(), rtol=1e-12)
  eng = O.OracleEngine(w, cfg, lr=3e-3, weight_decay=0.1, beta1=0.9, beta2=0.95, grad_clip=1.0, accum=4, steps_budget=6, warmup_steps=2)
  losses, lrs, norms = [], [], []
  for i in range(z['tokens'].shape[0]):
    losses.append(eng.step({'input_ids': z['tokens'][i]}).item())
    if (i + 1) % 4 == 0:
      lrs.append(eng.lr)
      norms.append([eng.params[n].norm().item() for n in O.param_names(cfg)])
  np.testing.assert_allclose(losses, z['losses'].numpy(), rtol=2e-6)
  np.testing.assert_allclose(lrs, z['lrs'].numpy(), rtol=1e-12)
  np.testing.assert_allclose(norms, z['param_norms'].numpy(), rtol=5e-6)
  rows = z['rows']
  _close(eng.params['embed_tokens.weight'][rows], z['final:embed_rows'], 5e-5)
  _close(eng.params['lm_head.weight'][rows], z['final:lm_head_rows'], 5e-5)
  _close(eng.params['layers.1.mlp.fc2.weight'], z['final:layers.1.mlp.fc2.weight'], 5e-5)
  _close(eng.params['layers.0.attn.w_qkv.weight'][:32], z['final:layers.0.attn.w_qkv.weight'], 5e-5)
  _close(eng.params['out_norm.weight'], z['final:out_norm.weight'], 5e-6)


@pytest.mark.parametrize('kind', ['mlp', 'mlp_relu_sq'])
def test_plain_mlp_classes_vs_reference(golden_dir, kind):
  """models/transformer.py:26: the two MLP classes beside 'glu' (components.py:31-40 silu MLP, :59-70 relu-squared MLP) - loss, logits and all
  15 gradients of the reference model on the CPU (tests/golden/make_mlp_classes.py)."""
  z = _load(golden_dir, 'mlp_classes.npz')
  cfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=2, mlp=kind)
  assert O.param_shapes(cfg)['layers.0.mlp.fc1.weight'] == (512, 128)  # one projection, not gate | up
  w = O.init_params(cfg, seed=3)
  np.testing.assert_allclose(_cfg1_checksums(w), z[f'{kind}:init_checksums'].numpy(), rtol=1e-12)
  tok = z['tokens']
  _close(O.forward(w, cfg, tok[:, :64]), z[f'{kind}:logits'], 5e-6)
  loss, g = O.loss_and_grads(w, cfg, tok[:, :64], tok[:, 1:])
  _close(loss, z[f'{kind}:loss'])
  for n in w:
    _close(g[n], z[f'{kind}:g:{n}'], 5e-6)


# ---- bf16-emulating mode (oracle/cpu_ref_bf16.py) ----------------------------------------------------------------------
def test_bf16_mode_without_rounding_equals_fp32_oracle(mdl):
  """The hand-written forward + backward of the emulating mode IS the reference's algorithm: with the bf16 rounding
  switched off it reproduces the golden loss and all 15 gradients of the reference model (causal and document-masked),
  and the tied-embedding variant of the fp32 oracle."""
  from oracle import cpu_ref_bf16 as E
  cfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=2)
  w = {k[2:]: v for k, v in mdl.items() if k.startswith('w:')}
  tok = mdl['tokens']
  ids, tgt = tok[:, :64], tok[:, 1:65]
  loss, g = E.loss_and_grads(w, cfg, ids, tgt, round_bf16=False)
  _close(loss, mdl['loss'])
  for n in w:
    _close(g[n], mdl['g:' + n], 5e-6)
  ds = O.doc_start_from_lengths(_docs(mdl, 'docs_lengths'), 64)
  l0, g0 = O.loss_and_grads(w, cfg, ids, tgt, ds, scale=0.25)
  l1, g1 = E.loss_and_grads(w, cfg, ids, tgt, ds, scale=0.25, round_bf16=False)
  _close(l1, l0)
  for n in w:
    _close(g1[n], g0[n], 5e-6)
  tcfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=2, tie_embeddings=True)
  tw = {k: v for k, v in w.items() if k != 'lm_head.weight'}
  l0, g0 = O.loss_and_grads(tw, tcfg, ids, tgt)
  l1, g1 = E.loss_and_grads(tw, tcfg, ids, tgt, round_bf16=False)
  _close(l1, l0)
  for n in tw:
    _close(g1[n], g0[n], 5e-6)


def test_bf16_mode_engine_tracks_the_reference_trajectory(mdl, golden_dir):
  """What bf16 rounding ALONE does to the reference's 16-micro-step trajectory (4 optimizer steps, the last three with
  lr > 0): the emulated bf16 flow stays within 1e-4 of the reference engine's own fp32 losses on every micro-step, before
  and after real parameter updates - so 1e-4 is a fair bar for the HIP engine on all 16 steps, and a kernel that is off by
  1e-3 cannot hide behind 'bf16 drift' (the GPU test asserts exactly this)."""
  from oracle import cpu_ref_bf16 as E
  en = np.load(os.path.join(golden_dir, 'engine.npz'))
  cfg = O.OracleConfig(vocab_size=256, seq_len=64, dim=128, n_layers=2, n_heads=2)
  w = {k[2:]: v for k, v in mdl.items() if k.startswith('w:')}
  tokens = torch.from_numpy(en['tokens'])
  kw = dict(lr=3e-3, weight_decay=0.1, beta1=0.9, beta2=0.95, grad_clip=1.0, accum=4, steps_budget=8, warmup_steps=2)
  emu = E.OracleEngineBF16(w, cfg, **kw)
  exact = E.OracleEngineBF16(w, cfg, round_bf16=False, **kw)
  le = np.array([emu.step({'input_ids': tokens[i]}).item() for i in range(16)])
  lx = np.array([exact.step({'input_ids': tokens[i]}).item() for i in range(16)])
  assert (np.abs(lx - en['losses']) / en['losses']).max() <= 2e-6
  rel = np.abs(le - en['losses']) / en['losses']
  assert 1e-7 < rel.max() <= 1e-4, rel  # rounding is on (non-zero) and harmless (<= 1e-4), also after the updates


def test_reference_resumes_hip_checkpoint(golden_dir):
  """SURVEY section 8f N4, HipEngine -> reference: tests/golden/hip_ckpt_step_2.pth was written on an MI355X by HipEngine
  (test_engine_checkpoint_has_the_reference_layout); the REFERENCE engine resumed from it with engine/engine.py:56-60,86-89
  and its next 4 micro-step losses are stored in hip_ckpt_ref_resume.npz (tests/golden/check_hip_ckpt_with_reference.py).
  Those losses reproduce, within 1e-4, both HipEngine's own continuation and the continuation the reference got from its own
  checkpoint; and the CPU oracle engine, resumed from the same file through the reference's checkpoint layout (model
  state_dict, torch AdamW state in (decay, no-decay) group order, scheduler iter), reproduces the reference's losses."""
  z = np.load(os.path.join(golden_dir, 'ckpt.npz'))
  hip = np.load(os.path.join(golden_dir, 'hip_ckpt_cont.npz'))['losses']
  ref = np.load(os.path.join(golden_dir, 'hip_ckpt_ref_resume.npz'))['losses']
  own = z['losses'][4:]
  assert ref.shape == hip.shape == own.shape == (4,)
  assert (np.abs(ref - hip) / hip).max() <= 1e-4 and (np.abs(ref - own) / own).max() <= 1e-4
  ck = torch.load(os.path.join(golden_dir, 'hip_ckpt_step_2.pth'), map_location='cpu', weights_only=False)
  assert set(ck) == {'step', 'state_dict', 'optimizer', 'scheduler', 'scaler'} and ck['step'] == 2
  cfg = O.OracleConfig(vocab_size=128, seq_len=32, dim=64, n_layers=2, n_heads=1)
  names = list(ck['state_dict'])
  assert names == O.param_names(cfg)
  eng = O.OracleEngine(ck['state_dict'], cfg, lr=3e-3, weight_decay=0.1, beta1=0.9, beta2=0.95, grad_clip=1.0, accum=2,
                       steps_budget=8, warmup_steps=2)
  decay = O.decay_mask(names)
  order = [n for n in names if decay[n]] + [n for n in names if not decay[n]]
  groups = ck['optimizer']['param_groups']
  assert [g['weight_decay'] for g in groups] == [0.1, 0.0] and sum(len(g['params']) for g in groups) == len(order)
  for i, n in enumerate(order):
    st = ck['optimizer']['state'][i]
    assert st['exp_avg'].shape == eng.params[n].shape and int(st['step']) == 2, n
    eng.m[n], eng.v[n] = st['exp_avg'].clone(), st['exp_avg_sq'].clone()
  eng.opt_step = 2
  eng.sched_iter = ck['scheduler']['iter']
  eng.lr = O.warmup_cosine_lr(eng.sched_iter, 0.0, 3e-3, 1e-5, 2, 8)
  tok = torch.from_numpy(z['tokens'])
  got = np.array([eng.step({'input_ids': tok[i]}).item() for i in range(4, 8)])
  assert (np.abs(got - ref) / ref).max() <= 2e-6, (got, ref)


def test_lr_schedules_vs_reference(golden_dir):
  """The reference's four schedulers through its initialize_scheduler (optim/init_optim.py:73-137; fixture: tests/golden/make_schedules.py, the
  reference imported in the build container): the learning rate before the first step and after every step - integer and fractional warm-up /
  cool-down lengths, lr_end and lr_end_pct, steps past the budget - bit for bit, and the state_dict (it travels in checkpoints,
  checkpoint_utils.py:22-24) key for key.  LinearCooldown takes only `iter` from a saved state, like the reference's."""
  import json
  from types import SimpleNamespace
  from plainlm_amd import engine
  cases = json.load(open(os.path.join(golden_dir, 'schedules.json')))
  assert {c['cfg']['scheduler'] for c in cases} == {'warmup_cosine', 'warmup_constant', 'wsd', 'linear_cooldown'}
  for c in cases:
    cfg = SimpleNamespace(**{k: v for k, v in c['cfg'].items() if k != 'n'})
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=cfg.lr)
    sch = engine.initialize_scheduler(opt, cfg)
    lrs = [opt.param_groups[0]['lr']]
    for _ in range(c['cfg']['n']):
      sch.step()
      lrs.append(opt.param_groups[0]['lr'])
    assert lrs == c['lrs'], (c['cfg'], lrs, c['lrs'])
    assert sch.state_dict() == c['state'], (c['cfg'], sch.state_dict(), c['state'])
    # a fresh scheduler resumed from the saved state continues the sequence
    opt2 = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=cfg.lr)
    s2 = engine.initialize_scheduler(opt2, cfg)
    s2.load_state_dict(dict(c['state'], iter=3))
    s2.step()
    assert opt2.param_groups[0]['lr'] == c['lrs'][4], c['cfg']
  with pytest.raises(NotImplementedError):
    engine.initialize_scheduler(opt, SimpleNamespace(scheduler='one_cycle', warmup_steps=1, steps_budget=4, lr_end=None, lr_end_pct=None, lr=1.0, lr_start=0.0))
  assert engine.initialize_scheduler(opt, SimpleNamespace(scheduler=None)) is None
