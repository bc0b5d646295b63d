"""Optimizer tail on the gfx950 kernels (engine/engine.py:126-135, optim/init_optim.py:7-70).

``FlatAdamW`` is a ``torch.optim.AdamW`` subclass, so ``engine.optimizer`` keeps the reference's interface
(``param_groups`` with per-group ``lr`` written by the LR schedule, ``state_dict()`` / ``load_state_dict()`` in
torch's layout: per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq``), but

  * parameters, gradients and both moments live in flat fp32 buffers (one span per weight-decay group),
  * ``clip_and_step(max_norm)`` = one deterministic ||g||^2 reduction + one fused AdamW launch per group; the
    clip coefficient min(1, max_norm / (||g|| + 1e-6)) is computed on the device and folded into the AdamW
    kernel, so clipping costs no extra pass over the gradients and no host synchronisation.

Arithmetic matches ``torch.optim.AdamW`` (decoupled decay ``p *= 1 - lr*wd``; bias-corrected moments;
``denom = sqrt(v)/sqrt(bc2) + eps``) and ``torch.nn.utils.clip_grad_norm_``.

The reference's other optimizers get the same treatment (same layout, clip and shadow emission, torch-layout state):
``FlatNAdamW`` (``torch.optim.NAdam(decoupled_weight_decay=True)``: ``step`` / ``mu_product`` / ``exp_avg`` / ``exp_avg_sq``),
``FlatSGD`` (``torch.optim.SGD``, nesterov off: ``momentum_buffer``) and ``FlatSignSGD`` (``SignSGD`` below, the arithmetic of the
reference's optim/signSGD.py: ``m``).

Schedule-free AdamW (the reference's ``sfo_adamw``: ``schedulefree.AdamWScheduleFree``, Defazio et al. 2024) is restated here without the
package: ``AdamWScheduleFree`` in plain torch for ``fused_optim: False``, ``FlatAdamWScheduleFree`` on the flat buffers.  Both keep the
package's state layout (group keys ``k`` / ``weight_sum`` / ``lr_max`` / ``scheduled_lr`` / ``train_mode`` / ...; per parameter ``z`` /
``exp_avg_sq``, created at a parameter's first step) and its ``train()`` / ``eval()`` swaps of the parameters between y (where gradients
are taken) and the averaged iterate x (what is evaluated).

Muon (``torch.optim.Muon``'s arithmetic) is ``Muon`` in plain torch and ``FlatMuon`` on the flat buffers: the weights
of the block linears take the Newton-Schulz update (prepare -> orthogonalize -> apply on the batched NT GEMM), every other parameter
takes AdamW in the same object, so the engine keeps one ``param_groups``.
"""

import os

import torch

from . import ops


class SignSGD(torch.optim.Optimizer):
  """signSGD / signum with the reference's arithmetic (optim/signSGD.py), per parameter and step:
  ``p *= 1 - lr*wd``; ``m`` starts as a copy of the first gradient and is then updated ``m = momentum*m + (1 - dampening)*g``
  on every step, the first one included (so the first ``m`` is ``(momentum + 1 - dampening)*g``); ``p -= lr*sign(m)``.
  State: ``m`` per parameter (no ``step``).  Parameters without a gradient are skipped."""

  def __init__(self, params, lr, momentum=0.0, dampening=0.0, weight_decay=0.1):
    for name, val, hi in (('learning rate', lr, None), ('momentum', momentum, 1.0), ('dampening', dampening, 1.0),
                          ('weight decay', weight_decay, None)):
      if not (val >= 0.0 and (hi is None or val <= hi)):
        raise ValueError(f'SignSGD: invalid {name}: {val}')
    super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay))

  @torch.no_grad()
  def step(self, closure=None):
    loss = None
    if closure is not None:
      with torch.enable_grad():
        loss = closure()
    for group in self.param_groups:
      lr, mom, damp, wd = group['lr'], group['momentum'], group['dampening'], group['weight_decay']
      for p in group['params']:
        if p.grad is None:
          continue
        st = self.state[p]
        p.mul_(1 - lr * wd)
        if 'm' not in st:
          st['m'] = p.grad.detach().clone()
        m = st['m']
        m.mul_(mom).add_(p.grad, alpha=1.0 - damp)
        p.add_(m.sign(), alpha=-lr)
    return loss


def _sfo_defaults(lr, betas, eps, weight_decay, warmup_steps, r, weight_lr_power):
  if not lr >= 0.0 or not eps >= 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
    raise ValueError(f'AdamWScheduleFree: invalid lr={lr} / eps={eps} / betas={betas}')
  if betas[0] == 0.0:
    raise ValueError('AdamWScheduleFree: beta1 = 0 has no averaged iterate to evaluate (eval() divides by beta1)')
  return dict(lr=lr, betas=tuple(betas), eps=eps, r=r, k=0, warmup_steps=warmup_steps, train_mode=True, weight_sum=0.0, lr_max=-1.0,
              scheduled_lr=0.0, weight_lr_power=weight_lr_power, weight_decay=weight_decay)


class AdamWScheduleFree(torch.optim.Optimizer):
  """Schedule-free AdamW with the arithmetic and state layout of ``schedulefree.AdamWScheduleFree`` (its defaults: eps 1e-8, r 0,
  weight_lr_power 2), in the y-only form: the parameters hold y, ``z`` and ``exp_avg_sq`` are per-parameter state, x is never stored.
  Per group and step the host forms (ops.sfo_scalars) the warmed-up lr, ckp1 = weight / weight_sum and bc2; per parameter
  ``v = b2 v + (1-b2) g^2``, ``gn = g / (sqrt(v / bc2) + eps) + wd y``, ``y = lerp(y, z, ckp1) + lr (b1 (1 - ckp1) - 1) gn``,
  ``z -= lr gn``.  ``eval()`` moves the parameters to x (``p.lerp_(z, 1 - 1/b1)``), ``train()`` back to y (``p.lerp_(z, 1 - b1)``);
  ``step()`` refuses to run in eval mode.  Unlike the package, ``p.grad`` is left as it was."""

  def __init__(self, params, lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, warmup_steps=0, r=0.0, weight_lr_power=2.0):
    super().__init__(params, _sfo_defaults(lr, betas, eps, weight_decay, warmup_steps, r, weight_lr_power))

  @torch.no_grad()
  def _swap(self, to_train):
    for group in self.param_groups:
      if group['train_mode'] == to_train:
        continue
      b1 = group['betas'][0]
      w = 1.0 - b1 if to_train else 1.0 - 1.0 / b1
      for p in group['params']:
        st = self.state.get(p)
        if st and 'z' in st:
          p.lerp_(st['z'], w)
      group['train_mode'] = to_train

  def eval(self):
    self._swap(False)

  def train(self):
    self._swap(True)

  @torch.no_grad()
  def step(self, closure=None):
    if not all(g['train_mode'] for g in self.param_groups):
      raise RuntimeError('AdamWScheduleFree: step() called in eval mode; call optimizer.train() first')
    loss = None
    if closure is not None:
      with torch.enable_grad():
        loss = closure()
    for group in self.param_groups:
      lr, ckp1, bc2 = ops.sfo_scalars(group)
      b1, b2 = group['betas']
      eps, wd = group['eps'], group['weight_decay']
      for p in group['params']:
        if p.grad is None:
          continue
        st = self.state[p]
        if 'z' not in st:
          st['z'] = p.detach().clone()
          st['exp_avg_sq'] = torch.zeros_like(p)
        z, v = st['z'], st['exp_avg_sq']
        v.mul_(b2).addcmul_(p.grad, p.grad, value=1.0 - b2)
        gn = p.grad / v.div(bc2).sqrt_().add_(eps)
        if wd != 0:
          gn.add_(p, alpha=wd)
        p.lerp_(z, ckp1)
        p.add_(gn, alpha=lr * (b1 * (1.0 - ckp1) - 1.0))
        z.sub_(gn, alpha=lr)
    return loss


def newton_schulz(u, steps=5, coefficients=ops.MUON_NS_COEFFICIENTS, eps=ops.MUON_EPS):
  """torch.optim._muon._zeropower_via_newtonschulz restated: bf16(u), on the transpose when tall, divided by its (bf16) norm clamped at
  eps, then ``steps`` times A = X X^T ; Bm = b A + c A A ; X = a X + Bm X in bf16 matmuls; transposed back."""
  a, b, c = coefficients
  x = u.bfloat16()
  tall = u.size(0) > u.size(1)
  if tall:
    x = x.T
  x = x / x.norm().clamp(min=eps)
  for _ in range(steps):
    gram = x @ x.T
    upd = torch.addmm(gram, gram, gram, beta=b, alpha=c)
    x = torch.addmm(x, upd, x, beta=a)
  return x.T if tall else x


def muon_param_groups(model, param_groups):
  """[muon (decay), adamw decay, adamw no-decay] from the two groups of construct.get_param_groups: the Muon group holds the weight of
  every HipLinear inside model.layers (the four block linears of a layer, whole: w_qkv and a GLU fc1 are not split); embed_tokens,
  lm_head (tied or not) and the norm weights stay with AdamW."""
  from .transformer import HipLinear
  decay, no_decay = param_groups
  ids = {id(m.weight) for layer in model.layers for m in layer.modules() if isinstance(m, HipLinear)}
  outside = {id(m.weight) for n, m in model.named_modules() if isinstance(m, HipLinear) and not n.startswith('layers.')}
  ids -= outside  # a weight shared with a module outside the blocks is not a block matrix
  muon = [p for p in decay['params'] if id(p) in ids]
  if len(muon) != len(ids):
    raise ValueError('muon_param_groups: a block linear weight is missing from the weight-decay group')
  rest = [p for p in decay['params'] if id(p) not in ids]
  return [{'params': muon, 'weight_decay': decay['weight_decay'], 'use_muon': True},
          {'params': rest, 'weight_decay': decay['weight_decay'], 'use_muon': False},
          {'params': list(no_decay['params']), 'weight_decay': no_decay['weight_decay'], 'use_muon': False}]


class Muon(torch.optim.Optimizer):
  """Muon for the groups with ``use_muon=True`` (2-D parameters only), AdamW for the others, in one optimizer.  Per Muon parameter and
  step, the arithmetic of torch.optim._muon._single_tensor_muon: ``buf.lerp_(g, 1 - momentum)``; ``u = g.lerp(buf, momentum)`` with
  nesterov, else buf; ``o = newton_schulz(u)``; ``p *= 1 - lr*wd``; ``p -= lr_adj * o`` with lr_adj = lr * 0.2 sqrt(max(rows, cols))
  ('match_rms_adamw', the default here: the schedule writes ONE lr into every group, and with this adjustment the matrices share
  AdamW's lr and weight decay) or lr * sqrt(max(1, rows / cols)) ('original').  State: ``momentum_buffer``, created at the first step.
  The other groups take torch.optim.AdamW's single-tensor arithmetic (state ``step`` / ``exp_avg`` / ``exp_avg_sq``)."""

  def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1, momentum=0.95, nesterov=True, ns_steps=5,
               adjust_lr='match_rms_adamw', ns_coefficients=ops.MUON_NS_COEFFICIENTS, muon_eps=ops.MUON_EPS):
    if not lr >= 0.0 or not eps >= 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or not weight_decay >= 0.0:
      raise ValueError(f'Muon: invalid lr={lr} / eps={eps} / betas={betas} / weight_decay={weight_decay}')
    if not 0.0 <= momentum < 1.0:
      raise ValueError(f'Muon: momentum={momentum} must lie in [0, 1)')
    if int(ns_steps) != ns_steps or not 1 <= ns_steps < 100:
      raise ValueError(f'Muon: ns_steps={ns_steps} must be an integer in 1..99')
    if adjust_lr not in ops.MUON_ADJUST_LR:
      raise ValueError(f'Muon: muon_adjust_lr {adjust_lr!r} is not one of {ops.MUON_ADJUST_LR}')
    if len(ns_coefficients) != 3:
      raise ValueError('Muon: ns_coefficients must be three values')
    super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, momentum=momentum, nesterov=bool(nesterov),
                                  ns_steps=int(ns_steps), adjust_lr=adjust_lr, ns_coefficients=tuple(ns_coefficients), muon_eps=muon_eps,
                                  use_muon=False))
    for g in self.param_groups:
      if g['use_muon'] and any(p.ndim != 2 for p in g['params']):
        raise ValueError('Muon: a use_muon group holds a parameter that is not 2-D')

  @torch.no_grad()
  def step(self, closure=None):
    loss = None
    if closure is not None:
      with torch.enable_grad():
        loss = closure()
    for group in self.param_groups:
      lr, wd = group['lr'], group['weight_decay']
      for p in group['params']:
        if p.grad is None:
          continue
        st = self.state[p]
        if group['use_muon']:
          if 'momentum_buffer' not in st:
            st['momentum_buffer'] = torch.zeros_like(p.grad)
          buf, mom = st['momentum_buffer'], group['momentum']
          buf.lerp_(p.grad, 1 - mom)
          u = p.grad.lerp(buf, mom) if group['nesterov'] else buf
          o = newton_schulz(u, group['ns_steps'], group['ns_coefficients'], group['muon_eps'])
          p.mul_(1 - lr * wd)
          p.add_(o, alpha=-ops.muon_adjusted_lr(lr, group['adjust_lr'], p.shape[0], p.shape[1]))
          continue
        if 'step' not in st:
          st['step'] = torch.tensor(0.0)
          st['exp_avg'] = torch.zeros_like(p)
          st['exp_avg_sq'] = torch.zeros_like(p)
        b1, b2 = group['betas']
        st['step'] += 1
        t = float(st['step'])
        m, v = st['exp_avg'], st['exp_avg_sq']
        p.mul_(1 - lr * wd)
        m.lerp_(p.grad, 1 - b1)
        v.mul_(b2).addcmul_(p.grad, p.grad, value=1 - b2)
        denom = (v.sqrt() / (1 - b2 ** t) ** 0.5).add_(group['eps'])
        p.addcdiv_(m, denom, value=-(lr / (1 - b1 ** t)))
    return loss


class _FlatTail:
  """What every flat optimizer shares, mixed in front of its torch class: the flat re-layout of parameters, gradients and state
  buffers (one span per parameter group), the model's gradient span table, the shadow-emitting launch plan, ``clip_and_step``,
  ``step`` and ``zero_grad``.  Subclasses name their per-parameter state buffers (``_state_names``, torch's keys) and implement
  ``_group_hparams`` / ``_publish_state`` / ``_restore_host_state``."""

  _state_names = ()

  def _lay_out(self, model):
    if getattr(model, '_flat_grad', None) is None:
      raise RuntimeError(f'{type(self).__name__} needs model.enable_main_grad() first (flat gradient buffer)')
    self.model = model
    dev = model._flat_grad.device
    # Re-lay parameters and gradients group by group so that every group is ONE contiguous span.
    order = [p for g in self.param_groups for p in g['params']]
    if len({id(p) for p in order}) != len(list(model.parameters())):
      raise ValueError('param_groups must cover every model parameter exactly once')
    total = sum(p.numel() for p in order)
    self.flat_p = torch.empty(total, dtype=torch.float32, device=dev)
    # state buffers, padded to two (the kernels' m and v; None where the optimizer has no such buffer)
    bufs = [torch.zeros(total, dtype=torch.float32, device=dev) for _ in self._state_names]
    self._state_bufs = bufs + [None] * (2 - len(bufs))
    self.flat_g = model._flat_grad
    if self.flat_g.numel() != total:
      raise ValueError('flat gradient buffer does not match the parameter groups')
    self.group_spans = [None] * len(self.param_groups)
    self._views = {}
    off = 0
    spans_by_param = {}
    # Placement: zero-weight-decay groups (the norm weights, 77 KB at 160M) FIRST, so that the flat buffer reads
    # [norms | embed_tokens | layer 0 ... | lm_head]: ddp.plan_buckets walks it from the end (= the order gradients become
    # ready) and the norm weights - complete only when layer 0 has been differentiated - share the LAST bucket with
    # embed_tokens instead of holding up lm_head's.  param_groups keeps the reference's order (decay, no-decay): only the
    # placement changes, optimizer.state_dict() does not.
    placement = sorted(range(len(self.param_groups)), key=lambda i: (self.param_groups[i]['weight_decay'] != 0.0, i))
    for gi in placement:
      g = self.param_groups[gi]
      lo = off
      for p in g['params']:
        n = p.numel()
        self.flat_p[off:off + n].copy_(p.data.reshape(-1))
        p.data = self.flat_p[off:off + n].view(p.shape)
        p.main_grad = self.flat_g[off:off + n].view(p.shape)
        spans_by_param[id(p)] = (off, n)
        self._views[id(p)] = tuple(b[off:off + n].view(p.shape) if b is not None else None for b in self._state_bufs)
        off += n
      self.group_spans[gi] = (lo, off)
    # the model's span table (used by the gradient reducer) follows parameters() order
    model._grad_spans = [spans_by_param[id(p)] for p in model.parameters()]
    model.invalidate_shadows()
    self._scratch = torch.empty(4096, dtype=torch.float32, device=dev)
    self._step_count = 0
    self.last_grad_norm = None
    # SURVEY section 8f N1, second half: the Linear weights' update also writes their bf16 shadows (W and W^T), so the training step has
    # no stand-alone weight cast (what autocast does per forward, engine/engine.py:75).  Per weight-decay group: the Linear weights
    # of the group (one fused launch) + the rest of its span (embed_tokens / the norm weights: flat kernel).  PLM_ADAMW_SHADOWS=0
    # restores the flat kernel for everything + invalidated shadows.
    self.emits_shadows = os.environ.get('PLM_ADAMW_SHADOWS', '1') != '0' and hasattr(model, 'linear_modules')
    self._fused = [None] * len(self.param_groups)  # per group: (linear modules, item tensors, ctypes table or None, leftover [(lo, hi)])
    if self.emits_shadows:
      for gi, g in enumerate(self.param_groups):
        ids = {id(p) for p in g['params']}
        lins = [m for m in model.linear_modules() if id(m.weight) in ids]
        if not lins:
          continue
        items, taken = [], []
        for lin in lins:
          w = lin.weight
          lin.stale_item()  # allocates the shadow buffers
          items.append(self._item(lin))
          taken.append(spans_by_param[id(w)])
        lo, hi = self.group_spans[gi]
        rest, cur = [], lo
        for o, n in sorted(taken):
          if o > cur:
            rest.append((cur, o))
          cur = o + n
        if cur < hi:
          rest.append((cur, hi))
        self._fused[gi] = (lins, items, None, rest)

  def _item(self, lin):
    return (lin.weight.data, lin.weight.main_grad) + self._views[id(lin.weight)] + (lin._shadow[0], lin._shadow[1])

  def _after_step(self):
    self._publish_state()

  def _check_step(self):
    pass

  def _step_group(self, gi, g, lo, hi, clip, fresh):
    """One group's update: the shadow-emitting launch over its Linear weights, the flat kernel over the rest of its span; the linears
    whose shadows this step has written are appended to ``fresh``."""
    hp = self._group_hparams(gi, g)
    spans = [(lo, hi)]
    if self._fused[gi] is not None:
      lins, items, table, spans = self._fused[gi]
      if any(lin._shadow[0] is not it[4] or lin.weight.data_ptr() != it[0].data_ptr() for lin, it in zip(lins, items)):
        # a shadow buffer or a weight was re-allocated behind our back (model moved, weights re-laid): rebuild the cached table
        items = [self._item(lin) for lin in lins]
        table = None
      table = ops.optim_cast_multi_(hp, items, clip, table)
      self._fused[gi] = (lins, items, table, spans)
      fresh.extend(lins)
    for a, b in spans:
      m, v = (t[a:b] if t is not None else None for t in self._state_bufs)
      ops.optim_(hp, self.flat_p[a:b], self.flat_g[a:b], m, v, clip)

  @torch.no_grad()
  def clip_and_step(self, max_norm=None):
    self._check_step()
    if getattr(self.model, 'sink', None) is not None:
      self.model.sink.flush_dw()  # queued weight-gradient GEMMs (functional.GradSink) must have been issued
    self._step_count += 1
    clip = None
    if max_norm:
      sq = ops.sumsq(self.flat_g, self._scratch)
      self.last_grad_norm = torch.sqrt(sq)
      clip = torch.clamp(float(max_norm) / (self.last_grad_norm + 1e-6), max=1.0).reshape(1).contiguous()
    fresh = []
    for gi, (g, (lo, hi)) in enumerate(zip(self.param_groups, self.group_spans)):
      if hi > lo:
        self._step_group(gi, g, lo, hi, clip, fresh)
    self._after_step()
    self.model.invalidate_shadows()  # raw-pointer update: torch's version counters did not move
    for lin in fresh:                # ... except where this step has just written the shadows itself
      lin.mark_fresh()

  @torch.no_grad()
  def step(self, closure=None):
    if closure is not None:
      raise NotImplementedError(f'{type(self).__name__}.step does not take a closure')
    self.clip_and_step(None)

  def zero_grad(self, set_to_none=True):
    # gradients live in the flat buffer and are overwritten by the first write of the next window
    for g in self.param_groups:
      for p in g['params']:
        p.grad = None

  def load_state_dict(self, state_dict):
    super().load_state_dict(state_dict)
    steps = []
    for gi, g in enumerate(self.param_groups):
      states = [self.state.get(p) or {} for p in g['params']]
      for p, st in zip(g['params'], states):
        for name, view in zip(self._group_state_names(gi), self._views[id(p)]):
          if name in st:
            view.copy_(st[name])
        if 'step' in st:
          steps.append(int(float(st['step'])))
      self._restore_host_state(gi, states)
    self._step_count = max(steps) if steps else 0
    self._publish_state()

  def _restore_host_state(self, gi, states):
    pass

  def _group_state_names(self, gi):
    """torch's keys of group gi's state buffers (FlatMuon: its Muon group keeps momentum_buffer where the others keep exp_avg)."""
    return self._state_names


class FlatAdamW(_FlatTail, torch.optim.AdamW):
  _state_names = ('exp_avg', 'exp_avg_sq')

  def __init__(self, model, param_groups, lr, betas, eps, weight_decay):
    torch.optim.AdamW.__init__(self, param_groups, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, fused=False, foreach=False)
    self._lay_out(model)
    self.flat_m, self.flat_v = self._state_bufs
    self._publish_state()

  def _publish_state(self):
    """torch-layout per-parameter state backed by views of the flat moment buffers."""
    for g in self.param_groups:
      for p in g['params']:
        m, v = self._views[id(p)]
        self.state[p] = {'step': torch.tensor(float(self._step_count)), 'exp_avg': m, 'exp_avg_sq': v}

  def _group_hparams(self, gi, g):
    b1, b2 = g['betas']
    return ops.optim_hparams('adamw', float(g['lr']), g['weight_decay'], beta1=b1, beta2=b2, eps=g['eps'],
                             bc1=1.0 - b1 ** self._step_count, bc2=1.0 - b2 ** self._step_count)

  def _after_step(self):
    for st in self.state.values():
      st['step'].fill_(float(self._step_count))


class FlatNAdamW(_FlatTail, torch.optim.NAdam):
  """torch.optim.NAdam(decoupled_weight_decay=True) on the flat buffers.  The product of the momentum cache (``mu_product``) is kept per
  group on the host in fp64 (torch: an fp32 tensor per parameter, so the two agree to rounding) and published per parameter."""
  _state_names = ('exp_avg', 'exp_avg_sq')

  def __init__(self, model, param_groups, lr, betas, eps, weight_decay, momentum_decay=4e-3):
    torch.optim.NAdam.__init__(self, param_groups, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                               momentum_decay=momentum_decay, decoupled_weight_decay=True, foreach=False)
    self._lay_out(model)
    self.flat_m, self.flat_v = self._state_bufs
    self._mu_product = [1.0] * len(self.param_groups)
    self._publish_state()

  def _publish_state(self):
    for gi, g in enumerate(self.param_groups):
      for p in g['params']:
        m, v = self._views[id(p)]
        self.state[p] = {'step': torch.tensor(float(self._step_count)), 'mu_product': torch.tensor(self._mu_product[gi]),
                         'exp_avg': m, 'exp_avg_sq': v}

  def _group_hparams(self, gi, g):
    if not g.get('decoupled_weight_decay', True) or g.get('maximize', False):
      raise NotImplementedError('FlatNAdamW implements decoupled weight decay and maximize=False only')
    b1, b2 = g['betas']
    lr = float(g['lr'])
    bc2, cg, cm, self._mu_product[gi] = ops.nadam_scalars(lr, b1, b2, g['momentum_decay'], self._step_count, self._mu_product[gi])
    return ops.optim_hparams('nadamw', lr, g['weight_decay'], beta1=b1, beta2=b2, eps=g['eps'], bc2=bc2, coef_grad=cg, coef_avg=cm)

  def _restore_host_state(self, gi, states):
    st = next((s for s in states if 'mu_product' in s), None)
    self._mu_product[gi] = float(st['mu_product']) if st else 1.0


class _FlatMomentum(_FlatTail):
  """SGD / signSGD: one state buffer per parameter that torch creates at a parameter's first step (no ``step`` key), so the state dict
  holds it only for groups that have stepped; ``_primed[gi]`` is the kernels' ``first`` flag, negated."""
  _kind = None

  def _init_flat(self, model):
    self._lay_out(model)
    self.flat_m, self.flat_v = self._state_bufs
    self._primed = [False] * len(self.param_groups)
    self._publish_state()

  def _has_buffer(self, g):
    return True

  def _publish_state(self):
    (name,) = self._state_names
    for gi, g in enumerate(self.param_groups):
      for p in g['params']:
        if self._primed[gi]:
          self.state[p] = {name: self._views[id(p)][0]}
        else:
          self.state.pop(p, None)

  def _group_hparams(self, gi, g):
    lr = float(g['lr'])
    hp = ops.optim_hparams(self._kind, lr, g['weight_decay'], first=not self._primed[gi], momentum=g['momentum'], dampening=g['dampening'])
    self._primed[gi] = self._primed[gi] or self._has_buffer(g)
    return hp

  def _restore_host_state(self, gi, states):
    (name,) = self._state_names
    have = [name in s for s in states]
    if any(have) and not all(have):
      raise ValueError(f'{type(self).__name__}: the state dict holds {name} for some parameters of group {gi} but not all')
    self._primed[gi] = bool(have) and all(have)


class FlatSGD(_FlatMomentum, torch.optim.SGD):
  """torch.optim.SGD (coupled L2 decay, momentum with dampening, nesterov off) on the flat buffers."""
  _state_names = ('momentum_buffer',)
  _kind = 'sgd'

  def __init__(self, model, param_groups, lr, momentum, dampening, weight_decay):
    torch.optim.SGD.__init__(self, param_groups, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, foreach=False)
    self._init_flat(model)

  def _has_buffer(self, g):
    return g['momentum'] != 0  # torch keeps no momentum_buffer without momentum

  def _group_hparams(self, gi, g):
    if g.get('nesterov', False) or g.get('maximize', False):
      raise NotImplementedError('FlatSGD implements nesterov=False, maximize=False only')
    return super()._group_hparams(gi, g)


class FlatSignSGD(_FlatMomentum, SignSGD):
  """SignSGD on the flat buffers."""
  _state_names = ('m',)
  _kind = 'signSGD'

  def __init__(self, model, param_groups, lr, momentum, dampening, weight_decay):
    SignSGD.__init__(self, param_groups, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay)
    self._init_flat(model)


class FlatAdamWScheduleFree(_FlatTail, AdamWScheduleFree):
  """AdamWScheduleFree on the flat buffers: the flat parameters hold y, the kernels' m / v slots carry z / exp_avg_sq.  The per-group
  host scalars (k, weight_sum, lr_max: Python floats, i.e. fp64, as the package keeps them) live in param_groups and travel with
  state_dict(); z / exp_avg_sq are published as views of the flat buffers once a group has stepped (``_primed``; its first step makes z a
  copy of y inside the update launch).  ``train()`` / ``eval()`` lerp each stepped group's span toward z (ops.lerp_) and invalidate the
  bf16 shadows, which the next forward re-casts."""
  _state_names = ('z', 'exp_avg_sq')

  def __init__(self, model, param_groups, lr, betas, weight_decay, warmup_steps=0, eps=1e-8, r=0.0, weight_lr_power=2.0):
    AdamWScheduleFree.__init__(self, param_groups, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                               warmup_steps=warmup_steps, r=r, weight_lr_power=weight_lr_power)
    self._lay_out(model)
    self.flat_z, self.flat_v = self._state_bufs
    self._primed = [False] * len(self.param_groups)
    self._publish_state()

  def _publish_state(self):
    for gi, g in enumerate(self.param_groups):
      for p in g['params']:
        if self._primed[gi]:
          z, v = self._views[id(p)]
          self.state[p] = {'z': z, 'exp_avg_sq': v}
        else:
          self.state.pop(p, None)

  def _check_step(self):
    if not all(g['train_mode'] for g in self.param_groups):
      raise RuntimeError('FlatAdamWScheduleFree: step() called in eval mode; call optimizer.train() first')

  def _group_hparams(self, gi, g):
    lr, ckp1, bc2 = ops.sfo_scalars(g)
    b1, b2 = g['betas']
    hp = ops.optim_hparams('sfo_adamw', lr, g['weight_decay'], first=not self._primed[gi], beta1=b1, beta2=b2, eps=g['eps'], bc2=bc2,
                           ckp1=ckp1)
    self._primed[gi] = True
    return hp

  @torch.no_grad()
  def _swap(self, to_train):
    moved = False
    for gi, (g, (lo, hi)) in enumerate(zip(self.param_groups, self.group_spans)):
      if g['train_mode'] == to_train:
        continue
      if self._primed[gi] and hi > lo:
        b1 = g['betas'][0]
        ops.lerp_(self.flat_p[lo:hi], self.flat_z[lo:hi], 1.0 - b1 if to_train else 1.0 - 1.0 / b1)
        moved = True
      g['train_mode'] = to_train
    if moved:
      self.model.invalidate_shadows()  # raw-pointer update; the next forward re-casts them

  def load_state_dict(self, state_dict):
    super().load_state_dict(state_dict)
    for g in self.param_groups:
      g['k'] = int(g['k'])
      g['weight_sum'], g['lr_max'], g['scheduled_lr'] = float(g['weight_sum']), float(g['lr_max']), float(g['scheduled_lr'])
      g['train_mode'] = bool(g['train_mode'])
    self._step_count = max(g['k'] for g in self.param_groups)

  def _restore_host_state(self, gi, states):
    have = ['z' in s and 'exp_avg_sq' in s for s in states]
    if any(have) and not all(have):
      raise ValueError(f'FlatAdamWScheduleFree: the state dict holds z / exp_avg_sq for some parameters of group {gi} but not all')
    self._primed[gi] = bool(have) and all(have)


class FlatMuon(_FlatTail, Muon):
  """Muon on the flat buffers.  State buffer 0 is ``momentum_buffer`` on the Muon group's span and ``exp_avg`` elsewhere, buffer 1 is
  ``exp_avg_sq`` (unused on the Muon span).  ``clip_and_step`` runs the AdamW groups exactly as FlatAdamW does (the PLM_OPTIM_ADAMW
  kernels, the shadow-emitting launch for an untied lm_head), and the Muon group through ops.muon_prepare -> ops.muon_orthogonalize ->
  ops.muon_apply on one workspace (the stream's arena); apply writes the block linears' bf16 shadows, which are marked fresh."""
  _state_names = ('exp_avg', 'exp_avg_sq')

  def __init__(self, model, param_groups, lr, betas, eps, weight_decay, momentum=0.95, nesterov=True, ns_steps=5,
               adjust_lr='match_rms_adamw'):
    Muon.__init__(self, param_groups, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov,
                  ns_steps=ns_steps, adjust_lr=adjust_lr)
    self._lay_out(model)
    self.flat_m, self.flat_v = self._state_bufs
    by_weight = {id(m.weight): m for m in model.linear_modules()}
    self._muon = {}  # group index -> [linears, ctypes item table, shapes, (weight, shadow) pointers the table was built from]
    for gi, g in enumerate(self.param_groups):
      if g['use_muon'] and g['params']:
        lins = [by_weight[id(p)] for p in g['params']]
        for lin in lins:
          lin.stale_item()  # allocates the shadow buffers
        self._muon[gi] = [lins, None, None, None]
    self._muon_nrm = torch.zeros(max([len(v[0]) for v in self._muon.values()] + [1]), dtype=torch.float32, device=self.flat_p.device)
    self._publish_state()

  def _group_state_names(self, gi):
    return ('momentum_buffer',) if self.param_groups[gi]['use_muon'] else self._state_names

  def _publish_state(self):
    for g in self.param_groups:
      for p in g['params']:
        m, v = self._views[id(p)]
        if g['use_muon']:
          self.state[p] = {'momentum_buffer': m}
        else:
          self.state[p] = {'step': torch.tensor(float(self._step_count)), 'exp_avg': m, 'exp_avg_sq': v}

  def _after_step(self):
    for st in self.state.values():
      if 'step' in st:
        st['step'].fill_(float(self._step_count))

  def _group_hparams(self, gi, g):
    b1, b2 = g['betas']
    return ops.optim_hparams('adamw', float(g['lr']), g['weight_decay'], beta1=b1, beta2=b2, eps=g['eps'],
                             bc1=1.0 - b1 ** self._step_count, bc2=1.0 - b2 ** self._step_count)

  def _step_group(self, gi, g, lo, hi, clip, fresh):
    if not g['use_muon']:
      return super()._step_group(gi, g, lo, hi, clip, fresh)
    lins, table, shapes, key = self._muon[gi]
    now = [(lin.weight.data_ptr(), lin._shadow[0].data_ptr(), lin._shadow[1].data_ptr()) for lin in lins]
    if table is None or now != key:  # first step, or a weight / shadow buffer was re-allocated behind our back
      table, shapes = ops.muon_items([(lin.weight.data, lin.weight.main_grad, self._views[id(lin.weight)][0], lin._shadow[0], lin._shadow[1])
                                      for lin in lins])
      self._muon[gi] = [lins, table, shapes, now]
    lr = float(g['lr'])
    ops.muon_set_lr(table, [ops.muon_adjusted_lr(lr, g['adjust_lr'], r, c) for r, c in shapes])
    dev = self.flat_p.device
    ws = ops.muon_arena(shapes, dev)
    ops.muon_prepare(table, shapes, g['momentum'], g['nesterov'], self._muon_nrm, clip, eps=g['muon_eps'], workspace=ws)
    ops.muon_orthogonalize(shapes, g['ns_steps'], dev, g['ns_coefficients'], workspace=ws)
    ops.muon_apply(table, shapes, 1.0 - lr * g['weight_decay'], g['ns_steps'], dev, workspace=ws)
    fresh.extend(lins)
