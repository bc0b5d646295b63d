"""``construct_model`` / ``get_param_groups`` with the reference's call signatures
(models/construct.py:5-75), building the gfx950-native Transformer."""

from fractions import Fraction

from .generate import check_kv_dtype
from .transformer import ModelConfig, Transformer, check_attn_mask_mode, check_linear_precision


def construct_model(cfg):
  """cfg: any object with the reference's YAML keys (model, vocab_size, d_model, expand,
  n_layers, n_heads, mlp_class, seq_len, tie_embeddings), plus the optional ``attn_mask_mode`` ('doc', the default, or 'dense') and
  ``linear_precision`` ('bf16', the default, or 'mxfp8') and ``kv_cache`` ('bf16', the default, or 'fp8'): see ModelConfig.  None of the three
  keys is in the reference.  Returns (model, model_cfg)."""
  if cfg.model != 'transformer':
    raise NotImplementedError(
      f"model '{cfg.model}' is outside the accelerated hot path (only 'transformer'; the Pythia/HF branch is not built)")
  attn_mask_mode = check_attn_mask_mode(getattr(cfg, 'attn_mask_mode', 'doc'))
  linear_precision = check_linear_precision(getattr(cfg, 'linear_precision', 'bf16'))
  kv_cache = check_kv_dtype(getattr(cfg, 'kv_cache', 'bf16'))
  model_cfg = ModelConfig(
    vocab_size=cfg.vocab_size,
    dim=cfg.d_model,
    expand=float(Fraction(cfg.expand)),
    n_layers=cfg.n_layers,
    n_heads=cfg.n_heads,
    rmsnorm_eps=1e-6,
    mlp=cfg.mlp_class,
    seq_len=cfg.seq_len,
    tie_embeddings=cfg.tie_embeddings,
    attn_mask_mode=attn_mask_mode,
    linear_precision=linear_precision,
    kv_cache=kv_cache,
  )
  model = Transformer(model_cfg)
  print(f'Number of parameters: {model.count_params(non_embedding=False):_}')
  print(f'Number of non-embedding parameters: {model.count_params(non_embedding=True):_}')
  return model, model_cfg


def get_param_groups(model, weight_decay):
  """Decay group = parameters whose name contains neither 'bias' nor 'norm'
  (models/construct.py:54-58); everything else gets weight_decay 0."""
  named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
  decay, no_decay = [], []
  for n, p in named:
    skip = getattr(p, '_no_weight_decay', False) or 'bias' in n or 'norm' in n
    (no_decay if skip else decay).append(p)
  return [
    {'params': decay, 'weight_decay': weight_decay},
    {'params': no_decay, 'weight_decay': 0.0},
  ]
