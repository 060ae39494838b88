"""Build one shard's model: the sequence every engine and ring stage runs."""
from __future__ import annotations

from pathlib import Path

import torch
import torch.nn as nn

from xotorch_amd.models import model_class_for
from xotorch_amd.models.weights import fast_random_init_gpu, load_shard_weights, random_init


def build_shard_model(cfg, shard, dtype, device, model_dir=None, seed: int = 1234,
                      fast_init: bool = False) -> nn.Module:
  """The decoder for `cfg` holding `shard`'s layers, in eval mode on `device`.
  Weights come from the safetensors under `model_dir` when one is given,
  else from the seeded random init (fast_init: drawn on the GPU for models
  of dim >= 2048, where the per-parameter CPU draw takes minutes). Decode
  weight prepacking is the caller's: its reserve depends on what else the
  caller allocates."""
  # construct at the target dtype so to_empty materializes it directly
  # (fp32-then-cast would peak at 2x the weight bytes and leave the
  # allocator's reserved pool at that level)
  prev_dtype = torch.get_default_dtype()
  torch.set_default_dtype(dtype)
  try:
    with torch.device("meta"):
      model = model_class_for(cfg)(cfg, shard)
  finally:
    torch.set_default_dtype(prev_dtype)
  model = model.to_empty(device=device).to(dtype)
  if model_dir:
    load_shard_weights(model, Path(model_dir), device="cpu")  # raises when it finds none
    model = model.to(device)
  elif fast_init and device == "cuda" and cfg.dim >= 2048:
    fast_random_init_gpu(model, seed)
  else:
    random_init(model, seed)
  model.reset_rope()  # to_empty left the tables uninitialized
  return model.eval()
