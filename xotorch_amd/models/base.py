"""What the three decoder shells (llama / gemma2 / deepseek) share: shard
bookkeeping, the fp32 RoPE tables, and the entry and exit of forward.
Layers, norm and head parameters, embed scaling, logit soft-capping and the
carried norm stay in the subclasses."""
from __future__ import annotations

import os
from typing import List

import torch
import torch.nn as nn

from xotorch_amd.engine.kvcache import LayerKV
from xotorch_amd.models.config import ModelConfig
from xotorch_amd.ops.torch_ref import rope_cos_sin
from xotorch_amd.shard import Shard


class ShardBase(nn.Module):
  """The layer range [shard.start_layer .. shard.end_layer] of one model.
  Subclasses register `layers`, then their norm and head, after this
  constructor (parameter order: embed_tokens, layers, norm, lm_head)."""

  def __init__(self, cfg: ModelConfig, shard: Shard, rope_dim: int):
    super().__init__()
    self.cfg = cfg
    self.shard = shard
    self.rope_dim = rope_dim
    if shard.is_first_layer:
      self.embed_tokens = nn.Embedding(cfg.vocab_size, cfg.dim)
    cos, sin = rope_cos_sin(rope_dim, cfg.max_seq_len, cfg.rope_theta, cfg.rope_scaling)
    self.register_buffer("rope_cos", cos, persistent=False)
    self.register_buffer("rope_sin", sin, persistent=False)

  def reset_rope(self):
    """(Re)compute the fp32 RoPE tables on the current device. Required after
    meta-device construction + to_empty (tables are uninitialized memory)."""
    cos, sin = rope_cos_sin(self.rope_dim, self.cfg.max_seq_len, self.cfg.rope_theta,
                            self.cfg.rope_scaling, device=self.rope_cos.device)
    self.rope_cos, self.rope_sin = cos, sin

  def _apply(self, fn, recurse=True):
    # keep RoPE tables fp32 (HIP kernel contract): a model-wide .to(bf16)
    # would quantize them; recompute at full precision on the new device.
    super()._apply(fn, recurse)
    if self.rope_cos.device.type != "meta" and self.rope_cos.dtype != torch.float32:
      self.reset_rope()
    return self

  @property
  def local_layer_ids(self) -> List[int]:
    return list(range(self.shard.start_layer, self.shard.end_layer + 1))

  def _enter(self, caches, positions):
    """-> (caches as LayerKV per local layer | None, positions with a
    dimension, whether to checkpoint each layer). caches=None selects the
    cache-free training forward; activation checkpointing (XOT_ACT_CKPT=1,
    training under grad) trades the per-layer activation residency for a
    recompute in backward."""
    if caches is not None:
      caches = [kv if isinstance(kv, LayerKV) else LayerKV(*kv) for kv in caches]
    if positions.dim() == 0:
      positions = positions.reshape(1)
    use_ckpt = (caches is None and self.training and torch.is_grad_enabled()
                and os.getenv("XOT_ACT_CKPT", "0") == "1")
    return caches, positions, use_ckpt

  def _run_layer(self, layer, use_ckpt: bool, h, positions, kv, start_pos, is_decode, seq_lens):
    args = (h, self.rope_cos, self.rope_sin, positions, kv, start_pos, is_decode, seq_lens)
    if use_ckpt:
      return torch.utils.checkpoint.checkpoint(layer, *args, use_reentrant=False)
    return layer(*args)

  @staticmethod
  def _last_rows(h, last_only: bool):
    """The rows the head sees: the last position alone under last_only."""
    if last_only and h.shape[1] > 1:
      return h[:, -1:, :].contiguous()  # kernels require contiguous rows
    return h

  @staticmethod
  def _pick(logits, is_decode: bool, last_only: bool):
    return logits[:, -1, :] if is_decode or last_only else logits


def ragged_decode_rows(attn, x, cos, sin, positions, kv: LayerKV, is_decode: bool):
  """Eager decode at start_pos < 0 (ring/serve contract: positions carry the
  slots' own rows). When the rows differ, run `attn.forward` one row at a
  time on that row's cache views (correctness first: CPU / no packed cache)
  and return the stacked result; else None, and the caller takes
  positions[0] as start_pos."""
  B, S = x.shape[0], x.shape[1]
  prow = positions.reshape(-1)
  if not (prow.numel() == B * S and S == 1 and B > 1 and int(prow.min()) != int(prow.max())):
    return None
  return torch.cat([attn.forward(x[b:b + 1], cos, sin, prow[b:b + 1], kv.rows(b, b + 1),
                                 int(prow[b]), is_decode, None) for b in range(B)], dim=0)
