"""Device-resident KV caches, laid out for the CDNA4 decode-attention kernels.

Standard layout [B, KVH, T, hd]: each (b, kv_head) has T contiguous rows of
hd elements (256 B at hd=128 bf16) — prefill attention (sdpa) and the VALU
decode kernel stream rows with coalesced 16 B/lane loads.

MFMA layout (GPU, hd in ops.PACKED_HEAD_DIMS = 128 or 256): a second copy of K
and V pre-shuffled into v_mfma_f32_16x16x32_bf16 B-fragment order so the MFMA
attention kernels stream the cache with fully-coalesced 1 KB wave loads:
  K_packed [B, KVH, T32/16, hd/32, 64, 8]   (16-position x 32-hd-chunk tiles)
  V_packed [B, KVH, hd/16, T32/32, 64, 8]   (32-position x 16-hd-column tiles)
(T32 = capacity rounded up to 32; both copies are appended by the fused
rope_qkv_append kernel. In fp8-KV mode they are e4m3 bytes with per-row
scales [B, KVH, T32], whatever the head dim.)  The reference's equivalent is torchtune's per-layer
cache setup (/root/reference/xotorch/inference/torch/sharded_inference_engine.py:71-82).
"""
from __future__ import annotations

import os
from typing import List, NamedTuple, Optional

import torch

from xotorch_amd import ops


class LayerKV(NamedTuple):
  k: Optional[torch.Tensor]  # None (with v) in a packed-only cache (ShardKVCache(plain=False))
  v: Optional[torch.Tensor]
  kp: Optional[torch.Tensor] = None  # MFMA-packed K (cuda, hd 128 or 256; bf16 or e4m3 bytes)
  vp: Optional[torch.Tensor] = None  # MFMA-packed V (same head dims and dtype as kp)
  ksc: Optional[torch.Tensor] = None  # fp8 mode: per-row K scales [B, KVH, T32]
  vsc: Optional[torch.Tensor] = None  # fp8 mode: per-row V scales

  def rows(self, b0: int, b1: int) -> "LayerKV":
    """Views of batch rows [b0, b1) over every field that is present."""
    return LayerKV(*(t[b0:b1] if t is not None else None for t in self))


class ShardKVCache:
  """One LayerKV per local layer of a shard."""

  def __init__(self, n_layers: int, batch: int, n_kv_heads: int, capacity: int, head_dim: int,
               dtype: torch.dtype = torch.bfloat16, device: str = "cpu",
               v_dim: Optional[int] = None, plain: bool = True):
    """v_dim: per-position width of the v tensor when it differs from
    head_dim (MLA latent caches: k stores the kv_lora latent, v the shared
    roped key — see ModelConfig.kv_cache_dims()).
    plain=False: a packed-only cache, LayerKV.k / .v are None. For callers
    whose append and attention read only (kp, vp): the llama decoder with MFMA
    attention. Honoured only where the bf16 GQA packed copies are allocated
    and XOT_FP8_KV is off (fp8-KV prefill reads the plain cache); anywhere
    else the argument is ignored and the plain tensors are allocated."""
    self.capacity = capacity
    self.batch = batch
    self.caches: List[LayerKV] = []
    vd = v_dim if v_dim is not None else head_dim
    t32 = (capacity + 31) // 32 * 32
    # fragment-packed second copies for the MFMA attention kernels: shapes of
    # (kp, vp) and of the fp8 mode's per-row scale tensors, or none (plain)
    packed = (str(device).startswith("cuda") and dtype == torch.bfloat16
              and ops.mfma_attn_enabled())
    if packed and vd == head_dim and ops.gqa_packed_kv(head_dim, dtype):
      # GQA (head_dim in ops.PACKED_HEAD_DIMS): 16-position x 32-hd-chunk K
      # tiles, 32-position x 16-hd-column V tiles
      kp_shape = (batch, n_kv_heads, t32 // 16, head_dim // 32, 64, 8)
      vp_shape = (batch, n_kv_heads, head_dim // 16, t32 // 32, 64, 8)
      scale_shapes = [(batch, n_kv_heads, t32)] * 2
    elif packed and n_kv_heads == 1 and head_dim == 512 and vd == 64:
      # MLA latent cache (k = 512-dim latent, v = 64-dim roped shared key,
      # one kv "head") for the absorbed-MQA decode kernel (18 qk chunks /
      # 32 pv groups — hip_ops.hip MLA section); one scale tensor
      kp_shape = (batch, t32 // 16, 18, 64, 8)
      vp_shape = (batch, 32, t32 // 32, 64, 8)
      scale_shapes = [(batch, t32)]
    else:
      kp_shape = vp_shape = None
      scale_shapes = []
    # fp8-KV: e4m3 packed copies (half the decode stream) + per-row scales;
    # the plain cache stays in `dtype` for prefill
    fp8_kv = kp_shape is not None and os.getenv("XOT_FP8_KV", "0") == "1"
    gqa_packed = kp_shape is not None and len(kp_shape) == 6
    self.plain = plain or not (gqa_packed and dtype == torch.bfloat16 and not fp8_kv)
    for _ in range(n_layers):
      layer = [None, None]
      if self.plain:
        layer = [torch.zeros(batch, n_kv_heads, capacity, head_dim, dtype=dtype, device=device),
                 torch.zeros(batch, n_kv_heads, capacity, vd, dtype=dtype, device=device)]
      if kp_shape is not None:
        pdt = torch.uint8 if fp8_kv else dtype
        layer += [torch.zeros(kp_shape, dtype=pdt, device=device),
                  torch.zeros(vp_shape, dtype=pdt, device=device)]
      if fp8_kv:
        layer += [torch.ones(s, dtype=torch.float32, device=device) for s in scale_shapes]
      self.caches.append(LayerKV(*layer))

  @classmethod
  def for_config(cls, cfg, n_layers: int, batch: int, capacity: int,
                 dtype: torch.dtype = torch.bfloat16, device: str = "cpu",
                 plain: bool = True) -> "ShardKVCache":
    """The cache `cfg`'s decoder expects (ModelConfig.kv_cache_dims())."""
    heads, k_dim, v_dim = cfg.kv_cache_dims()
    return cls(n_layers, batch, heads, capacity, k_dim, dtype, device, v_dim=v_dim, plain=plain)

  def rows(self, b0: int, b1: int) -> List[LayerKV]:
    """Every layer's LayerKV.rows(b0, b1): a batch slice of the whole cache."""
    return [c.rows(b0, b1) for c in self.caches]

  def __getitem__(self, i):
    return self.caches[i]

  def __len__(self):
    return len(self.caches)

  def reset(self):
    for c in self.caches:
      for t in (c.k, c.v, c.kp, c.vp):
        if t is not None:
          t.zero_()

  def nbytes(self) -> int:
    total = 0
    for c in self.caches:
      total += sum(t.numel() * t.element_size() for t in (c.k, c.v, c.kp, c.vp) if t is not None)
    return total
