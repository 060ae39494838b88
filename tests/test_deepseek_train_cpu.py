"""DeepSeek cache-free training forward (MLAttention._forward_nocache) on the
CPU in fp32: parity with the cached prefill forward, gradients into the MLA
projections, and torch_ref.attn_train_mla against an independent fp64
expression."""
import pytest
import torch

from test_build_cpu import DS_TINY

FAMILIES = {"v3": DS_TINY, "v2": {**DS_TINY, "model_type": "deepseek_v2", "q_lora_rank": 0}}


def tiny(family):
  """4 layers: one dense, three MoE."""
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.deepseek_v3 import DeepseekV3Model
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  cfg = config_from_hf(FAMILIES[family], "ds-tiny")
  torch.manual_seed(5)
  m = DeepseekV3Model(cfg, Shard("ds-tiny", 0, 3, 4)).float()
  random_init(m)
  return cfg, m


@pytest.mark.parametrize("family", list(FAMILIES))
def test_deepseek_train_forward_matches_inference(family):
  from xotorch_amd.engine.kvcache import ShardKVCache
  cfg, m = tiny(family)
  B, S = 2, 12
  toks = torch.randint(0, 101, (B, S))
  pos = torch.arange(S, dtype=torch.int32)
  heads, kd, vd = cfg.kv_cache_dims()
  cache = ShardKVCache(4, B, heads, S + 2, kd, torch.float32, "cpu", v_dim=vd)
  m.eval()
  with torch.no_grad():
    ref = m(toks, caches=cache.caches, positions=pos, start_pos=0, last_only=False)
  out = m(toks, caches=None, positions=pos, start_pos=0, last_only=False)
  assert out.shape == ref.shape == (B, S, 101)
  assert torch.allclose(out, ref, atol=1e-4, rtol=1e-4), (out - ref).abs().max()


@pytest.mark.parametrize("family", list(FAMILIES))
def test_deepseek_train_gradients_reach_mla(family):
  _, m = tiny(family)
  m.train()
  B, S = 2, 12
  toks, tgts = torch.randint(0, 101, (B, S)), torch.randint(0, 101, (B, S))
  logits = m(toks, caches=None, positions=torch.arange(S, dtype=torch.int32), start_pos=0, last_only=False)
  torch.nn.functional.cross_entropy(logits.reshape(-1, 101), tgts.reshape(-1)).backward()
  q_projs = ("q_a_proj.weight", "q_b_proj.weight") if family == "v3" else ("q_proj.weight",)
  wanted = ("kv_a_proj_with_mqa.weight", "kv_b_proj.weight", "o_proj.weight") + q_projs
  grads = {n: p.grad for n, p in m.named_parameters() if n.endswith(wanted)}
  assert len(grads) == 4 * len(wanted)
  for n, g in grads.items():
    assert g is not None and torch.isfinite(g).all() and g.abs().max() > 0, n


def test_attn_train_mla_definition_fp64():
  """Value and gradients of torch_ref.attn_train_mla at dims 16 / 8 / 12 against
  per-head, per-row softmax sums written out here; the k_rot gradient is the
  sum over heads of the per-head rope-key gradients."""
  from xotorch_amd.ops import torch_ref
  B, S, H, nope, rope, vd = 2, 19, 3, 16, 8, 12
  g = torch.Generator().manual_seed(7)
  q, kvx, k_rot, do = (torch.randn(*s, generator=g, dtype=torch.float64) for s in
                       ((B, S, H, nope + rope), (B, S, H, nope + vd), (B, S, rope), (B, S, H, vd)))
  scale = 0.23
  a, b, c = (x.clone().requires_grad_(True) for x in (q, kvx, k_rot))
  out = torch_ref.attn_train_mla(a, b, c, scale)
  assert out.dtype == torch.float64
  got = (out,) + torch.autograd.grad(out, (a, b, c), do)

  a, b = (x.clone().requires_grad_(True) for x in (q, kvx))
  per_head = [k_rot.clone().requires_grad_(True) for _ in range(H)]  # one copy of the shared key per head
  rows = []
  for bi in range(B):
    for s in range(S):
      for h in range(H):
        k = torch.cat([b[bi, :s + 1, h, :nope], per_head[h][bi, :s + 1]], dim=-1)  # [s + 1, nope + rope]
        w = torch.exp(scale * (k @ a[bi, s, h]))
        rows.append((w / w.sum()) @ b[bi, :s + 1, h, nope:])
  ref = torch.stack(rows).view(B, S, H, vd)
  dq, dkvx, *drot = torch.autograd.grad(ref, [a, b] + per_head, do)
  for what, x, r in zip(("out", "dq", "d_kvx", "d_k_rot"), got, (ref, dq, dkvx, sum(drot))):
    assert torch.allclose(x, r, atol=1e-12, rtol=1e-10), (what, (x - r).abs().max())
