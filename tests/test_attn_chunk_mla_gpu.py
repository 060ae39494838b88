"""Absorbed MLA chunk attention (attn_chunk_mla: q [B, S, H, 576] at an offset
over the packed latent cache, four row tiles per workgroup on one LDS-staged
tile stream, split over the live length) against an fp64 reference, its
refusals, and the XOT_MLA_CHUNK route of a DeepSeek model.

Bound: tests/test_attn_chunk_gpu.py's, restated for MLA: one shared K of 576
dims whose first 512 are V, no softcap, hd + 8 = 584, and the split-KV merge
term 2^-24 (2 T + 16 + nsplit + 2). No constant is fitted to kernel output.

Worst err / bound measured on the MI355X, in case order:
0.00, 0.60, 0.57, 0.58, 0.37, 0.36. Model route, logits max abs err against the
fp32 CPU forward: absorbed chunk route 0.0067, kv_b expansion route 0.0069."""
import pytest
import torch

from attn_oracle import mla_pack

pytestmark = pytest.mark.gpu

LAT, DQK = 512, 576
SCALE = DQK ** -0.5


def _reference(q, k, q_start, nsplit, shift=0):
  """fp64 over q's bf16 values [B, S, H, 576] and the latent | rope rows k [B, T, 576] the kernel reads; row s
  of sequence b sees [0, q_start[b] + s + 1 + shift) -> (ref, bound), [B, S, H, 512]."""
  S, T = q.shape[1], k.shape[1]
  qd, v = q.double(), k[..., :LAT]
  end = (torch.tensor(q_start)[:, None] + torch.arange(S)[None, :] + 1 + shift)[:, None, :, None]  # [B, 1, S, 1]
  masked = torch.arange(T) >= end
  s = SCALE * torch.einsum("bshd,btd->bhst", qd, k)
  sabs = (SCALE * torch.einsum("bshd,btd->bhst", qd.abs(), k.abs())).masked_fill(masked, 0.0).amax(-1)
  w = s.masked_fill(masked, float("-inf")).softmax(-1).nan_to_num(0.0)  # a row that sees nothing gives 0
  ref = torch.einsum("bhst,btd->bshd", w, v)
  absw = torch.einsum("bhst,btd->bshd", w, v.abs())
  eps_rel = 2 * (2.0 ** -24 * (DQK + 8) * sabs + 2.0 ** -22) + 2.0 ** -24 * (2 * T + 16 + nsplit + 2)
  eps_rel = eps_rel.permute(0, 2, 1)[..., None]  # [B, S, H, 1]
  bound = (2.0 ** -8 * absw + eps_rel * absw) * (1 + 2.0 ** -8) + 2.0 ** -8 * ref.abs()
  return ref, bound


@pytest.mark.parametrize("B,H,S,q_start,cap,nsplit,forced", [
  (1, 16, 1, 0, 32, 1, None),         # one tile, one position, direct store
  (1, 16, 5, 0, 32, 1, None),         # rows seeing 1..5 positions; five row tiles: a second workgroup, one live wave
  (2, 20, 3, 29, 256, 8, None),       # tiles that straddle s, partial last tile, limits across a tile edge, empty splits
  (2, 16, 7, (5, 90), 128, 4, None),  # per-sequence offsets
  (1, 128, 5, 100, 256, 8, None),     # 40 row tiles, ten workgroups per split
  (1, 16, 5, 200, 256, 2, "2"),       # XOT_MLA_CHUNK_NSPLIT=2: several tiles per wave, so (m, l), the rescale and
])                                    # the double buffer carry state
def test_attn_chunk_mla_vs_fp64(monkeypatch, B, H, S, q_start, cap, nsplit, forced):
  from xotorch_amd import ops
  assert ops.hip_available()
  if forced:
    monkeypatch.setenv("XOT_MLA_CHUNK_NSPLIT", forced)
  starts = list(q_start) if isinstance(q_start, tuple) else [q_start] * B
  T = max(starts) + S  # from T to the capacity: poison
  g = torch.Generator().manual_seed(1000 * S + starts[-1] + H)
  q = (0.5 * torch.randn(B, S, H, DQK, generator=g)).bfloat16()
  kb = (2.5 * torch.randn(B, cap, DQK, generator=g)).bfloat16()
  kb[:, T:] = torch.where(torch.rand(B, cap - T, DQK, generator=g) < 0.5, -1e30, 1e30).bfloat16()
  k = kb[:, :T].double()
  ref, bound = _reference(q, k, starts, nsplit)
  if T > 1:
    moved, _ = _reference(q, k, starts, nsplit, shift=-1)
    assert ((moved - ref).abs() / bound).max() > 4, "inputs cannot tell a limit read one position early"
  assert ops._hip.attn_chunk_mla_nsplit(B, H, S, cap) == nsplit
  kp, vp = (t.cuda() for t in mla_pack(kb[..., :LAT], kb[..., LAT:], cap))
  qs = torch.tensor(starts, dtype=torch.int32, device="cuda") if isinstance(q_start, tuple) else q_start
  out = ops.attn_chunk_mla(q.cuda(), kp, vp, qs, SCALE)
  assert out.shape == (B, S, H, LAT) and out.dtype == torch.bfloat16
  ratio = ((out.cpu().double() - ref).abs() / bound).max().item()
  print(f"attn_chunk_mla B={B} H={H} S={S} q_start={q_start} cap={cap} nsplit={nsplit}: worst err / bound {ratio:.3f}")
  assert ratio <= 1, ratio


@pytest.mark.parametrize("S,H,dqk,dtype,q_start", [
  (1, 16, 512, torch.bfloat16, 0),   # last dim 512
  (1, 16, DQK, torch.uint8, 0),      # an e4m3 (uint8) cache
  (65, 16, DQK, torch.bfloat16, 0),  # R = 1040
  (5, 16, DQK, torch.bfloat16, 60),  # int q_start + S = 65 above the capacity 64
], ids=["dim512", "uint8-cache", "rows1040", "capacity"])
def test_attn_chunk_mla_refuses(S, H, dqk, dtype, q_start):
  from xotorch_amd import ops
  kp = torch.zeros(1, 4, 18, 64, 8, dtype=dtype, device="cuda")
  vp = torch.zeros(1, 32, 2, 64, 8, dtype=dtype, device="cuda")
  q = torch.zeros(1, S, H, dqk, dtype=torch.bfloat16, device="cuda")
  with pytest.raises(RuntimeError):
    ops.attn_chunk_mla(q, kp, vp, q_start)


def test_deepseek_chunk_route(monkeypatch):
  """Tiny 2-layer DeepSeek (the config and weight scaling of tests/test_mla_prefill_gpu.py, where attention
  visibly matters), B = 2: 60 tokens prefilled with the knob off, then a 5-token chunk at 60 with XOT_MLA_CHUNK=1
  (both layers on attn_chunk_mla) and 0 (none), each against the fp32 CPU forward of the same chunk. The absorbed
  route rounds q_lat and out_lat to bf16, which the other does not: it may err at most twice as far."""
  from xotorch_amd import ops
  from xotorch_amd.engine.kvcache import ShardKVCache
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.deepseek_v3 import DeepseekV3Model
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  raw = dict(model_type="deepseek_v3", vocab_size=512, hidden_size=256, intermediate_size=512,
             num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
             kv_lora_rank=512, qk_rope_head_dim=64, qk_nope_head_dim=128, v_head_dim=128,
             q_lora_rank=0, first_k_dense_replace=2, n_routed_experts=0,
             rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=128)
  cfg = config_from_hf(raw, "ds-tiny")
  shard = Shard("ds-tiny", 0, 1, 2)
  torch.manual_seed(11)
  m = DeepseekV3Model(cfg, shard).to("cuda").to(torch.bfloat16)
  random_init(m)
  with torch.no_grad():
    for name, p in m.named_parameters():
      if name.endswith("norm"):
        p.fill_(1.0)
      elif name.endswith("q_proj.weight"):
        p.mul_(4.0)
      elif name.endswith("kv_b_proj.weight"):
        p.mul_(2.0)
  m.reset_rope()
  m.eval()
  mc = DeepseekV3Model(cfg, shard).float()
  mc.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()}, strict=False)
  mc.reset_rope()
  mc.eval()
  B = 2
  toks = torch.randint(0, 512, (B, 65))
  heads, kd, vd = cfg.kv_cache_dims()
  calls = []
  kernel = ops._hip.attn_chunk_mla
  monkeypatch.setattr(ops._hip, "attn_chunk_mla", lambda *a: calls.append(1) or kernel(*a))

  def chunk_logits(model, dev, dtype, knob):
    cache = ShardKVCache(2, B, heads, 128, kd, dtype, dev, v_dim=vd)
    step = lambda s0, n: model(toks[:, s0:s0 + n].to(dev), caches=cache.caches, start_pos=s0,
                               positions=torch.arange(s0, s0 + n, dtype=torch.int32, device=dev)).float().cpu()
    with torch.inference_mode():
      monkeypatch.setenv("XOT_MLA_CHUNK", "0")
      step(0, 60)
      monkeypatch.setenv("XOT_MLA_CHUNK", knob)
      return step(60, 5)

  ref = chunk_logits(mc, "cpu", torch.float32, "0")
  on = chunk_logits(m, "cuda", torch.bfloat16, "1")
  assert calls == [1, 1], "both layers must take the chunk kernel, once each"
  off = chunk_logits(m, "cuda", torch.bfloat16, "0")
  assert calls == [1, 1]
  err_on, err_off = (on - ref).abs().max().item(), (off - ref).abs().max().item()
  print(f"logits max abs err vs fp32 CPU: absorbed chunk route {err_on:.4g}, kv_b expansion route {err_off:.4g}")
  assert (on.argmax(-1) == off.argmax(-1)).all()
  assert err_on <= 2 * err_off, (err_on, err_off)
