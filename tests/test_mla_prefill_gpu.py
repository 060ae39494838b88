"""attn_prefill_mla (MLA causal flash prefill, qk 192 = nope 128 | shared rope
64, v 128): the binding against an fp64 reference under the derived bf16-P
bound of tests/attn_oracle.py, and the model route against the torch route."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NOPE, ROPE, VD = 128, 64, 128
SCALE = (NOPE + ROPE) ** -0.5


def _reference(q, kvx, rot, start_pos):
  """fp64 over the bf16 values the kernel reads -> (ref, bound), [B, S, H, 128]."""
  B, S, H, _ = q.shape
  T = start_pos + S
  qd, kd = q.double(), kvx.double()
  k = torch.cat([kd[..., :NOPE], rot.double()[:, :T, None, :].expand(B, T, H, ROPE)], dim=-1)
  masked = torch.arange(T)[None, :] > start_pos + torch.arange(S)[:, None]
  s = (SCALE * torch.einsum("bshd,bthd->bhst", qd, k)).masked_fill(masked, float("-inf"))
  sabs = (SCALE * torch.einsum("bshd,bthd->bhst", qd.abs(), k.abs())).masked_fill(masked, 0.0).amax(-1)
  w = s.softmax(-1)
  v = kd[..., NOPE:]
  ref = torch.einsum("bhst,bthd->bshd", w, v)
  absw = torch.einsum("bhst,bthd->bshd", w, v.abs())
  eps_rel = 2 * (2.0 ** -24 * (NOPE + ROPE + 8) * sabs + 2.0 ** -22) + 2.0 ** -24 * (2 * T + 16)
  eps_rel = eps_rel.permute(0, 2, 1)[..., None]  # [B, S, H, 1]
  bound = (2.0 ** -8 * absw + eps_rel * absw) * (1 + 2.0 ** -8) + 2.0 ** -8 * ref.abs()
  return ref, bound


@pytest.mark.parametrize("B,H,S,start_pos", [
  (1, 1, 16, 0),      # one sub-tile, one K tile
  (2, 3, 80, 0),      # ragged q block, odd H, batch stride
  (1, 2, 130, 0),     # a second q block holding 2 rows
  (2, 2, 48, 40),     # chunk offset that is no multiple of 32
  (1, 2, 33, 95),     # T = 128 exactly: the last row sees a full last tile
  (1, 16, 256, 256),  # v2-lite's H, a prefix as long as the chunk
])
def test_attn_prefill_mla_vs_fp64(B, H, S, start_pos):
  from xotorch_amd import ops
  T = start_pos + S
  g = torch.Generator().manual_seed(1000 * S + start_pos + H)
  q = torch.randn(B, S, H, NOPE + ROPE, generator=g).bfloat16()
  kvx = torch.randn(B, T, H, NOPE + VD, generator=g)
  kvx[..., NOPE:] *= 0.5
  kvx = kvx.bfloat16()  # exactly T rows: an unpredicated tail read leaves the tensor
  # the rope key carries half a score's variance (64 * 2 = 128 * 1); rows from T on are poison
  rot_c = torch.full((B, 1, T + 24, ROPE), 1e4).bfloat16()
  rot_c[:, 0, :T] = (torch.randn(B, T, ROPE, generator=g) * 2 ** 0.5).bfloat16()
  ref, bound = _reference(q, kvx, rot_c[:, 0], start_pos)
  no_rope, _ = _reference(q, kvx, torch.zeros_like(rot_c[:, 0]), start_pos)
  assert ((no_rope - ref).abs() / bound).max() > 4, "inputs cannot tell a kernel that drops the rope chunks"
  out = ops.attn_prefill_mla(q.cuda(), kvx.cuda(), rot_c.cuda(), start_pos, SCALE)
  assert out.shape == (B, S, H, VD) and out.dtype == torch.bfloat16
  ratio = ((out.cpu().double() - ref).abs() / bound).max().item()
  print(f"attn_prefill_mla B={B} H={H} S={S} start_pos={start_pos}: worst err / bound {ratio:.3f}")
  assert ratio <= 1, ratio


def test_deepseek_prefill_kernel_route_vs_torch_route(monkeypatch):
  """Tiny DeepSeek model, prefill of 70 tokens then a 40-token chunk at
  start_pos 70: logits of the kernel route and of the XOT_MLA_PREFILL=0
  route, each against the fp32 CPU forward. Both round P to bf16 and
  accumulate in fp32 in different orders, so the kernel route may err at
  most twice as far as the torch route does. random_init leaves this
  family's norm weights (named without a `.weight` suffix) near 0, which
  makes every softmax a uniform average that no attention mistake can move;
  so the norms are set to 1 and q_proj / kv_b_proj scaled up until scores
  spread by O(1), and the fp32 model must answer a doubled softmax scale
  with a logit change far above the tolerance."""
  from xotorch_amd import ops
  from xotorch_amd.engine.kvcache import ShardKVCache
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.deepseek_v3 import DeepseekV3Model, MLAttention
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  raw = dict(model_type="deepseek_v3", vocab_size=512, hidden_size=256, intermediate_size=512,
             num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
             kv_lora_rank=512, qk_rope_head_dim=ROPE, qk_nope_head_dim=NOPE, v_head_dim=VD,
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
  B, chunks = 2, ((0, 70), (70, 40))
  toks = torch.randint(0, 512, (B, 110))
  heads, kd, vd = cfg.kv_cache_dims()

  def logits(model, dev, dtype):
    cache = ShardKVCache(2, B, heads, 128, kd, dtype, dev, v_dim=vd)
    with torch.inference_mode():
      return torch.cat([model(toks[:, s0:s0 + n].to(dev), caches=cache.caches, start_pos=s0,
                              positions=torch.arange(s0, s0 + n, dtype=torch.int32, device=dev)).float().cpu()
                        for s0, n in chunks], dim=1)

  calls = []
  kernel = ops.attn_prefill_mla
  monkeypatch.setattr(ops, "attn_prefill_mla", lambda *a: calls.append(1) or kernel(*a))
  ref = logits(mc, "cpu", torch.float32)
  monkeypatch.setenv("XOT_MLA_PREFILL", "1")
  err_kernel = (logits(m, "cuda", torch.bfloat16) - ref).abs().max().item()
  assert len(calls) == 4, "2 layers x 2 chunks must take the kernel route"
  monkeypatch.setenv("XOT_MLA_PREFILL", "0")
  err_torch = (logits(m, "cuda", torch.bfloat16) - ref).abs().max().item()
  assert len(calls) == 4
  attns = [mod for mod in mc.modules() if isinstance(mod, MLAttention)]
  for a in attns:
    a.scale *= 2
  moved = (logits(mc, "cpu", torch.float32) - ref).abs().max().item()
  print(f"logits max abs err vs fp32 CPU: kernel route {err_kernel:.4g}, torch route {err_torch:.4g}; "
        f"a doubled softmax scale moves the fp32 logits by {moved:.4g}")
  assert moved > 4 * 2 * err_torch, "the model cannot tell a wrong attention from a right one"
  assert err_kernel <= 2 * err_torch, (err_kernel, err_torch)
