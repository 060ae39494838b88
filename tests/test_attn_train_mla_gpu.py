"""MLA training attention (ops.attn_train_mla: attn_train_mla_fwd / _bwd, causal,
bf16, nope 128 | shared rope 64 keys, 128-dim values) against fp64 on the CPU
over the same bf16 values, under a bound derived from the kernels' arithmetic;
determinism; and the DeepSeek training forward on XOT_TRAIN_ATTN=1 against the
torch route.

Bounds: the derivation of tests/test_attn_train_gpu.py with this kernel's
widths. out takes prefill_reference's bound as it stands, with K expanded to
192 dims and V at 128. u = 2^-8 is half a bf16 ulp. In fp64: p the softmax,
dP = dO . V_t, delta = sum_t p dP, dS = p (dP - delta). The kernels compute
  p~  = exp(scale s - lse) in fp32 from an fp32 score of 192 exact products and
        the forward's fp32 lse: relative error
        e1 = 2 (2^-24 (192 + 8) sabs + 2^-22) + 2^-24 (2 S + 16);
  dP~ = an fp32 sum of 128 exact products: e_dp = 2^-24 (128 + 8) sum_d |dO||V|;
  delta~ = an fp32 sum over 128 dims of dO times the kernel's own bf16 out:
        e_delta = sum_d |dO_d| bound_out_d + 2^-24 (128 + 8) sum_d |dO||out|;
  dS~ = p~ (dP~ - delta~) rounded once to bf16:
        |err dS| <= (u + e1) |dS| + p (e_dp + e_delta);
  dQ  = scale * an fp32 sum over at most S positions of dS~ K (192 dims), to bf16:
        (scale sum_t |err dS||K_t| + 2^-24 (S + 16) scale sum_t |dS||K_t|)(1 + u) + u |dQ|;
  dK of one head (G = 1), before any rounding, an fp32 sum over at most S rows:
        E_h = scale sum_r |err dS||Q_r| + 2^-24 (S + 16) scale sum_r |dS||Q_r|;
  d_kvx[.., :128] = dK_nope rounded to bf16: E_h (1 + u) + u |dK_nope|;
  d_kvx[.., 128:] = dV, an fp32 sum over rows of bf16(p~) dO: with A = sum_r p |dO_r|,
        ((u + e1) A + 2^-24 (S + 16) A)(1 + u) + u |dV|;
  d_k_rot = the H per-head fp32 rope parts of dK added in fp32 and rounded ONCE:
        (sum_h E_h + 2^-24 (H + 16) sum_h |dK_h|)(1 + u) + u |d_k_rot|.
No constant is fitted to kernel output."""
import functools

import pytest
import torch

import attn_oracle as ao

pytestmark = pytest.mark.gpu

U = 2.0 ** -8
NOPE, ROPE, VD = 128, 64, 128
CASES = {  # (B, S, H)
  "a": (1, 16, 1),    # one tile
  "b": (2, 130, 3),   # 2-row tail, odd H, batch stride; kvx a view of the GEMM output, q a non-contiguous slice
  "c": (1, 33, 2),    # one row into a second tile
  "d": (1, 70, 4),    # rope gradient over 4 heads, a kv block with a partial wave
  "e": (2, 257, 2),   # one row past the q blocks; dkv walks many q tiles
}
NAMES = ("out", "dq", "d_k_nope", "d_v", "d_k_rot")


def reference(q, kvx, rot, do, scale, limit_shift=0):
  """fp64 -> ((out, dq, d_k_nope, d_v, d_k_rot), their bounds)."""
  B, S, H, _ = q.shape
  qd, kd, rd = (x.double().requires_grad_(True) for x in (q, kvx, rot))
  dod = do.double()
  k = torch.cat([kd[..., :NOPE], rd[:, :, None, :].expand(B, S, H, ROPE)], dim=-1)  # [B, S, H, 192], per head
  v = kd[..., NOPE:]
  masked = torch.arange(S)[None, :] > torch.arange(S)[:, None] + limit_shift
  p = (scale * torch.einsum("bshd,bthd->bhst", qd, k)).masked_fill(masked, float("-inf")).softmax(-1)
  out = torch.einsum("bhst,bthd->bshd", p, v)
  dq, dkvx, drot, dk = torch.autograd.grad((out * dod).sum(), (qd, kd, rd, k))
  with torch.no_grad():
    _, b_out = ao.prefill_reference(q, k.transpose(1, 2), v.transpose(1, 2), (1 + torch.arange(S)).expand(B, S), scale, 0.0, 0)
    sabs = (scale * torch.einsum("bshd,bthd->bhst", qd.abs(), k.abs())).masked_fill(masked, 0.0).amax(-1)
    e1 = (2 * (2.0 ** -24 * (NOPE + ROPE + 8) * sabs + 2.0 ** -22) + 2.0 ** -24 * (2 * S + 16))[..., None]  # [B, H, S, 1]
    dP = torch.einsum("bshd,bthd->bhst", dod, v)
    dS = p * (dP - (p * dP).sum(-1, keepdim=True))
    e_dp = 2.0 ** -24 * (VD + 8) * torch.einsum("bshd,bthd->bhst", dod.abs(), v.abs())
    e_delta = (dod.abs() * (b_out + 2.0 ** -24 * (VD + 8) * out.abs())).sum(-1).transpose(1, 2)[..., None]
    err = (U + e1) * dS.abs() + p * (e_dp + e_delta) + 2.0 ** -24 * (S + 16) * dS.abs()
    b_dq = scale * torch.einsum("bhst,bthd->bshd", err, k.abs()) * (1 + U) + U * dq.abs()
    e_h = scale * torch.einsum("bhst,bshd->bthd", err, qd.abs())  # [B, S, H, 192]
    b_dk = e_h[..., :NOPE] * (1 + U) + U * dkvx[..., :NOPE].abs()
    b_dv = torch.einsum("bhst,bshd->bthd", p * (U + e1 + 2.0 ** -24 * (S + 16)), dod.abs()) * (1 + U) + U * dkvx[..., NOPE:].abs()
    b_drot = (e_h[..., NOPE:].sum(2) + 2.0 ** -24 * (H + 16) * dk[..., NOPE:].abs().sum(2)) * (1 + U) + U * drot.abs()
  return (out.detach(), dq, dkvx[..., :NOPE], dkvx[..., NOPE:], drot), (b_out, b_dq, b_dk, b_dv, b_drot)


def views(qw, kvw, name):
  """q [B, S, H, 192] out of 200-wide head rows (case b: the slice itself, a head stride of 200) and kvx as the
  per-head view of a [B, S, H * 256] GEMM output."""
  q = qw[..., : NOPE + ROPE]
  return (q if name == "b" else q.contiguous()), kvw.view(*kvw.shape[:2], -1, NOPE + VD)


@functools.lru_cache(maxsize=None)
def case(name):
  """Seeded bf16 inputs (q std 0.5, K 2.5 nope and rope, V 0.5, dO 1) -> (qw, kvw, rot, dO, scale, references,
  bounds), built once and shared."""
  B, S, H = CASES[name]
  g = torch.Generator().manual_seed(4000 + S)
  qw = (torch.randn(B, S, H, NOPE + ROPE + 8, generator=g) * 0.5).bfloat16()
  std = torch.cat([torch.full((NOPE,), 2.5), torch.full((VD,), 0.5)]).repeat(H)
  kvw = (torch.randn(B, S, H * (NOPE + VD), generator=g) * std).bfloat16()
  rot = (torch.randn(B, S, ROPE, generator=g) * 2.5).bfloat16()
  do = torch.randn(B, S, H, VD, generator=g).bfloat16()
  scale = (NOPE + ROPE) ** -0.5
  return (qw, kvw, rot, do, scale) + reference(*views(qw, kvw, name), rot, do, scale)


def on_gpu(name):
  qw, kvw, rot, do, scale = case(name)[:5]
  return list(views(qw.cuda(), kvw.cuda(), name)) + [rot.cuda(), do.cuda(), scale]


def split(out, dq, d_kvx, d_rot):
  return out, dq, d_kvx[..., :NOPE], d_kvx[..., NOPE:], d_rot


@pytest.mark.parametrize("name", list(CASES))
def test_attn_train_mla_vs_fp64(name):
  from xotorch_amd import ops
  q, kvx, rot, do, scale = on_gpu(name)
  assert q.is_contiguous() == (name != "b")
  q, kvx, rot = (x.detach().requires_grad_(True) for x in (q, kvx, rot))
  out = ops.attn_train_mla(q, kvx, rot, scale)
  grads = torch.autograd.grad(out, (q, kvx, rot), do)
  assert all(x.dtype == torch.bfloat16 and x.is_contiguous() for x in (out,) + grads)
  refs, bounds = case(name)[5:]
  worst = {}
  for what, x, ref, bound in zip(NAMES, split(out, *grads), refs, bounds):
    assert x.shape == ref.shape
    worst[what] = ((x.detach().cpu().double() - ref).abs() / bound).max().item()
  print(f"attn_train_mla case {name} {CASES[name]}: worst err / bound " + " ".join(f"{w} {r:.3f}" for w, r in worst.items()))
  assert all(r <= 1 for r in worst.values()), worst


def test_attn_train_mla_deterministic():
  from xotorch_amd import ops
  q, kvx, rot, do, scale = on_gpu("d")
  runs = []
  for _ in range(2):
    out, lse = ops._gpu().attn_train_mla_fwd(q, kvx, rot, scale)
    runs.append((out, lse) + tuple(ops._gpu().attn_train_mla_bwd(do, q, kvx, rot, out, lse, scale)))
  assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_deepseek_training_route(monkeypatch):
  """Tiny 2-layer DeepSeek (128 / 64 / 128, H = 4, both layers dense: no routing
  flips between bf16 and fp32; B = 2, S = 70) in bf16 training mode: logits and
  MLA weight gradients of the XOT_TRAIN_ATTN=1 route and of the torch route,
  each against the same model's fp32 CPU forward and backward; the kernel
  route may err at most twice as far as the torch route (the llama route
  test's criterion). Norms are 1 and q_proj / kv_b_proj scaled up as in
  tests/test_mla_prefill_gpu.py, so the fp32 model answers a doubled softmax
  scale with a logit change above 8 x either error."""
  from xotorch_amd import ops
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
  m.train()
  mc = DeepseekV3Model(cfg, shard).float()
  mc.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()}, strict=False)
  mc.reset_rope()
  mc.train()
  B, S = 2, 70
  toks, tgts = torch.randint(0, 512, (B, S)), torch.randint(0, 512, (B, S))
  watched = [n for n, _ in m.named_parameters()
             if n.endswith(("kv_a_proj_with_mqa.weight", "kv_b_proj.weight", "o_proj.weight"))]
  assert len(watched) == 6

  def step(model, dev):
    model.zero_grad(set_to_none=True)
    logits = model(toks.to(dev), caches=None, positions=torch.arange(S, device=dev), start_pos=0, last_only=False)
    ce = torch.nn.functional.cross_entropy(logits.float().reshape(-1, 512), tgts.to(dev).reshape(-1), reduction="none")
    ce.mean().backward()
    params = dict(model.named_parameters())
    return [logits.detach().float().cpu()] + [params[n].grad.float().cpu() for n in watched]

  calls = []
  fwd = ops._gpu().attn_train_mla_fwd
  monkeypatch.setattr(ops._hip, "attn_train_mla_fwd", lambda *a: calls.append(1) or fwd(*a))
  ref = step(mc, "cpu")
  monkeypatch.delenv("XOT_ACT_CKPT", raising=False)
  monkeypatch.delenv("XOT_TRAIN_ATTN", raising=False)
  old = step(m, "cuda")
  assert not calls
  monkeypatch.setenv("XOT_TRAIN_ATTN", "1")
  new = step(m, "cuda")
  assert len(calls) == 2, "both layers must take the kernel route"
  monkeypatch.setenv("XOT_ACT_CKPT", "1")
  ckpt = step(m, "cuda")
  assert len(calls) == 6, "checkpointing runs each layer's forward again in backward"
  assert all(torch.equal(x, y) for x, y in zip(new, ckpt))
  for mod in mc.modules():
    if isinstance(mod, MLAttention):
      mod.scale *= 2
  moved = (step(mc, "cpu")[0] - ref[0]).abs().max().item()
  for what, r, o, n in zip(["logits"] + watched, ref, old, new):
    e_old, e_new = (o - r).abs().max().item(), (n - r).abs().max().item()
    print(f"{what}: max abs err vs fp32 CPU: kernel route {e_new:.4g}, torch route {e_old:.4g}")
    assert e_new <= 2 * e_old, (what, e_new, e_old)
    if what == "logits":
      print(f"a doubled softmax scale moves the fp32 logits by {moved:.4g}")
      assert moved > 8 * max(e_old, e_new), "the model cannot tell a wrong attention from a right one"
