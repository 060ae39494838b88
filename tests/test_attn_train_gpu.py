"""Training attention (ops.attn_train: attn_train_fwd / attn_train_bwd, causal
GQA in bf16 at head dims 64 and 128) against fp64 on the CPU over the same bf16
values, under a bound derived from the kernels' arithmetic; determinism; and
the llama training forward on XOT_TRAIN_ATTN=1 against the fp32 sdpa route.

Bound on the gradients (out takes prefill_reference's bound as it stands).
u = 2^-8 is half a bf16 ulp. In fp64: p the softmax, dP = dO . V_t,
delta = sum_t p dP, dS = p (dP - delta). The kernels compute
  p~  = exp(scale s - lse) in fp32 from an fp32 score of hd exact products and
        the forward's fp32 lse = m + log(l): relative error e1, the oracle's
        eps_rel = 2 (2^-24 (hd + 8) sabs + 2^-22) + 2^-24 (2 S + 16) (score, exp
        and the sum l; the fp32 rounding of lse and the log are within the 8
        spare operations of the score term);
  dP~ = an fp32 sum of hd exact products: e_dp = 2^-24 (hd + 8) sum_d |dO||V|;
  delta~ = an fp32 sum over d of dO times the kernel's own bf16 out, which is
        within bound_out of the reference: e_delta = sum_d |dO_d| bound_out_d
        + 2^-24 (hd + 8) sum_d |dO||out|;
  dS~ = p~ (dP~ - delta~) rounded once to bf16:
        |err dS| <= (u + e1) |dS| + p (e_dp + e_delta);
  dQ  = scale * an fp32 sum over at most S positions of dS~ K, rounded to bf16:
        (scale sum_t |err dS||K_t| + 2^-24 (S + 16) scale sum_t |dS||K_t|)(1 + u) + u |dQ|;
  dK  the same with |Q_r|, summed in registers over the rows and the G heads of
        the kv head, G S terms: 2^-24 (G S + 16);
  dV  = an fp32 sum over rows and heads of bf16(p~) dO: with A = sum_{r,g} p |dO_r|,
        ((u + e1) A + 2^-24 (G S + 16) A)(1 + u) + u |dV|.
No constant is fitted to kernel output."""
import functools

import pytest
import torch

import attn_oracle as ao

pytestmark = pytest.mark.gpu

U = 2.0 ** -8
CASES = {  # (B, S, H, KVH, hd)
  "a": (1, 16, 1, 1, 128),    # one tile
  "b": (2, 130, 4, 2, 128),   # several q blocks, a 2-row tail, a kv block with a partial wave; packed qkv slices
  "c": (1, 70, 8, 1, 64),     # hd 64; dK / dV summed over G = 8 heads
  "d": (1, 33, 2, 2, 64),     # one row into a second tile
  "e": (2, 257, 4, 1, 128),   # one row past four q blocks; dkv loops over many q tiles
}


def reference(q, k, v, do, scale, limit_shift=0):
  """fp64 -> ((out, dq, dk, dv), their bounds); q / do [B, S, H, hd], k / v [B, S, KVH, hd] bf16."""
  B, S, H, hd = q.shape
  G = H // k.shape[2]
  qd, kd, vd = (x.double().requires_grad_(True) for x in (q, k, v))
  dod = do.double()
  kk, vv = kd.repeat_interleave(G, dim=2), vd.repeat_interleave(G, dim=2)
  masked = torch.arange(S)[None, :] > torch.arange(S)[:, None] + limit_shift
  p = (scale * torch.einsum("bshd,bthd->bhst", qd, kk)).masked_fill(masked, float("-inf")).softmax(-1)
  out = torch.einsum("bhst,bthd->bshd", p, vv)
  dq, dk, dv = torch.autograd.grad((out * dod).sum(), (qd, kd, vd))
  with torch.no_grad():
    kt, vt = (x.detach().transpose(1, 2) for x in (kd, vd))
    _, b_out = ao.prefill_reference(q, kt, vt, (1 + torch.arange(S)).expand(B, S), scale, 0.0, 0)
    sabs = (scale * torch.einsum("bshd,bthd->bhst", qd.abs(), kk.abs())).masked_fill(masked, 0.0).amax(-1)
    e1 = (2 * (2.0 ** -24 * (hd + 8) * sabs + 2.0 ** -22) + 2.0 ** -24 * (2 * S + 16))[..., None]  # [B, H, S, 1]
    dP = torch.einsum("bshd,bthd->bhst", dod, vv)
    dS = p * (dP - (p * dP).sum(-1, keepdim=True))
    e_dp = 2.0 ** -24 * (hd + 8) * torch.einsum("bshd,bthd->bhst", dod.abs(), vv.abs())
    e_delta = (dod.abs() * (b_out + 2.0 ** -24 * (hd + 8) * out.abs())).sum(-1).transpose(1, 2)[..., None]
    err = (U + e1) * dS.abs() + p * (e_dp + e_delta)
    acc = lambda n: 2.0 ** -24 * (n + 16) * dS.abs()
    over_g = lambda x: x.view(B, S, H // G, G, hd).sum(3)
    b_dq = scale * torch.einsum("bhst,bthd->bshd", err + acc(S), kk.abs()) * (1 + U) + U * dq.abs()
    b_dk = over_g(scale * torch.einsum("bhst,bshd->bthd", err + acc(G * S), qd.abs())) * (1 + U) + U * dk.abs()
    b_dv = over_g(torch.einsum("bhst,bshd->bthd", p * (U + e1 + 2.0 ** -24 * (G * S + 16)), dod.abs())) * (1 + U) + U * dv.abs()
  return (out.detach(), dq, dk, dv), (b_out, b_dq, b_dk, b_dv)


def views(qkv, name):
  """q, k, v of a packed [B, S, (H + 2 KVH) hd] tensor: its column slices in case b (the strides the model hands over)."""
  _, _, H, KVH, hd = CASES[name]
  parts = torch.split(qkv, [H * hd, KVH * hd, KVH * hd], dim=-1)
  return [x.reshape(*qkv.shape[:2], -1, hd) if name == "b" else x.reshape(*qkv.shape[:2], -1, hd).contiguous() for x in parts]


@functools.lru_cache(maxsize=None)
def case(name):
  """Seeded bf16 inputs (q std 0.5, K 2.5, V 0.5, dO 1) -> (qkv, dO, scale, references, bounds), built once and shared."""
  B, S, H, KVH, hd = CASES[name]
  g = torch.Generator().manual_seed(3000 + S)
  std = torch.cat([torch.full((H * hd,), 0.5), torch.full((KVH * hd,), 2.5), torch.full((KVH * hd,), 0.5)])
  qkv = (torch.randn(B, S, (H + 2 * KVH) * hd, generator=g) * std).bfloat16()
  do = torch.randn(B, S, H, hd, generator=g).bfloat16()
  return (qkv, do, hd ** -0.5) + reference(*views(qkv, name), do, hd ** -0.5)


def on_gpu(name):
  qkv, do, scale = case(name)[:3]
  return views(qkv.cuda(), name) + [do.cuda(), scale]


@pytest.mark.parametrize("name", list(CASES))
def test_attn_train_vs_fp64(name):
  from xotorch_amd import ops
  q, k, v, do, scale = on_gpu(name)
  q, k, v = (x.detach().requires_grad_(True) for x in (q, k, v))
  out = ops.attn_train(q, k, v, scale)
  got = (out,) + torch.autograd.grad(out, (q, k, v), do)
  refs, bounds = case(name)[3:]
  worst = {}
  for what, x, ref, bound in zip(("out", "dq", "dk", "dv"), got, refs, bounds):
    assert x.dtype == torch.bfloat16 and x.shape == ref.shape and x.is_contiguous()
    worst[what] = ((x.detach().cpu().double() - ref).abs() / bound).max().item()
  print(f"attn_train case {name} {CASES[name]}: worst err / bound " + " ".join(f"{w} {r:.3f}" for w, r in worst.items()))
  assert all(r <= 1 for r in worst.values()), worst


def test_attn_train_deterministic():
  from xotorch_amd import ops
  q, k, v, do, scale = on_gpu("c")
  runs = []
  for _ in range(2):
    out, lse = ops._gpu().attn_train_fwd(q, k, v, scale)
    runs.append((out,) + tuple(ops._gpu().attn_train_bwd(do, q, k, v, out, lse, scale)))
  assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_llama_training_route(monkeypatch):
  """Tiny 2-layer llama (hd 64, H / KVH = 4 / 2, B = 2, S = 70) in bf16 training
  mode, loss through cross_entropy as DPTrainer.step computes it: logits and
  the qkv_proj / o_proj weight gradients of the XOT_TRAIN_ATTN=1 route and of
  the fp32 sdpa route, each against the same model's fp32 CPU forward and
  backward. Both routes round to bf16 around attention and accumulate in fp32
  in different orders, so the kernel route may err at most twice as far as the
  existing route does (the criterion of the MoE prefill test). Norm weights
  are 1 and the q / k rows of qkv_proj scaled up so that attention matters: the
  fp32 model must answer a doubled softmax scale with a logit change far above
  either error. Under XOT_ACT_CKPT=1 the kernel route must repeat itself bit
  for bit."""
  from xotorch_amd import ops
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import ShardedModel
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  raw = dict(model_type="llama", vocab_size=512, hidden_size=256, intermediate_size=512,
             num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
             head_dim=64, rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=128)
  cfg = config_from_hf(raw, "train-tiny")
  H, KVH, hd = 4, 2, 64
  torch.manual_seed(13)
  m = ShardedModel(cfg, Shard("train-tiny", 0, 1, 2)).to("cuda").to(torch.bfloat16)
  random_init(m)
  with torch.no_grad():
    for name, p in m.named_parameters():
      if "norm" in name:
        p.fill_(1.0)
      elif name.endswith("qkv_proj.weight"):
        p[:(H + KVH) * hd].mul_(4.0)
  m.reset_rope()
  m.train()
  mc = ShardedModel(cfg, Shard("train-tiny", 0, 1, 2)).float()
  mc.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()}, strict=False)
  mc.reset_rope()
  mc.train()
  B, S = 2, 70
  toks, tgts = torch.randint(0, 512, (B, S)), torch.randint(0, 512, (B, S))
  watched = [n for n, _ in m.named_parameters() if n.endswith(("qkv_proj.weight", "o_proj.weight"))]
  assert len(watched) == 4

  def step(model, dev):
    model.zero_grad(set_to_none=True)
    logits = model(toks.to(dev), caches=None, positions=torch.arange(S, device=dev), start_pos=0, last_only=False)
    ce = torch.nn.functional.cross_entropy(logits.float().reshape(-1, 512), tgts.to(dev).reshape(-1), reduction="none")
    ce.mean().backward()
    params = dict(model.named_parameters())
    return [logits.detach().float().cpu()] + [params[n].grad.float().cpu() for n in watched]

  calls = []
  fwd = ops._gpu().attn_train_fwd
  monkeypatch.setattr(ops._hip, "attn_train_fwd", lambda *a: calls.append(1) or fwd(*a))
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
  attn_train = ops.torch_ref.attn_train
  monkeypatch.setattr(ops.torch_ref, "attn_train", lambda q, k, v: attn_train(q, k, v, 2 * hd ** -0.5))
  moved = (step(mc, "cpu")[0] - ref[0]).abs().max().item()
  for what, r, o, n in zip(["logits"] + watched, ref, old, new):
    e_old, e_new = (o - r).abs().max().item(), (n - r).abs().max().item()
    print(f"{what}: max abs err vs fp32 CPU: kernel route {e_new:.4g}, sdpa route {e_old:.4g}")
    assert e_new <= 2 * e_old, (what, e_new, e_old)
    if what == "logits":
      print(f"a doubled softmax scale moves the fp32 logits by {moved:.4g}")
      assert moved > 4 * 2 * max(e_old, e_new), "the model cannot tell a wrong attention from a right one"
