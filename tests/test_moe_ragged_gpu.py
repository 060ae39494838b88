"""MoE prefill on the ragged grouped GEMM (moe_plan + moe_gemm_ragged, BM = 128):
exact integer products of both instantiations over a fixed routing that has an
expert of two full tiles and a tail, one of exactly one tile, a one-row expert,
an empty one and dead table entries; the block (models.moe.moe_prefill) and the
XOT_MOE_PREFILL=1 route of both model families against an fp64 reference.

No fitted tolerance: the new route's max abs error may be at most twice that of
the parent's route (sorted_expert_prefill) on the same inputs. Both round gu, h
and y to bf16 once each and sum k terms in fp32; they differ in fp32 summation
order only."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T, TOPK, E = 300, 2, 5
COUNTS = [300, 128, 1, 171, 0]
SHAPES = [(192, 128), (256, 192)]  # (D, I): K-steps 3 / 2 and 4 / 3; down N = 192 half-fills its second n tile


def _ids():
  second = torch.cat([torch.full((128,), 1), torch.full((1,), 2), torch.full((171,), 3)])
  return torch.stack([torch.zeros(T, dtype=torch.long), second], dim=1).to(torch.int32).cuda()


def _pack(w):
  from xotorch_amd import ops
  return torch.stack([ops.pack_decode_weight(we) for we in w]).contiguous()


def _block_ref(flat, ids, w, wgu, wd):
  """fp64 routed block over the bf16 values: sum_j w[t, j] * down_e(silu(gate_e x_t) * up_e x_t), e = ids[t, j]."""
  out = torch.zeros(flat.shape, dtype=torch.float64, device=flat.device)
  I = wd.shape[2]
  for e in range(wgu.shape[0]):
    tok, j = torch.where(ids == e)
    gu = flat[tok].double() @ wgu[e].double().T
    y = (torch.nn.functional.silu(gu[:, :I]) * gu[:, I:]) @ wd[e].double().T
    out.index_add_(0, tok, y * w[tok, j, None].double())
  return out


@pytest.mark.parametrize("gate_up", [True, False])
@pytest.mark.parametrize("D,I", SHAPES)
def test_ragged_gemm_exact(D, I, gate_up):
  from xotorch_amd import ops
  g = torch.Generator().manual_seed(D + I + gate_up)
  tern = lambda *s: torch.randint(-1, 2, s, generator=g).bfloat16().cuda()
  ids = _ids()
  sorted_tok, inv_pos, tile_expert, tile_row0, offsets = ops.moe_plan(ids, E, ops.moe_ragged_bm())
  assert ops.moe_ragged_bm() == 128
  assert offsets.tolist() == [0, 300, 428, 429, 600, 600]
  assert tile_expert.tolist() == [0, 0, 0, 1, 2, 3, 3, -1, -1, -1]
  assert tile_row0.tolist()[:7] == [0, 128, 256, 300, 428, 429, 557]
  slot_expert = torch.repeat_interleave(torch.arange(E), torch.tensor(COUNTS)).cuda()
  assert sorted(inv_pos.flatten().tolist()) == list(range(T * TOPK))
  assert torch.equal(sorted_tok[inv_pos.long()], torch.arange(T, device="cuda", dtype=torch.int32)[:, None].expand(T, TOPK))
  assert torch.equal(slot_expert[inv_pos.long()], ids.long())
  K, N = (D, 2 * I) if gate_up else (I, D)
  x, w = tern(T, K), tern(E, N, K)
  rows = x[sorted_tok.long()]  # the reference's gathered copy; the down launch reads it, gate_up gathers itself
  ref = torch.cat([rows[a:b].double() @ w[e].double().T for e, (a, b) in enumerate(zip(offsets[:-1], offsets[1:]))])
  assert ref.abs().max() <= 256  # exact in bf16
  got = ops.moe_gemm_ragged(x if gate_up else rows, _pack(w), N, sorted_tok, tile_expert, tile_row0, offsets,
                            gate_up, gate_up)
  want = ops.swiglu_packed(ref.bfloat16()) if gate_up else ref.bfloat16()
  assert got.shape == want.shape and torch.equal(got, want), (got.float() - want.float()).abs().max()


def _errs(new, old, ref):
  e_new, e_old = ((o.bfloat16().double() - ref).abs().max().item() for o in (new, old))
  print(f"max abs err vs fp64: ragged route {e_new:.5f}, sorted per-expert route {e_old:.5f}")
  assert e_new <= 2 * e_old, (e_new, e_old)


@pytest.mark.parametrize("D,I", SHAPES)
def test_moe_prefill_block(D, I):
  """Measured on the MI355X, (192, 128) then (256, 192): see docs/KERNELS.md, Ragged grouped expert GEMM."""
  from xotorch_amd import ops
  from xotorch_amd.models import moe
  g = torch.Generator().manual_seed(7 * D + I)
  rnd = lambda *s, std=1.0: (std * torch.randn(*s, generator=g)).bfloat16().cuda()
  flat, wgu, wd = rnd(T, D), rnd(E, 2 * I, D, std=D ** -0.5), rnd(E, D, I, std=I ** -0.5)
  ids, w = _ids(), torch.randn(T, TOPK, generator=g).softmax(-1).cuda()
  lin = torch.nn.functional.linear
  experts = [lambda xe, e=e: lin(ops.swiglu_packed(lin(xe, wgu[e])), wd[e]) for e in range(E)]
  with torch.inference_mode():
    new = moe.moe_prefill(flat, ids, w, E, I, _pack(wgu), _pack(wd))
    old = moe.sorted_expert_prefill(flat, w, ids.long(), experts)
  assert new.dtype == torch.bfloat16 and new.shape == (T, D)
  _errs(new, old, _block_ref(flat, ids, w, wgu, wd))


def _tiny_mixtral():
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import MoEMLP
  from xotorch_amd.models.registry import builtin_config
  raw = dict(builtin_config("mixtral-8x7b"))
  raw.update(hidden_size=256, intermediate_size=512)
  torch.manual_seed(2)
  m = MoEMLP(config_from_hf(raw, "mixtral-gpu-tiny")).to("cuda").to(torch.bfloat16).eval()
  for e in m.experts:
    e.gate_up_proj.pack_decode()
    e.down_proj.pack_decode()
  wgu, wd = (torch.stack([getattr(e, p).weight.detach() for e in m.experts]) for p in ("gate_up_proj", "down_proj"))
  old_route = lambda f: m._route(f)[::-1]
  new_route = lambda f, ops: ops.moe_route(m.gate(f).float().contiguous(), None, m.top_k, 0)
  return m, wgu, wd, old_route, new_route, lambda f: 0.0


def _tiny_dsmoe():
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.deepseek_v3 import DsMoE
  raw = dict(model_type="deepseek_v2", vocab_size=64, hidden_size=256, intermediate_size=512,
             moe_intermediate_size=256, n_routed_experts=8, num_experts_per_tok=2, n_shared_experts=1, n_group=1,
             topk_group=1, routed_scaling_factor=1.0, norm_topk_prob=False, first_k_dense_replace=0,
             num_attention_heads=4, num_key_value_heads=4, kv_lora_rank=512, qk_rope_head_dim=64,
             qk_nope_head_dim=64, v_head_dim=64, rms_norm_eps=1e-6, max_position_embeddings=64)
  torch.manual_seed(11)
  m = DsMoE(config_from_hf(raw, "dsmoe-tiny")).to("cuda").to(torch.bfloat16).eval()
  with torch.no_grad():
    m.gate_weight.normal_(0, 0.5)
    for p in list(m.experts.parameters()) + list(m.shared_experts.parameters()):
      p.normal_(0, 0.05)
  wgu = torch.stack([torch.cat([e.gate_proj.weight, e.up_proj.weight]).detach() for e in m.experts])
  wd = torch.stack([e.down_proj.weight.detach() for e in m.experts])
  new_route = lambda f, ops: ops.moe_route(
    torch.nn.functional.linear(f.float(), m.gate_weight.float()).contiguous(),
    m.e_score_correction_bias.float().contiguous(), 2, 1, 1, 1, 1.0, False)
  sh = m.shared_experts
  shared = lambda f: (torch.nn.functional.silu(f.double() @ sh.gate_proj.weight.double().T)
                      * (f.double() @ sh.up_proj.weight.double().T)) @ sh.down_proj.weight.double().T
  return m, wgu, wd, m.route, new_route, shared


@pytest.mark.parametrize("build", [_tiny_mixtral, _tiny_dsmoe])
def test_model_route_and_capture(monkeypatch, build):
  from xotorch_amd import ops
  m, wgu, wd, old_route, new_route, shared = build()
  m.pack_grouped()
  assert m.wp_gate_up is not None
  x = (torch.randn(2, 150, 256, device="cuda") * 0.5).to(torch.bfloat16)
  flat = x.view(-1, 256)
  with torch.inference_mode():
    monkeypatch.delenv("XOT_MOE_PREFILL", raising=False)
    old = m(x)
    monkeypatch.setenv("XOT_MOE_PREFILL", "1")
    new = m(x)
    refs = [_block_ref(flat, ids.long(), w, wgu, wd) + shared(flat) for ids, w in (new_route(flat, ops), old_route(flat))]
    e_new, e_old = ((o.view(-1, 256).double() - r).abs().max().item() for o, r in zip((new, old), refs))
    print(f"max abs err vs fp64: XOT_MOE_PREFILL=1 {e_new:.5f}, unset {e_old:.5f}")
    assert e_new <= 2 * e_old, (e_new, e_old)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      captured = m(x)
    for _ in range(3):
      graph.replay()
      torch.cuda.synchronize()
      assert torch.equal(captured, new)
