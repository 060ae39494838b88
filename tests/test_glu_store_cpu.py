"""The GLU-interleaved pack (SwiGLU in the gate_up GEMM's store), the policy
that hands it out, and the packed-only KV cache: everything that has no
kernel in it."""
import pytest
import torch

from xotorch_amd import ops
from xotorch_amd.engine.kvcache import LayerKV, ShardKVCache


# ---- the permutation

@pytest.mark.parametrize("I", [64, 128, 192])
def test_perm_is_a_bijection(I):
  perm = ops.glu_interleave_perm(I)
  assert perm.shape == (2 * I,)
  assert sorted(perm.tolist()) == list(range(2 * I))


@pytest.mark.parametrize("I", [64, 128, 192])
def test_rows_eight_apart_are_gate_and_up_of_one_column(I):
  perm = ops.glu_interleave_perm(I).tolist()
  seen = []
  for rho in range(2 * I):
    if rho % 16 < 8:
      c = perm[rho]
      assert c < I and perm[rho + 8] == I + c, (rho, c, perm[rho + 8])
      seen.append(c)
  assert sorted(seen) == list(range(I))


@pytest.mark.parametrize("I", [64, 128, 192])
def test_store_columns_cover_the_output_once(I):
  """The store's column formula over (n32, p, lane >> 5, j), and the pair of
  accumulators it reads there: D-layout n_local = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)."""
  perm = ops.glu_interleave_perm(I).tolist()
  cols = []
  for n32 in range(2 * I // 32):
    for p in range(2):
      for half in range(2):
        for j in range(4):
          col = 16 * n32 + 8 * p + 4 * half + j
          cols.append(col)
          for r, want in ((8 * p + j, col), (8 * p + 4 + j, I + col)):  # gate acc, up acc
            n_local = (r & 3) + 8 * (r >> 2) + 4 * half
            assert perm[32 * n32 + n_local] == want
  assert sorted(cols) == list(range(I))


def test_glu_pack_is_the_plain_pack_of_the_permuted_rows():
  torch.manual_seed(0)
  for I, K in ((64, 64), (192, 128)):
    w = torch.randn(2 * I, K).to(torch.bfloat16)
    assert torch.equal(ops.pack_decode_weight_glu(w), ops.pack_decode_weight(w[ops.glu_interleave_perm(I)]))


# ---- the policy

LLAMA = {
  "model_type": "llama", "hidden_size": 128, "num_hidden_layers": 2,
  "num_attention_heads": 2, "num_key_value_heads": 1, "intermediate_size": 128,
  "vocab_size": 256, "rope_theta": 10000.0, "rms_norm_eps": 1e-5,
  "max_position_embeddings": 64, "tie_word_embeddings": False, "torch_dtype": "bfloat16",
}
MOE = dict(LLAMA, model_type="mixtral", num_local_experts=2, num_experts_per_tok=1)


def _model(raw):
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import ShardedModel
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  cfg = config_from_hf(raw, "tiny-glu")
  model = ShardedModel(cfg, Shard("tiny-glu", 0, 1, 2)).to(torch.bfloat16)
  random_init(model)
  return model.eval()


@pytest.fixture
def gpu_policy(monkeypatch):
  """The pack policy on the CPU: CUDA looks present with unlimited memory,
  pack_decode packs CPU weights, and the plan binding says "unsplit"."""
  from xotorch_amd.models import linear
  for v in ("XOT_W4_GEMM", "XOT_FP8_GEMM", "XOT_GLU_STORE"):
    monkeypatch.delenv(v, raising=False)
  monkeypatch.setenv("XOT_PACK", "all")
  monkeypatch.setattr(linear.XotLinear, "pack_decode", lambda self: self._pack() if self.packable() else None)
  monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
  monkeypatch.setattr(torch.cuda, "mem_get_info", lambda: (1 << 40, 1 << 40))
  plans = []
  monkeypatch.setattr(ops, "skinny_plan_nsplit", lambda N, K: plans.append((N, K)) or 1)
  return plans


def _flags(model):
  from xotorch_amd.models.linear import XotLinear
  return {n: (m.glu_store, m.glu_packed) for n, m in model.named_modules() if isinstance(m, XotLinear)}


def test_dense_gate_up_is_flagged_in_bf16_mode(gpu_policy):
  model = _model(LLAMA)
  model.pack_decode_weights(reserve_bytes=0)
  flags = _flags(model)
  assert len(flags) == 9
  for name, (flag, packed) in flags.items():
    assert flag == packed == name.endswith("mlp.gate_up_proj"), name
  assert gpu_policy == [(256, 128), (256, 128)]  # asked of the plan binding, not re-derived
  for lid in "01":
    gu = model.layers[lid].mlp.gate_up_proj
    w = gu.weight.detach()
    assert torch.equal(gu.weight_packed, ops.pack_decode_weight(w[ops.glu_interleave_perm(128)]))
    assert not torch.equal(gu.weight_packed, ops.pack_decode_weight(w))
    down = model.layers[lid].mlp.down_proj
    assert torch.equal(down.weight_packed, ops.pack_decode_weight(down.weight.detach()))


def test_a_shape_whose_plan_splits_is_not_flagged(gpu_policy, monkeypatch):
  monkeypatch.setattr(ops, "skinny_plan_nsplit", lambda N, K: 2)
  model = _model(LLAMA)
  model.pack_decode_weights(reserve_bytes=0)
  assert not any(flag or packed for flag, packed in _flags(model).values())
  gu = model.layers["0"].mlp.gate_up_proj
  assert torch.equal(gu.weight_packed, ops.pack_decode_weight(gu.weight.detach()))


def test_kill_switch_flags_none(gpu_policy, monkeypatch):
  monkeypatch.setenv("XOT_GLU_STORE", "0")
  model = _model(LLAMA)
  model.pack_decode_weights(reserve_bytes=0)
  assert not any(flag or packed for flag, packed in _flags(model).values())
  gu = model.layers["1"].mlp.gate_up_proj
  assert torch.equal(gu.weight_packed, ops.pack_decode_weight(gu.weight.detach()))


@pytest.mark.parametrize("mode", ["XOT_FP8_GEMM", "XOT_W4_GEMM"])
def test_fp8_and_mxfp4_are_not_flagged(gpu_policy, monkeypatch, mode):
  monkeypatch.setenv(mode, "1")
  model = _model(LLAMA)
  model.pack_decode_weights(reserve_bytes=0)
  assert not any(flag or packed for flag, packed in _flags(model).values())
  assert model.layers["0"].mlp.gate_up_proj.weight_packed is None


def test_experts_are_not_flagged(gpu_policy):
  model = _model(MOE)
  model.pack_decode_weights(reserve_bytes=0)
  flags = _flags(model)
  assert any("experts." in n and n.endswith("gate_up_proj") for n in flags)
  assert not any(flag or packed for flag, packed in flags.values())
  assert gpu_policy == []


def test_direct_pack_decode_without_the_flag_is_the_plain_pack(gpu_policy):
  model = _model(LLAMA)
  gu = model.layers["0"].mlp.gate_up_proj
  gu.pack_decode()
  assert not gu.glu_packed and torch.equal(gu.weight_packed, ops.pack_decode_weight(gu.weight.detach()))
  gu.unpack_decode()
  gu.glu_store = True
  gu.pack_decode()
  assert gu.glu_packed and gu.weight_packed is not None
  gu.unpack_decode()
  assert not gu.glu_packed and gu.weight_packed is None


def test_flagged_pack_never_reaches_the_plain_packed_arms(gpu_policy, monkeypatch):
  """A decode-shaped call of XotLinear itself on a GLU-interleaved pack goes to
  the library; MLP.forward runs the fused launch under the GEMM's own key."""
  from xotorch_amd.models import linear, llama
  monkeypatch.setattr(linear, "decode_rows", lambda x, K: x.numel() // K)
  monkeypatch.setattr(llama, "decode_rows", lambda x, K: x.numel() // K)
  monkeypatch.setattr(linear, "DECODE_PICKS", {(256, 128, 32): "packed", (128, 128, 32): "blaslt"})
  boom = lambda *a: pytest.fail("a plain packed arm ran on a GLU-interleaved pack")
  for name in ("skinny_gemm_packed", "skinny_gemm_packed_xreg", "skinny_gemm_packed_epilogue"):
    monkeypatch.setattr(ops, name, boom)
  calls = []

  def glu(x, wp, N):
    calls.append((wp, N))
    return torch.zeros(list(x.shape[:-1]) + [N // 2], dtype=x.dtype)

  monkeypatch.setattr(ops, "skinny_gemm_packed_glu", glu)
  model = _model(LLAMA)
  model.pack_decode_weights(reserve_bytes=0)
  mlp = model.layers["0"].mlp
  x = torch.randn(32, 1, 128).to(torch.bfloat16)
  with torch.no_grad():
    y = mlp.gate_up_proj(x)
    assert torch.equal(y, torch.nn.functional.linear(x, mlp.gate_up_proj.weight))
    assert calls == []
    out = mlp(x)
    assert out.shape == (32, 1, 128)
    assert len(calls) == 1 and calls[0][0] is mlp.gate_up_proj.weight_packed and calls[0][1] == 256
    linear.DECODE_PICKS[(256, 128, 32)] = "blaslt"
    want = mlp.down_proj(ops.swiglu_packed(torch.nn.functional.linear(x, mlp.gate_up_proj.weight)))
    assert torch.equal(mlp(x), want) and len(calls) == 1
  assert set(linear.DECODE_PICKS) == {(256, 128, 32), (128, 128, 32)}  # no new key


# ---- the packed-only cache

def test_plain_false_is_ignored_without_packed_copies():
  cache = ShardKVCache(2, 3, 1, 10, 128, torch.bfloat16, "cpu", plain=False)
  assert cache.plain
  for c in cache.caches:
    assert c.k.shape == c.v.shape == (3, 1, 10, 128) and c.kp is None
  ref = ShardKVCache(2, 3, 1, 10, 128, torch.bfloat16, "cpu")
  assert cache.nbytes() == ref.nbytes() == 2 * 2 * 3 * 10 * 128 * 2


def test_layerkv_rows_reset_and_nbytes_cope_with_none():
  kp = torch.ones(4, 1, 2, 4, 64, 8, dtype=torch.bfloat16)
  vp = torch.ones(4, 1, 8, 1, 64, 8, dtype=torch.bfloat16)
  kv = LayerKV(None, None, kp, vp)
  part = kv.rows(1, 3)
  assert part.k is None and part.v is None and part.ksc is None
  assert part.kp.shape[0] == 2 and part.kp.data_ptr() == kp[1:3].data_ptr()
  cache = ShardKVCache(0, 4, 1, 32, 128)
  cache.caches.append(kv)
  assert cache.rows(0, 2)[0].vp.shape[0] == 2
  assert cache.nbytes() == (kp.numel() + vp.numel()) * 2
  cache.reset()
  assert not kp.any() and not vp.any()


def test_ops_without_the_plain_cache_raise_where_they_need_it():
  q = torch.zeros(2, 1, 2, 128, dtype=torch.bfloat16)
  kp = torch.zeros(2, 1, 2, 4, 64, 8, dtype=torch.bfloat16)
  vp = torch.zeros(2, 1, 8, 1, 64, 8, dtype=torch.bfloat16)
  with pytest.raises(RuntimeError, match="plain KV cache"):
    ops.attn_decode(q, None, None, 1, kp, vp)  # CPU: the torch path reads the plain cache
  with pytest.raises(RuntimeError, match="plain KV cache"):
    ops.attn_prefill(q, None, None, 0, 1, kp, vp)
  qkv = torch.zeros(2, 1, 4 * 128, dtype=torch.bfloat16)
  cos = sin = torch.zeros(8, 64)
  with pytest.raises(RuntimeError, match="plain KV cache"):
    ops.rope_qkv_append(qkv, cos, sin, torch.zeros(1, dtype=torch.int32), None, None, 2, 1, 128, kp, vp)
