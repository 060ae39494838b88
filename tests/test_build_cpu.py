"""Shard model construction: state-dict keys and parameter order of the
three decoder shells (the GPU-side random init draws from one generator in
named_parameters() order, so the order is part of the bench's weights),
build_shard_model, the fp32 rope-table guard and the downloader's key map."""
import pytest
import torch

from xotorch_amd.models import model_class_for
from xotorch_amd.models.config import config_from_hf
from xotorch_amd.models.registry import BUILTIN_CONFIGS
from xotorch_amd.models.weights import hf_key_map, random_init
from xotorch_amd.ops.torch_ref import rope_cos_sin
from xotorch_amd.shard import Shard

GEMMA2_TINY = dict(model_type="gemma2", vocab_size=101, hidden_size=64, intermediate_size=128,
                   num_hidden_layers=4, num_attention_heads=4, num_key_value_heads=2, head_dim=16,
                   sliding_window=8, attn_logit_softcapping=50.0, final_logit_softcapping=30.0,
                   query_pre_attn_scalar=16, rms_norm_eps=1e-6, rope_theta=10000.0,
                   max_position_embeddings=64, tie_word_embeddings=True)
DS_TINY = dict(model_type="deepseek_v3", vocab_size=101, hidden_size=64, intermediate_size=128,
               moe_intermediate_size=48, num_hidden_layers=4, num_attention_heads=4,
               num_key_value_heads=4, n_routed_experts=2, num_experts_per_tok=2, n_shared_experts=1,
               n_group=1, topk_group=1, q_lora_rank=32, kv_lora_rank=16, qk_rope_head_dim=8,
               qk_nope_head_dim=16, v_head_dim=16, first_k_dense_replace=1, rms_norm_eps=1e-6,
               max_position_embeddings=64, tie_word_embeddings=False)
RAW = {
  "llama": BUILTIN_CONFIGS["dummy"],  # tied embeddings
  "qwen3": {**BUILTIN_CONFIGS["qwen-3-8b"], "num_hidden_layers": 4},
  "mixtral": {**BUILTIN_CONFIGS["mixtral-8x7b"], "num_hidden_layers": 4, "num_local_experts": 2},
  "gemma2": GEMMA2_TINY,
  "deepseek_v3": DS_TINY,
  "deepseek_v2": {**DS_TINY, "model_type": "deepseek_v2", "q_lora_rank": 0},
}
SHARDS = {"full": (0, 3), "first": (0, 1), "last": (2, 3)}

# Per-layer parameter names in named_parameters() order, written out from the
# model code before the shells were folded onto ShardBase.
_LLAMA_ATTN = ["self_attn.qkv_proj.weight", "self_attn.o_proj.weight"]
_LLAMA_MLP = ["mlp.gate_up_proj.weight", "mlp.down_proj.weight"]
_MIXTRAL_MLP = ["mlp.gate.weight",
                "mlp.experts.0.gate_up_proj.weight", "mlp.experts.0.down_proj.weight",
                "mlp.experts.1.gate_up_proj.weight", "mlp.experts.1.down_proj.weight"]
_DS_DENSE = ["mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight"]
_DS_MOE = ["mlp.gate_weight",
           "mlp.experts.0.gate_proj.weight", "mlp.experts.0.up_proj.weight", "mlp.experts.0.down_proj.weight",
           "mlp.experts.1.gate_proj.weight", "mlp.experts.1.up_proj.weight", "mlp.experts.1.down_proj.weight",
           "mlp.shared_experts.gate_proj.weight", "mlp.shared_experts.up_proj.weight",
           "mlp.shared_experts.down_proj.weight"]
_DS_NORMS = ["input_layernorm", "post_attention_layernorm"]
_DS_V3_ATTN = ["self_attn.q_a_layernorm", "self_attn.kv_a_layernorm", "self_attn.q_a_proj.weight",
               "self_attn.q_b_proj.weight", "self_attn.kv_a_proj_with_mqa.weight",
               "self_attn.kv_b_proj.weight", "self_attn.o_proj.weight"]
_DS_V2_ATTN = ["self_attn.kv_a_layernorm", "self_attn.q_proj.weight",
               "self_attn.kv_a_proj_with_mqa.weight", "self_attn.kv_b_proj.weight",
               "self_attn.o_proj.weight"]
LAYER = {
  "llama": lambda lid: ["input_layernorm.weight"] + _LLAMA_ATTN
                       + ["post_attention_layernorm.weight"] + _LLAMA_MLP,
  "qwen3": lambda lid: ["input_layernorm.weight", "self_attn.q_norm", "self_attn.k_norm"] + _LLAMA_ATTN
                       + ["post_attention_layernorm.weight"] + _LLAMA_MLP,
  "mixtral": lambda lid: ["input_layernorm.weight"] + _LLAMA_ATTN
                         + ["post_attention_layernorm.weight"] + _MIXTRAL_MLP,
  "gemma2": lambda lid: ["input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm",
                         "post_feedforward_layernorm"] + _LLAMA_ATTN + _LLAMA_MLP,
  "deepseek_v3": lambda lid: _DS_NORMS + _DS_V3_ATTN + (_DS_DENSE if lid < 1 else _DS_MOE),
  "deepseek_v2": lambda lid: _DS_NORMS + _DS_V2_ATTN + (_DS_DENSE if lid < 1 else _DS_MOE),
}
# (names before the layers, names after them) on the first / last shard. The
# llama shell's final norm is a module and follows the layers; the other two
# hold it as a parameter of the model itself, which named_parameters() lists
# first. Tied llama / gemma2 keep an lm_head copy only where embed_tokens is
# on another shard.
ENDS = {
  "llama": lambda first, last: (["embed_tokens.weight"] * first,
                                (["norm.weight"] + ["lm_head.weight"] * (not first)) * last),
  "qwen3": lambda first, last: (["embed_tokens.weight"] * first, ["norm.weight", "lm_head.weight"] * last),
  "mixtral": lambda first, last: (["embed_tokens.weight"] * first, ["norm.weight", "lm_head.weight"] * last),
  "gemma2": lambda first, last: (["norm"] * last + ["embed_tokens.weight"] * first,
                                 ["lm_head.weight"] * (last and not first)),
  "deepseek_v3": lambda first, last: (["norm"] * last + ["embed_tokens.weight"] * first,
                                      ["lm_head.weight"] * last),
  "deepseek_v2": lambda first, last: (["norm"] * last + ["embed_tokens.weight"] * first,
                                      ["lm_head.weight"] * last),
}


def _meta_model(family, span):
  cfg = config_from_hf(RAW[family], family)
  shard = Shard(family, span[0], span[1], cfg.n_layers)
  with torch.device("meta"):
    return model_class_for(cfg)(cfg, shard), cfg, shard


@pytest.mark.parametrize("span", SHARDS.values(), ids=SHARDS.keys())
@pytest.mark.parametrize("family", RAW.keys())
def test_state_dict_keys_and_parameter_order(family, span):
  model, cfg, shard = _meta_model(family, span)
  assert cfg.n_layers == 4
  assert set(model.state_dict()) == {v.split("#")[0] for v in hf_key_map(shard, cfg).values()}
  head, tail = ENDS[family](shard.is_first_layer, shard.is_last_layer)
  want = list(head)
  for lid in range(span[0], span[1] + 1):
    want += [f"layers.{lid}.{n}" for n in LAYER[family](lid)]
  assert [n for n, _ in model.named_parameters()] == want + list(tail)
  assert [n for n, _ in model.named_buffers() if "rope" in n] == ["rope_cos", "rope_sin"]


def test_build_shard_model_matches_inline_sequence():
  from xotorch_amd.models.build import build_shard_model
  from xotorch_amd.models.llama import ShardedModel
  cfg = config_from_hf(BUILTIN_CONFIGS["dummy"], "dummy")
  shard = Shard("dummy", 0, 3, 4)
  built = build_shard_model(cfg, shard, torch.float32, "cpu", seed=77)
  # the sequence the engines used to spell out
  with torch.device("meta"):
    ref = ShardedModel(cfg, shard)
  ref = ref.to_empty(device="cpu").to(torch.float32)
  random_init(ref, 77)
  ref.reset_rope()
  ref.eval()
  assert type(built) is ShardedModel and not built.training
  got, want = dict(built.named_parameters()), dict(ref.named_parameters())
  assert list(got) == list(want)
  for name in want:
    assert torch.equal(got[name], want[name]), name
  cos, sin = rope_cos_sin(cfg.head_dim, cfg.max_seq_len, cfg.rope_theta, cfg.rope_scaling)
  for got_t, want_t in ((built.rope_cos, cos), (built.rope_sin, sin)):
    assert got_t.dtype == torch.float32 and torch.isfinite(got_t).all() and torch.equal(got_t, want_t)
  assert torch.get_default_dtype() == torch.float32


def test_build_shard_model_restores_default_dtype_when_constructor_raises(monkeypatch):
  from xotorch_amd.models import build

  class Broken(torch.nn.Module):
    def __init__(self, cfg, shard):
      super().__init__()
      assert torch.get_default_dtype() == torch.bfloat16  # constructed under the target dtype
      raise RuntimeError("no such decoder")

  monkeypatch.setattr(build, "model_class_for", lambda cfg: Broken)
  cfg = config_from_hf(BUILTIN_CONFIGS["dummy"], "dummy")
  prev = torch.get_default_dtype()
  with pytest.raises(RuntimeError, match="no such decoder"):
    build.build_shard_model(cfg, Shard("dummy", 0, 3, 4), torch.bfloat16, "cpu")
  assert torch.get_default_dtype() == prev


@pytest.mark.parametrize("family", ["llama", "gemma2", "deepseek_v3"])
def test_rope_tables_stay_fp32_under_model_wide_cast(family):
  cfg = config_from_hf(RAW[family], family)
  model = model_class_for(cfg)(cfg, Shard(family, 0, 3, 4)).to(torch.bfloat16)
  rope_dim = cfg.qk_rope_head_dim if family == "deepseek_v3" else cfg.head_dim
  cos, sin = rope_cos_sin(rope_dim, cfg.max_seq_len, cfg.rope_theta, cfg.rope_scaling)
  assert model.rope_cos.dtype == torch.float32 and torch.equal(model.rope_cos, cos)
  assert model.rope_sin.dtype == torch.float32 and torch.equal(model.rope_sin, sin)
  assert next(model.parameters()).dtype == torch.bfloat16


def test_downloader_allow_patterns_use_the_architecture_key_map():
  """A DeepSeek shard's MLA and expert tensors are not in the llama key map;
  files that hold only those must still be fetched."""
  from xotorch_amd.download.downloader import shard_allow_patterns
  cfg = config_from_hf(DS_TINY, "ds-tiny")
  shard = Shard("ds-tiny", 2, 3, 4)
  weight_map = {k: "model-rest.safetensors" for k in hf_key_map(shard, cfg)}
  weight_map["model.layers.2.self_attn.kv_a_proj_with_mqa.weight"] = "model-mla.safetensors"
  for p in ("gate_proj", "up_proj", "down_proj"):
    weight_map[f"model.layers.3.mlp.experts.1.{p}.weight"] = "model-expert.safetensors"
  weight_map["model.layers.0.self_attn.o_proj.weight"] = "model-other-shard.safetensors"
  pats = shard_allow_patterns(shard, weight_map, cfg)
  assert "model-mla.safetensors" in pats
  assert "model-expert.safetensors" in pats
  assert "model-rest.safetensors" in pats
  assert "model-other-shard.safetensors" not in pats
