"""ShardedModel's carried-norm forward (each layer's down-projection epilogue
produces the next norm) against the per-layer-norm forward, on the dummy model
in fp32 on the CPU: the plumbing, through the torch_ref fallbacks."""
import pytest
import torch


def _models(bounds):
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import ShardedModel
  from xotorch_amd.models.registry import builtin_config
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  cfg = config_from_hf(builtin_config("dummy"), "dummy")
  torch.manual_seed(11)
  whole = ShardedModel(cfg, Shard("dummy", 0, cfg.n_layers - 1, cfg.n_layers)).float()
  random_init(whole)
  models = []
  for lo, hi in bounds:
    m = ShardedModel(cfg, Shard("dummy", lo, hi, cfg.n_layers)).float()
    m.load_state_dict({k: v for k, v in whole.state_dict().items() if k in m.state_dict()}, strict=False)
    if not hasattr(m, "embed_tokens") and hasattr(m, "lm_head"):  # tied head on a later shard
      m.lm_head.weight.data.copy_(whole.embed_tokens.weight)
    models.append(m.eval())
  return cfg, models


def _run(cfg, models, carry, last_only=True):
  from xotorch_amd.engine.kvcache import ShardKVCache
  B, S, GEN = 2, 7, 3
  caches = [ShardKVCache(m.shard.get_layer_count(), B, cfg.n_kv_heads, S + GEN, cfg.head_dim,
                         torch.float32, "cpu") for m in models]
  tokens = torch.randint(0, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(5))

  def run(x, **kw):
    for i, (m, c) in enumerate(zip(models, caches)):
      x = m(x, caches=c.caches, carry_norm=carry, **kw)
    return x

  outs = []
  with torch.inference_mode():
    logits = run(tokens, positions=torch.arange(S), start_pos=0, last_only=last_only)
    outs.append(logits)
    cur = logits.reshape(B, -1, cfg.vocab_size)[:, -1].argmax(dim=-1, keepdim=True)
    for i in range(GEN):
      logits = run(cur, positions=torch.tensor([S + i]), start_pos=S + i, is_decode=True)
      outs.append(logits)
      cur = logits.argmax(dim=-1, keepdim=True)
  return outs


@pytest.mark.parametrize("bounds", [[(0, 3)], [(0, 1), (2, 3)]])
@pytest.mark.parametrize("last_only", [True, False])
def test_carried_norm_forward_equals_layer_norm_forward(bounds, last_only):
  cfg, models = _models(bounds)
  ref = _run(cfg, models, False, last_only)
  got = _run(cfg, models, True, last_only)
  assert len(ref) == len(got) == 4
  for step, (a, b) in enumerate(zip(ref, got)):
    assert a.shape == b.shape and torch.isfinite(a).all()
    assert torch.equal(a, b), (step, (a - b).abs().max().item())


def test_carried_norm_hands_each_layer_the_next_norm_weight(monkeypatch):
  """Layer i is given layer i+1's input norm weight; the last layer of the last
  shard the final norm's in decode and None where the final norm sees a
  sliced h; the end of a non-last shard None."""
  from xotorch_amd.models.llama import DecoderLayer
  cfg, models = _models([(0, 1), (2, 3)])
  seen = []
  orig = DecoderLayer.forward_carry

  def spy(self, x, normed_in, next_norm_w, *a, **kw):
    seen.append((normed_in is None, next_norm_w))
    return orig(self, x, normed_in, next_norm_w, *a, **kw)

  monkeypatch.setattr(DecoderLayer, "forward_carry", spy)
  _run(cfg, models, True)
  m0, m1 = models
  prefill, decode = seen[:4], seen[4:8]
  for step, final_w in ((prefill, None), (decode, m1.norm.weight)):
    assert [first for first, _ in step] == [True, False, True, False]
    assert step[0][1] is m0.layers["1"].input_layernorm.weight
    assert step[1][1] is None
    assert step[2][1] is m1.layers["3"].input_layernorm.weight
    assert step[3][1] is final_w
