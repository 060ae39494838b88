"""SwiGLU in the packed gate_up GEMM's store, and the packed-only KV cache.

The fused launch never splits K, rounds both sums to bf16 as the plain store
does and applies the expression swiglu_packed applies, so it is required to
equal swiglu_packed(skinny_gemm_packed(x, plain pack)) bit for bit wherever
that plain launch is unsplit too. The model policy hands the interleaved pack
only to such shapes; the small N of these tests would split at K >= 2048, so
the reference launch runs under XOT_SKINNY_TARGET=1 (read per call), which is
the same kernel and pack with the unsplit plan."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
  from xotorch_amd import ops
  assert ops.hip_available(), f"HIP ext must be built: {ops._hip_load_error}"
  return ops


def bt(*shape, scale=1.0, seed=0):
  g = torch.Generator(device="cuda").manual_seed(seed)
  return (torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32) * scale).to(torch.bfloat16)


_W = {}


def packs(hip, I, K):
  """(plain pack, GLU-interleaved pack) of one random [2I, K] weight; sums of
  a few units, so silu is exercised on both sides of zero."""
  if (I, K) not in _W:
    w = bt(2 * I, K, scale=2.0 / K ** 0.5, seed=I + K)
    _W[(I, K)] = (hip.pack_decode_weight(w), hip.pack_decode_weight(w[hip.glu_interleave_perm(I).cuda()]))
    assert torch.equal(_W[(I, K)][1], hip.pack_decode_weight_glu(w))
  return _W[(I, K)]


# K: one step; an odd step count at BK=64; BK=128 eligible; an odd step count at BK=128
@pytest.mark.parametrize("K", [64, 192, 2048, 2176])
@pytest.mark.parametrize("I", [64, 128])  # N = 128: the 128-row tile only; N = 256: one wide tile
def test_fused_store_equals_gemm_then_swiglu(hip, monkeypatch, I, K):
  N = 2 * I
  plain, glu = packs(hip, I, K)
  for M in (32, 96, 128, 224, 256):  # MT = 1, 3, 4, 7 (BK=64 on the wide tile), 8
    x = bt(M, 1, K, seed=M)
    monkeypatch.delenv("XOT_SKINNY_BN", raising=False)
    monkeypatch.setenv("XOT_SKINNY_TARGET", "1")
    assert hip.skinny_plan_nsplit(N, K) == 1
    want = hip.swiglu_packed(hip.skinny_gemm_packed(x, plain, N, None))
    monkeypatch.delenv("XOT_SKINNY_TARGET")
    assert want.shape == (M, 1, I) and want.float().abs().max() > 0
    tiles = (None, "128", "256") if M >= 128 and N % 256 == 0 else (None, "128")
    for bn in tiles:
      if bn is None:
        monkeypatch.delenv("XOT_SKINNY_BN", raising=False)
      else:
        monkeypatch.setenv("XOT_SKINNY_BN", bn)
      got = hip.skinny_gemm_packed_glu(x, glu, N)
      assert got.shape == want.shape and got.is_contiguous()
      assert torch.equal(got, want), (M, bn, (got.float() - want.float()).abs().max().item())
    # a wrong pairing cannot pass: the plain pack through the fused store is something else
    assert not torch.equal(hip.skinny_gemm_packed_glu(x, plain, N), want)


def test_argument_checks(hip):
  plain, glu = packs(hip, 64, 64)
  with pytest.raises(RuntimeError):
    hip.skinny_gemm_packed_glu(bt(48, 64), glu, 128)       # rows not a multiple of 32
  with pytest.raises(RuntimeError):
    hip.skinny_gemm_packed_glu(bt(32, 64), glu, 64)        # N not a multiple of 128
  with pytest.raises(RuntimeError):
    hip.skinny_gemm_packed_glu(bt(32, 64).float(), glu, 128)
  assert hip.skinny_plan_nsplit(57344, 8192) == 1 and hip.skinny_plan_nsplit(8192, 28672) > 1


# ---- rope_qkv_append without the plain tensors

@pytest.mark.parametrize("S", [1, 5])
def test_append_writes_the_same_packed_copies_without_the_plain_cache(hip, S):
  from xotorch_amd.engine.kvcache import ShardKVCache
  B, H, KVH, hd, T = 2, 2, 1, 128, 40
  both = ShardKVCache(1, B, KVH, T, hd, torch.bfloat16, "cuda").caches[0]
  only = ShardKVCache(1, B, KVH, T, hd, torch.bfloat16, "cuda", plain=False).caches[0]
  assert only.k is None and only.v is None and only.kp.shape == both.kp.shape
  g = torch.Generator(device="cuda").manual_seed(S)
  ang = torch.rand(T, hd // 2, generator=g, device="cuda") * 6.28
  cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
  pos = torch.arange(17, 17 + S, dtype=torch.int32, device="cuda")
  qkv = bt(B, S, (H + 2 * KVH) * hd, seed=S)
  qa, qb = qkv.clone(), qkv.clone()
  hip.rope_qkv_append(qa, cos, sin, pos, both.k, both.v, H, KVH, hd, both.kp, both.vp)
  hip.rope_qkv_append(qb, cos, sin, pos, None, None, H, KVH, hd, only.kp, only.vp)
  torch.cuda.synchronize()
  assert both.kp.float().abs().sum() > 0 and both.vp.float().abs().sum() > 0
  assert torch.equal(both.kp, only.kp) and torch.equal(both.vp, only.vp)
  assert torch.equal(qa, qb) and not torch.equal(qa, qkv)
  with pytest.raises(RuntimeError):
    hip.rope_qkv_append(qb, cos, sin, pos, None, None, H, KVH, hd)  # nothing to append to


def test_attention_without_the_plain_cache_raises_off_the_mfma_path(hip, monkeypatch):
  from xotorch_amd.engine.kvcache import ShardKVCache
  only = ShardKVCache(1, 2, 1, 40, 128, torch.bfloat16, "cuda", plain=False).caches[0]
  q = bt(2, 1, 2, 128)
  sl = torch.full((2,), 3, dtype=torch.int32, device="cuda")
  assert hip.attn_decode(q, None, None, sl, only.kp, only.vp).shape == q.shape  # kv heads and capacity from kp
  monkeypatch.setenv("XOT_MFMA_ATTN", "0")  # toggled after the cache was built
  with pytest.raises(RuntimeError, match="plain KV cache"):
    hip.attn_decode(q, None, None, sl, only.kp, only.vp)
  with pytest.raises(RuntimeError, match="plain KV cache"):
    hip.attn_prefill(q, None, None, 0, 1, only.kp, only.vp)
  monkeypatch.delenv("XOT_MFMA_ATTN")
  q17 = bt(2, 1, 17, 128)  # 17 query heads per kv head: not an MFMA decode shape
  with pytest.raises(RuntimeError, match="plain KV cache"):
    hip.attn_decode(q17, None, None, sl, only.kp, only.vp)


# ---- one whole model: prefill and three decode steps, eager and under a captured graph

B, S, GEN = 32, 4, 3


def _tiny_llama(seed=11):
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import ShardedModel
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  # the tiny llama of test_skinny_mxfp4_gpu.py: head_dim 128, every projection at the packing minimum
  cfg = config_from_hf({
    "model_type": "llama", "hidden_size": 128, "num_hidden_layers": 2, "num_attention_heads": 1,
    "num_key_value_heads": 1, "head_dim": 128, "intermediate_size": 128, "vocab_size": 256,
    "rope_theta": 10000.0, "rms_norm_eps": 1e-5, "max_position_embeddings": 64,
    "tie_word_embeddings": False, "torch_dtype": "bfloat16"}, "tiny-glu")
  model = ShardedModel(cfg, Shard("tiny-glu", 0, 1, 2)).to("cuda", torch.bfloat16).eval()
  torch.manual_seed(seed)
  random_init(model)
  return cfg, model


def _tokens(cfg):
  g = torch.Generator().manual_seed(5)
  return (torch.randint(0, cfg.vocab_size, (B, S), generator=g).cuda(),
          torch.randint(0, cfg.vocab_size, (GEN, B, 1), generator=g).cuda())


def _run(cfg, model, plain, graph):
  """Logits of one prefill (B*S = 128 rows: a decode shape too) and GEN decode
  steps on fixed tokens; graph = the decode step is captured once and replayed."""
  from xotorch_amd.engine.kvcache import ShardKVCache
  cache = ShardKVCache(2, B, cfg.n_kv_heads, S + GEN, cfg.head_dim, torch.bfloat16, "cuda", plain=plain)
  assert (cache.caches[0].k is None) == (not plain) and cache.caches[0].kp is not None
  tokens, nxt = _tokens(cfg)
  tok = torch.zeros(B, 1, dtype=torch.int64, device="cuda")
  pos = torch.zeros(1, dtype=torch.int32, device="cuda")
  sl = torch.zeros(B, dtype=torch.int32, device="cuda")
  step = lambda: model(tok, caches=cache.caches, positions=pos, start_pos=-1, is_decode=True, seq_lens=sl)
  outs = []
  with torch.inference_mode():
    g = None
    if graph:  # warm up and capture before the prefill: decode overwrites these slots before it reads them
      pos.fill_(S)
      sl.fill_(S + 1)
      side = torch.cuda.Stream()
      side.wait_stream(torch.cuda.current_stream())
      with torch.cuda.stream(side):
        step()
      torch.cuda.current_stream().wait_stream(side)
      g = torch.cuda.CUDAGraph()
      with torch.cuda.graph(g):
        static_out = step()
      cache.reset()
    p0 = torch.arange(S, dtype=torch.int32, device="cuda")
    outs.append(model(tokens, caches=cache.caches, positions=p0, start_pos=0).clone())
    for i in range(GEN):
      tok.copy_(nxt[i])
      pos.fill_(S + i)
      sl.fill_(S + i + 1)
      if g is not None:
        g.replay()
        outs.append(static_out.clone())
      else:
        outs.append(step().clone())
  torch.cuda.synchronize()
  return outs


def test_model_logits_do_not_change(hip, monkeypatch):
  from xotorch_amd.models.linear import DECODE_PICKS
  monkeypatch.setenv("XOT_PACK", "all")  # the tiny down_proj is below the default policy's size rule
  for v in ("XOT_FP8_GEMM", "XOT_W4_GEMM", "XOT_FP8_KV", "XOT_MFMA_ATTN", "XOT_SKINNY_BN"):
    monkeypatch.delenv(v, raising=False)
  saved = dict(DECODE_PICKS)
  DECODE_PICKS.clear()
  try:
    for N, K in [(384, 128), (128, 128), (256, 128)]:  # qkv, o and down, gate_up and lm_head
      for M in (32, 128):
        DECODE_PICKS[(N, K, M)] = "packed"
        DECODE_PICKS[("fuse_swiglu", N, K, M)] = "split"
    monkeypatch.setenv("XOT_GLU_STORE", "0")
    cfg, old = _tiny_llama()
    assert old.pack_decode_weights(reserve_bytes=0) > 0
    assert not any(l.mlp.gate_up_proj.glu_packed for l in old.layers.values())
    monkeypatch.delenv("XOT_GLU_STORE")
    _, new = _tiny_llama()
    assert new.pack_decode_weights(reserve_bytes=0) > 0
    assert all(l.mlp.gate_up_proj.glu_packed for l in new.layers.values())
    want = _run(cfg, old, plain=True, graph=False)
    assert len(want) == 1 + GEN
    for b in want:
      assert torch.isfinite(b.float()).all() and b.float().abs().max() > 0
    assert not torch.equal(want[1], want[2])
    runs = {(name, plain, graph): _run(cfg, model, plain, graph)
            for name, model in (("XOT_GLU_STORE=0", old), ("default", new))
            for plain in (True, False) for graph in (False, True)}
  finally:
    DECODE_PICKS.clear()
    DECODE_PICKS.update(saved)
  for key, got in runs.items():
    for step, (a, b) in enumerate(zip(got, want)):
      assert torch.equal(a, b), (key, step, (a.float() - b.float()).abs().max().item())
