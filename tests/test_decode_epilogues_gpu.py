"""The decode step's fused reduce / epilogue launches against the launches they
replace, bit for bit: the in-workgroup split-KV merge of attn_decode_mfma
(XOT_ATTN_FUSED_MERGE) against workspace + attn_decode_merge, the down
projection's row epilogue against combine -> bf16 add -> rmsnorm, and the
model's carried norm (XOT_FUSE_EPILOGUE) against the per-layer norms."""
import pytest
import torch

from attn_oracle import pack_k as _pack_k, pack_v as _pack_v  # reference packers of the MFMA cache images

pytestmark = pytest.mark.gpu

HD = 128


def bt(*shape, scale=1.0, seed=0):
  g = torch.Generator(device="cuda").manual_seed(seed)
  return (torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32) * scale).to(torch.bfloat16)


@pytest.fixture(scope="module")
def hipmod():
  from xotorch_amd import ops
  assert ops.hip_available(), f"HIP ext must be built: {ops._hip_load_error}"
  from xotorch_amd.ops import _hip_ops
  return _hip_ops


# ---------------- attention: in-workgroup merge vs workspace + merge launch ----------------

# B = 3, KVH = 2: 6 * nsplit waves, so the last 4-wave workgroup is partly
# filled at nsplit 1 and 2. The launcher picks nsplit from the capacity T.
# Lengths are ragged: sl = 1, a length inside the first 32-position chunk
# (every later split empty: l = 0), and the full capacity.
_ATTN_CASES = [
  # H, T, seq_lens, nsplit the launcher picks
  (16, 32, [1, 17, 32], 1),
  (16, 64, [1, 20, 64], 2),
  (16, 128, [1, 33, 128], 4),
  (16, 512, [1, 40, 512], 16),   # > 4: the workspace path stays in use
  (32, 128, [1, 33, 128], 4),    # NQ = 16: every row of the MFMA tile is real
]


@pytest.fixture(scope="module")
def attn_inputs(hipmod):
  """Per (H, T): q, plain caches for the reference, bf16- and fp8-packed
  copies (appended by rope_qkv_append, as the model does)."""
  from xotorch_amd.ops.torch_ref import rope_cos_sin
  made = {}
  B, KVH = 3, 2
  for H, T, _, _ in _ATTN_CASES:
    qkv = bt(B, T, (H + 2 * KVH) * HD, seed=300 + H + T, scale=0.5)
    kc = torch.zeros(B, KVH, T, HD, dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    kp8 = torch.zeros(B, KVH, T // 16, 4, 64, 8, dtype=torch.uint8, device="cuda")
    vp8 = torch.zeros(B, KVH, 8, T // 32, 64, 8, dtype=torch.uint8, device="cuda")
    ksc = torch.ones(B, KVH, T, dtype=torch.float32, device="cuda")
    vsc = torch.ones_like(ksc)
    cos, sin = rope_cos_sin(HD, T, 10000.0, device="cuda")
    pos = torch.arange(T, dtype=torch.int32, device="cuda")
    hipmod.rope_qkv_append(qkv.clone(), cos, sin, pos, kc, vc, H, KVH, HD)
    hipmod.rope_qkv_append(qkv.clone(), cos, sin, pos, kc.clone(), vc.clone(), H, KVH, HD, kp8, vp8,
                           k_scale=ksc, v_scale=vsc)
    q = bt(B, 1, H, HD, seed=301 + H + T, scale=0.5)
    made[(H, T)] = dict(q=q, kc=kc, vc=vc, kp=_pack_k(kc, T), vp=_pack_v(vc, T),
                        kp8=kp8, vp8=vp8, ksc=ksc, vsc=vsc)
  return made


@pytest.mark.parametrize("prefetch", [True, False])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("H,T,sls,nsplit", _ATTN_CASES)
def test_attn_fused_merge_equals_merge_launch(hipmod, attn_inputs, monkeypatch, H, T, sls, nsplit,
                                              fp8, prefetch):
  from xotorch_amd.ops import torch_ref
  c = attn_inputs[(H, T)]
  sl_t = torch.tensor(sls, dtype=torch.int32, device="cuda")
  if not prefetch:
    monkeypatch.setenv("XOT_ATTN_PREFETCH", "0")

  def run():
    if fp8:
      return hipmod.attn_decode_mfma(c["q"], c["kp8"], c["vp8"], sl_t, T,
                                     k_scale=c["ksc"], v_scale=c["vsc"])
    return hipmod.attn_decode_mfma(c["q"], c["kp"], c["vp"], sl_t, T)

  monkeypatch.setenv("XOT_ATTN_FUSED_MERGE", "0")
  old = run()
  monkeypatch.delenv("XOT_ATTN_FUSED_MERGE")
  new = run()
  assert new.shape == old.shape == c["q"].shape
  assert torch.equal(old, new), (nsplit, (old.float() - new.float()).abs().max().item())
  for b, s in enumerate(sls):
    ref = torch_ref.attn_decode(c["q"][b:b + 1], c["kc"][b:b + 1, :, :s], c["vc"][b:b + 1, :, :s], s).float()
    o = new[b:b + 1].float()
    err = (o - ref).abs().max().item()
    print(f"H={H} T={T} fp8={fp8} b={b} sl={s} max abs err {err:.4g}")
    if fp8:  # the fp8-KV bound of test_attn_decode_mfma_prefetch_off_equals_on
      assert err < 0.12 * max(ref.abs().max().item(), 1.0) + 0.05, (b, err)
    else:
      assert torch.allclose(o, ref, atol=3e-2, rtol=3e-2), (b, err)


# ---------------- row epilogue vs combine -> bf16 add -> rmsnorm ----------------

EPS = 1e-5

# (M, K, N): K = 4096 splits 4 ways at every N here; N = 128 is a row shorter
# than one 2048-element pass, 2176 crosses the pass boundary, 8192 is the real
# width. K = 1024 does not split: the GEMM writes bf16 y, the epilogue reads it.
_ROW_SHAPES = [(M, 4096, N) for M in (32, 128) for N in (128, 2176, 8192)] + [(32, 1024, 256)]
# (bias, norm weight, w_bias)
_ROW_MODES = [(False, True, 0.0), (True, True, 0.0), (False, False, 0.0), (True, True, 1.0)]


def _row_chain(hipmod, y, h, w, w_bias):
  hp = y + h  # the bf16 torch add of the layer
  return hp, (hipmod.rmsnorm(hp, w, EPS, w_bias) if w is not None else None)


def _check_rows(out, hp, normed, w):
  assert len(out) == (2 if w is not None else 1)
  assert torch.equal(out[0], hp), (out[0].float() - hp.float()).abs().max().item()
  if w is not None:
    assert torch.equal(out[1], normed), (out[1].float() - normed.float()).abs().max().item()


@pytest.mark.parametrize("bias,norm,w_bias", _ROW_MODES)
@pytest.mark.parametrize("M,K,N", _ROW_SHAPES)
def test_row_epilogue_equals_chain(hipmod, M, K, N, bias, norm, w_bias):
  from xotorch_amd import ops
  x = bt(M, K, scale=0.5, seed=M + N + 11)
  wp = ops.pack_decode_weight(bt(N, K, scale=0.02, seed=K + N))
  b = bt(N, seed=13) if bias else None
  h = bt(M, N, seed=14)
  w = bt(N, seed=15) if norm else None
  hp, normed = _row_chain(hipmod, hipmod.skinny_gemm_packed(x, wp, N, b), h, w, w_bias)
  out = hipmod.skinny_gemm_packed_epilogue(x, wp, N, b, h, w, EPS, w_bias)
  _check_rows(out, hp, normed, w)


@pytest.mark.parametrize("bias,norm,w_bias", _ROW_MODES)
@pytest.mark.parametrize("M,K,N", _ROW_SHAPES)
def test_row_epilogue_swiglu_equals_chain(hipmod, M, K, N, bias, norm, w_bias):
  from xotorch_amd import ops
  gu = bt(M, 2 * K, scale=0.5, seed=M + N + 21)
  wp = ops.pack_decode_weight(bt(N, K, scale=0.02, seed=K + N + 1))
  b = bt(N, seed=23) if bias else None
  h = bt(M, N, seed=24)
  w = bt(N, seed=25) if norm else None
  hp, normed = _row_chain(hipmod, hipmod.skinny_gemm_packed_swiglu(gu, wp, N, b), h, w, w_bias)
  out = hipmod.skinny_gemm_packed_swiglu_epilogue(gu, wp, N, b, h, w, EPS, w_bias)
  _check_rows(out, hp, normed, w)


@pytest.mark.parametrize("shape", [(3, 1, 64), (5, 1, 2176), (2, 3, 8192), (1, 1, 16384)])
@pytest.mark.parametrize("norm,w_bias", [(True, 0.0), (True, 1.0), (False, 0.0)])
def test_add_rmsnorm_equals_add_then_rmsnorm(hipmod, shape, norm, w_bias):
  from xotorch_amd import ops
  y = bt(*shape, seed=31)
  h = bt(*shape, seed=32)
  w = bt(shape[-1], seed=33) if norm else None
  hp, normed = _row_chain(hipmod, y, h, w, w_bias)
  got_h, got_n = ops.add_rmsnorm(y, h, w, EPS, w_bias)
  assert got_h.shape == y.shape and torch.equal(got_h, hp)
  if norm:
    assert torch.equal(got_n, normed)
  else:
    assert got_n is None


# ---------------- model: carried norm vs per-layer norms ----------------

def _dummy_shards(bounds):
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import ShardedModel
  from xotorch_amd.models.registry import builtin_config
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  # the built-in dummy llama, at the head_dim of the GPU attention kernels (its
  # own 16 has no HIP decode kernel): prefill and decode attention then run on
  # the packed-cache MFMA path, in-workgroup merge included
  cfg = config_from_hf(dict(builtin_config("dummy"), head_dim=128), "dummy")
  torch.manual_seed(7)
  whole = ShardedModel(cfg, Shard("dummy", 0, cfg.n_layers - 1, cfg.n_layers)).to("cuda", torch.bfloat16)
  random_init(whole)
  models = []
  for lo, hi in bounds:
    m = ShardedModel(cfg, Shard("dummy", lo, hi, cfg.n_layers)).to("cuda", torch.bfloat16)
    m.load_state_dict({k: v for k, v in whole.state_dict().items() if k in m.state_dict()}, strict=False)
    if not hasattr(m, "embed_tokens") and hasattr(m, "lm_head"):  # tied head on a later shard
      m.lm_head.weight.data.copy_(whole.embed_tokens.weight)
    models.append(m.eval())
  return cfg, models


def _decode_logits(cfg, models, fuse, monkeypatch, graph):
  """Prefill 9 tokens, then 4 decode steps (greedy); returns every step's logits."""
  from xotorch_amd.engine.kvcache import ShardKVCache
  monkeypatch.setenv("XOT_FUSE_EPILOGUE", "1" if fuse else "0")
  B, S, GEN = 3, 9, 4
  caches = [ShardKVCache(m.shard.get_layer_count(), B, cfg.n_kv_heads, S + GEN, cfg.head_dim,
                         torch.bfloat16, "cuda") for m in models]
  tokens = torch.randint(0, cfg.vocab_size, (B, S), generator=torch.Generator().manual_seed(3)).cuda()
  pos = torch.zeros(1, dtype=torch.int32, device="cuda")
  sl = torch.zeros(B, dtype=torch.int32, device="cuda")
  cur = torch.zeros(B, 1, dtype=torch.int64, device="cuda")

  def run(x, **kw):
    for m, c in zip(models, caches):
      x = m(x, caches=c.caches, **kw)
    return x

  def step(start):
    return run(cur, positions=pos, start_pos=start, is_decode=True, seq_lens=sl)

  outs = []
  with torch.inference_mode():
    logits = run(tokens, positions=torch.arange(S, dtype=torch.int32, device="cuda"), start_pos=0)
    outs.append(logits.clone())
    for i in range(GEN):
      cur.copy_(logits.argmax(dim=-1, keepdim=True))
      pos.fill_(S + i)
      sl.fill_(S + i + 1)
      if graph:
        # capture this step (lengths live in device tensors), then replay it
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
          step(S + i)  # warm-up outside capture; rewrites the same cache slot
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
          captured = step(S + i)
        g.replay()
        logits = captured.clone()
      else:
        logits = step(S + i)
      outs.append(logits.clone())
  torch.cuda.synchronize()
  return outs


@pytest.mark.parametrize("bounds,graph", [
  ([(0, 3)], False),
  ([(0, 3)], True),
  ([(0, 1), (2, 3)], False),   # shard 0 ends with no following norm
])
def test_model_carried_norm_equals_layer_norms(hipmod, monkeypatch, bounds, graph):
  cfg, models = _dummy_shards(bounds)
  off = _decode_logits(cfg, models, False, monkeypatch, graph)
  on = _decode_logits(cfg, models, True, monkeypatch, graph)
  assert len(on) == len(off) == 5
  for step, (a, b) in enumerate(zip(off, on)):
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a, b), (step, (a.float() - b.float()).abs().max().item())
