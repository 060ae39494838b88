"""The MXFP4 weight-only decode GEMM against the bf16 packed kernel on the
dequantized weight: every e2m1 value times a power of two is exact in bf16 and
the W4 instantiation keeps the bf16 one's staging, split-K plan and MFMA
order, so the results are required to be equal bit for bit. The dequantized
weight comes from the definition (dequant_mxfp4) on the UNPACKED images, so
the pack and the kernel are tested against it, not against each other."""
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


def spread_weight(N, K, seed):
  """Random bf16 weight whose rows and 32-blocks each carry a magnitude of
  2^-6 .. 2^6, so many scale exponents occur; rows 0 and 1 are rebuilt from
  codes that run through all 16 values (every block holds a +-6, which makes
  the round trip through the quantizer exact) under a ramp of exponents."""
  from xotorch_amd import ops
  g = torch.Generator(device="cuda").manual_seed(seed)
  row = torch.randint(-6, 7, (N, 1, 1), generator=g, device="cuda")
  blk = torch.randint(-6, 7, (N, K // 32, 1), generator=g, device="cuda")
  w = torch.randn(N, K // 32, 32, generator=g, device="cuda") * 0.02
  w = torch.ldexp(w, row + blk).view(N, K).to(torch.bfloat16)
  codes, e8 = ops.quant_mxfp4(w)
  ramp = torch.arange(K, device="cuda")
  codes[0] = (ramp % 16).to(torch.uint8)
  codes[1] = (15 - ramp % 16).to(torch.uint8)
  e8[0] = (100 + torch.arange(K // 32, device="cuda") % 50).to(torch.uint8)
  e8[1] = (150 - torch.arange(K // 32, device="cuda") % 50).to(torch.uint8)
  return ops.dequant_mxfp4(codes, e8).to(torch.bfloat16), codes, e8


_CACHE = {}


def operands(hip, N, K, seed=None):
  """(wq, ws, wp_ref): the two MXFP4 images and the bf16 pack of the weight
  dequantized from their unpacked contents; built once per (N, K, seed)."""
  key = (N, K, seed)
  if key not in _CACHE:
    w, codes, e8 = spread_weight(N, K, K + N if seed is None else seed)
    wq, ws, _ = hip.pack_decode_weight_mxfp4(w)
    c2, s2 = hip.unpack_decode_weight_mxfp4(wq, ws, N, K)
    assert torch.equal(c2, codes) and torch.equal(s2, e8)  # the constructed rows survived the quantizer
    assert len(torch.unique(c2[0])) == 16 and len(torch.unique(s2)) > 20
    w_dq = hip.dequant_mxfp4(c2, s2).to(torch.bfloat16)
    _CACHE[key] = (wq, ws, hip.pack_decode_weight(w_dq))
  return _CACHE[key]


def both_tiles(monkeypatch, fn):
  out = []
  for bn in ("128", "256"):
    monkeypatch.setenv("XOT_SKINNY_BN", bn)
    out.append(fn())
  monkeypatch.delenv("XOT_SKINNY_BN")
  return out


SHAPES = {
  "mt1": (32, 128, 1024),           # MT=1, unsplit
  "mt2_split": (64, 512, 4096),     # MT=2, split
  "a": (128, 256, 2048),            # one wide tile, nsplit 2
  "b": (128, 512, 1024),            # unsplit, two wide tiles
  "c": (256, 512, 4096),            # MT=8, nsplit 4
  "d": (128, 768, 4096 + 64),       # BK=64, 17 steps (four trips of the 4-deep ring + 1) and a 14-step last split (+ 2)
  "bk128": (128, 256, 34816),       # BK=128, 17 steps: eight trips of the 2-deep ring + 1
  "mt5": (160, 256, 2048),          # ragged staging piece
  "mt8_bk128": (256, 256, 32768),   # the wide tile stages BK=64 at MT=8
  "n384": (128, 384, 2048),         # stays on the narrow tile
  # beyond the issue's table: the ring's other corner cases
  "rest3": (32, 128, 1216),         # 19 steps: four trips + 3
  "short": (64, 128, 128),          # 2 steps, fewer than the ring holds: the prologue clamps its loads
  "one_step": (32, 128, 64),        # a single step
}


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("case", list(SHAPES))
def test_same_bits_as_bf16_kernel_on_dequantized_weight(hip, monkeypatch, case, bias):
  M, N, K = SHAPES[case]
  wq, ws, wp = operands(hip, N, K)
  x = bt(M, K, scale=0.5, seed=M + N + 1)
  b = bt(N, seed=7) if bias else None
  for bn, got, want in zip((128, 256),
                           both_tiles(monkeypatch, lambda: hip.skinny_gemm_mxfp4(x, wq, ws, 1, N, b)),
                           both_tiles(monkeypatch, lambda: hip.skinny_gemm_packed(x, wp, N, b))):
    assert got.shape == (M, N) and got.dtype == torch.bfloat16
    assert torch.isfinite(want.float()).all() and want.float().abs().max() > 0
    assert torch.equal(got, want), (bn, (got.float() - want.float()).abs().max())


@pytest.mark.parametrize("norm", [False, True])
def test_epilogue(hip, monkeypatch, norm):
  M, N, K = 128, 512, 4096
  wq, ws, wp = operands(hip, N, K)
  x = bt(M, K, scale=0.5, seed=1)
  res = bt(M, N, scale=0.5, seed=3)
  nw = (1.0 + bt(N, scale=0.1, seed=4).float()).to(torch.bfloat16) if norm else None
  got = both_tiles(monkeypatch, lambda: hip.skinny_gemm_mxfp4_epilogue(x, wq, ws, N, None, (res, nw, 1e-5)))
  want = both_tiles(monkeypatch, lambda: hip.skinny_gemm_packed_epilogue(x, wp, N, None, (res, nw, 1e-5)))
  for (h, n), (h_ref, n_ref) in zip(got, want):
    assert torch.equal(h, h_ref)
    if norm:
      assert torch.equal(n, n_ref)
    else:
      assert n is None and n_ref is None


def test_grouped(hip, monkeypatch):
  E, C, K, N = 2, 128, 2048, 256
  packs = [operands(hip, N, K, seed=100 + e) for e in range(E)]
  wq = torch.stack([p[0] for p in packs]).contiguous()
  ws = torch.stack([p[1] for p in packs]).contiguous()
  wp = torch.stack([p[2] for p in packs]).contiguous()
  x = bt(E, C, K, scale=0.5, seed=11)
  got = both_tiles(monkeypatch, lambda: hip.skinny_gemm_mxfp4(x, wq, ws, E, N))
  want = both_tiles(monkeypatch, lambda: hip.skinny_gemm_grouped(x, wp, E, N))
  for y, ref in zip(got, want):
    assert y.shape == (E, C, N)
    assert not torch.equal(ref[0], ref[1])
    assert torch.equal(y, ref)


def test_captured_graph_replay(hip):
  M, N, K = 128, 256, 2048
  wq, ws, _ = operands(hip, N, K)
  x = bt(M, K, scale=0.5, seed=2)
  want = hip.skinny_gemm_mxfp4(x, wq, ws, 1, N, None)
  torch.cuda.synchronize()
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    got = hip.skinny_gemm_mxfp4(x, wq, ws, 1, N, None)
  g.replay()
  torch.cuda.synchronize()
  assert torch.equal(got, want)


def test_argument_checks(hip):
  M, N, K = 32, 128, 1024
  wq, ws, _ = operands(hip, N, K)
  x = bt(M, K, seed=1)
  hip.skinny_gemm_mxfp4(x, wq, ws, 1, N, None)
  bad = [
    (x, wq.view(torch.int8), ws),                    # dtype of wq
    (x, wq, ws.to(torch.float32)),                   # dtype of ws
    (x, wq.view(-1)[:-1024].contiguous(), ws),       # one 64-k step of codes short
    (x, wq, ws.view(-1)[:-64].contiguous()),         # one step of scales short
    (x, torch.cat([wq, wq]), ws),                    # sizes that do not agree with N and K
    (x, wq.transpose(0, 1), ws),                     # not contiguous
    (x.float(), wq, ws),
    (bt(48, K, seed=1), wq, ws),                     # M not a multiple of 32
  ]
  for args in bad:
    with pytest.raises(RuntimeError):
      hip.skinny_gemm_mxfp4(args[0], args[1], args[2], 1, N, None)
  with pytest.raises(RuntimeError):
    hip.skinny_gemm_mxfp4(x, wq, ws, 1, 64, None)    # N not a multiple of 128
  res = bt(M, N, seed=2)
  with pytest.raises(RuntimeError):
    hip.skinny_gemm_mxfp4_epilogue(x, wq.view(torch.int8), ws, N, None, (res, None, 1e-5))
  with pytest.raises(RuntimeError):
    hip.skinny_gemm_mxfp4_epilogue(x, wq, ws.view(-1)[:-64].contiguous(), N, None, (res, None, 1e-5))


# ---- one whole model: a W4 decode against the same fake-quantized weights on the bf16 kernels

def _tiny_llama():
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import ShardedModel
  from xotorch_amd.shard import Shard
  # head_dim 128 (the MFMA attention kernels) and every projection at the packing minimum
  cfg = config_from_hf({
    "model_type": "llama", "hidden_size": 128, "num_hidden_layers": 2, "num_attention_heads": 1,
    "num_key_value_heads": 1, "head_dim": 128, "intermediate_size": 128, "vocab_size": 256,
    "rope_theta": 10000.0, "rms_norm_eps": 1e-5, "max_position_embeddings": 64,
    "tie_word_embeddings": False, "torch_dtype": "bfloat16"}, "tiny-w4")
  return cfg, ShardedModel(cfg, Shard("tiny-w4", 0, 1, 2)).to("cuda", torch.bfloat16).eval()


def _run(cfg, model, B=32, S=4, GEN=2):
  """One prefill (B*S = 128 rows: a decode shape too) and GEN decode steps on fixed tokens."""
  from xotorch_amd.engine.kvcache import ShardKVCache
  cache = ShardKVCache(2, B, cfg.n_kv_heads, S + GEN, cfg.head_dim, torch.bfloat16, "cuda")
  g = torch.Generator().manual_seed(5)
  tokens = torch.randint(0, cfg.vocab_size, (B, S), generator=g).cuda()
  nxt = torch.randint(0, cfg.vocab_size, (GEN, B, 1), generator=g).cuda()
  outs = []
  with torch.inference_mode():
    pos = torch.arange(S, dtype=torch.int32, device="cuda")
    outs.append(model(tokens, caches=cache.caches, positions=pos, start_pos=0).clone())
    for i in range(GEN):
      p = torch.full((1,), S + i, dtype=torch.int32, device="cuda")
      sl = torch.full((B,), S + i + 1, dtype=torch.int32, device="cuda")
      outs.append(model(nxt[i], caches=cache.caches, positions=p, start_pos=S + i,
                        is_decode=True, seq_lens=sl).clone())
  torch.cuda.synchronize()
  return outs


def test_model_decode_equals_bf16_kernels_on_the_quantized_weights(hip, monkeypatch):
  from xotorch_amd.models.linear import DECODE_PICKS, XotLinear
  from xotorch_amd.models.weights import random_init
  monkeypatch.setenv("XOT_PACK", "all")  # the tiny down_proj is below the default policy's size rule
  monkeypatch.delenv("XOT_FP8_GEMM", raising=False)
  saved = dict(DECODE_PICKS)
  DECODE_PICKS.clear()
  try:
    shapes = [(384, 128), (128, 128), (256, 128)]  # qkv, o and down, gate_up and lm_head
    for N, K in shapes:
      for M in (32, 128):
        DECODE_PICKS[("w4", N, K, M)] = "mxfp4"
        DECODE_PICKS[(N, K, M)] = "packed"
        DECODE_PICKS[("fuse_swiglu", N, K, M)] = "split"
    cfg, w4 = _tiny_llama()
    torch.manual_seed(11)
    random_init(w4)
    before = w4.layers["0"].mlp.down_proj.weight.detach().clone()
    monkeypatch.setenv("XOT_W4_GEMM", "1")
    assert w4.pack_decode_weights(reserve_bytes=0) > 0
    lins = [m for n, m in w4.named_modules() if isinstance(m, XotLinear) and n != "lm_head"]
    assert len(lins) == 8 and all(m.weight_packed_w4 is not None and m.weight_packed is None for m in lins)
    assert w4.lm_head.weight_packed is not None and w4.lm_head.weight_packed_w4 is None
    assert not torch.equal(w4.layers["0"].mlp.down_proj.weight.detach(), before)  # weight holds w_dq now
    got = _run(cfg, w4)

    monkeypatch.delenv("XOT_W4_GEMM")
    _, ref = _tiny_llama()
    ref.load_state_dict(w4.state_dict())  # the already fake-quantized weights
    assert ref.pack_decode_weights(reserve_bytes=0) > 0
    assert all(m.weight_packed is not None and m.weight_packed_w4 is None
               for m in ref.modules() if isinstance(m, XotLinear))
    want = _run(cfg, ref)
  finally:
    DECODE_PICKS.clear()
    DECODE_PICKS.update(saved)
  assert len(got) == 3
  for step, (a, b) in enumerate(zip(got, want)):
    assert torch.isfinite(b.float()).all() and b.float().abs().max() > 0
    assert torch.equal(a, b), (step, (a.float() - b.float()).abs().max())
