"""MXFP4 (e2m1 codes, one e8m0 scale per 32 along K) on the CPU: the
quantizer against its stated properties, the two packed images against an
independent statement of their layouts, and the W4 routing of XotLinear and
pack_decode_weights with the GPU bindings replaced by recorders."""
import pytest
import torch

from xotorch_amd import ops

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


@pytest.fixture(scope="module")
def weights():
  """bf16 N(0, 0.02^2) weights [256, 1024] with their codes, scales and dequantized values."""
  g = torch.Generator().manual_seed(0)
  w = (torch.randn(256, 1024, generator=g) * 0.02).to(torch.bfloat16)
  codes, e8 = ops.quant_mxfp4(w)
  return w, codes, e8, ops.dequant_mxfp4(codes, e8)


def test_shapes_and_ranges(weights):
  w, codes, e8, dq = weights
  assert codes.shape == (256, 1024) and codes.dtype == torch.uint8 and int(codes.max()) < 16
  assert e8.shape == (256, 32) and e8.dtype == torch.uint8
  assert dq.shape == (256, 1024) and dq.dtype == torch.float32
  assert len(torch.unique(e8)) > 1  # more than one block exponent occurs


def test_dequantized_values_are_exact_in_bf16(weights):
  _, _, _, dq = weights
  assert torch.equal(dq.to(torch.bfloat16).float(), dq)


def test_quantizer_is_idempotent(weights):
  _, codes, e8, dq = weights
  codes2, e82 = ops.quant_mxfp4(dq.to(torch.bfloat16))
  assert torch.equal(codes2, codes) and torch.equal(e82, e8)


def test_error_is_half_the_local_spacing(weights):
  """In units of the block scale: |v| <= 6 errs by at most half the grid
  spacing where v lies; 6 < |v| < 8 (which e = floor(log2 amax) - 2 allows)
  saturates at 6 and errs by |v| - 6."""
  w, _, e8, dq = weights
  scale = torch.ldexp(torch.ones(()), e8.to(torch.int32) - 127).repeat_interleave(32, dim=1)
  v = w.float() / scale
  err = (dq / scale - v).abs()
  a = v.abs()
  assert float(a.max()) < 8.0
  assert float(a.view(256, 32, 32).amax(-1).min()) >= 4.0  # the OCP exponent: every block's amax in [4, 8)
  half = torch.where(a <= 2.0, 0.25, torch.where(a <= 4.0, 0.5, 1.0))
  inside = a <= 6.0
  assert bool((err[inside] <= half[inside]).all())
  assert torch.equal(err[~inside], a[~inside] - 6.0)
  share = 1.0 - inside.float().mean().item()
  print(f"saturating share {share:.4f}")
  assert 0.0 < share < 0.05


def _block(vals):
  """A [32, 64] weight whose row 0 starts with vals, then a 4.0 that pins the block scale to 1."""
  w = torch.zeros(32, 64)
  w[0, :len(vals)] = torch.tensor(vals)
  w[0, 31] = 4.0
  return w.to(torch.bfloat16)


def test_every_code_round_trips():
  codes = torch.zeros(32, 64, dtype=torch.uint8)
  codes[0, :16] = torch.arange(16, dtype=torch.uint8)
  e8 = torch.full((32, 2), 127, dtype=torch.uint8)
  e8[0, 0] = 120
  dq = ops.dequant_mxfp4(codes, e8)
  want = torch.cat([GRID, -GRID]) * 2.0 ** -7
  assert torch.equal(dq[0, :16], want)
  assert bool(torch.signbit(dq[0, 8]))  # code 8 is -0
  codes2, e82 = ops.quant_mxfp4(dq.to(torch.bfloat16))
  assert torch.equal(codes2, codes)
  assert int(e82[0, 0]) == 120  # amax 6 * 2^-7: floor(log2) - 2 = -7


def test_ties_go_to_the_even_code():
  ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
  even = [0, 2, 2, 4, 4, 6, 6]  # 0, 1, 1, 2, 2, 4, 4
  codes, e8 = ops.quant_mxfp4(_block(ties + [-t for t in ties]))
  assert int(e8[0, 0]) == 127
  assert codes[0, :7].tolist() == even
  assert codes[0, 7:14].tolist() == [c | 8 for c in even]
  # just past a tie the nearer neighbour wins (bf16 has the bits at these magnitudes)
  codes, _ = ops.quant_mxfp4(_block([0.251953125, 0.74609375, 2.515625, 4.96875]))
  assert codes[0, :4].tolist() == [1, 1, 5, 6]


def test_all_zero_block_and_saturation():
  w = torch.zeros(32, 64, dtype=torch.bfloat16)
  w[1, 32:] = 7.5  # amax 7.5 -> scale 1, saturates at 6
  codes, e8 = ops.quant_mxfp4(w)
  assert int(e8[0, 0]) == 127 and int(codes[0].max()) == 0
  assert int(e8[1, 0]) == 127 and int(e8[1, 1]) == 127
  assert codes[1, 32:].tolist() == [7] * 32
  assert torch.equal(ops.dequant_mxfp4(codes, e8)[1, 32:], torch.full((32,), 6.0))


def test_tiny_and_huge_blocks_clamp_the_exponent():
  w = torch.zeros(32, 64)
  w[0, 0] = 2.0 ** -130  # a bf16 subnormal: e would be -132
  w[0, 32] = 2.0 ** -123  # the smallest amax that needs no clamp: e = -125
  w[1, 0] = 2.0 ** 127 * 1.5  # e = 125 exactly
  w = w.to(torch.bfloat16)
  assert float(w[0, 0]) == 2.0 ** -130
  codes, e8 = ops.quant_mxfp4(w)
  assert int(e8[0, 0]) == 2 and int(codes[0, 0]) == 0  # 2^-130 / 2^-125 = 2^-5 rounds to zero
  assert int(e8[0, 1]) == 2 and int(codes[0, 32]) == 6  # 4 * 2^-125
  assert int(e8[1, 0]) == 252 and int(codes[1, 0]) == 7  # 6 * 2^125
  dq = ops.dequant_mxfp4(codes, e8)
  assert torch.isfinite(dq).all() and float(dq[1, 0]) == 6.0 * 2.0 ** 125
  nz = dq[dq != 0].abs()
  assert float(nz.min()) >= 2.0 ** -126  # normal in bf16 and fp32


def test_quant_refuses_unpackable_shapes():
  with pytest.raises(AssertionError):
    ops.quant_mxfp4(torch.zeros(32, 32))
  with pytest.raises(AssertionError):
    ops.quant_mxfp4(torch.zeros(16, 64))


# ---- the packed images

def test_unpack_inverts_pack(weights):
  w, codes, e8, dq = weights
  wq, ws, w_dq = ops.pack_decode_weight_mxfp4(w)
  assert wq.shape == (8, 16, 64, 16) and wq.dtype == torch.uint8 and wq.is_contiguous()
  assert ws.shape == (8, 16, 32, 2) and ws.dtype == torch.uint8 and ws.is_contiguous()
  assert w_dq.dtype == torch.bfloat16 and torch.equal(w_dq.float(), dq)
  c2, s2 = ops.unpack_decode_weight_mxfp4(wq, ws, 256, 1024)
  assert torch.equal(c2, codes) and torch.equal(s2, e8)
  assert wq.numel() + ws.numel() == 256 * 1024 * 17 // 32


def test_large_weight_packs_in_row_chunks_to_the_same_images():
  g = torch.Generator().manual_seed(1)
  w = (torch.randn(4096 + 64, 64, generator=g) * 0.02).to(torch.bfloat16)
  wq, ws, w_dq = ops.pack_decode_weight_mxfp4(w)
  codes, e8 = ops.quant_mxfp4(w)
  c2, s2 = ops.unpack_decode_weight_mxfp4(wq, ws, *w.shape)
  assert torch.equal(c2, codes) and torch.equal(s2, e8)
  assert torch.equal(w_dq.float(), ops.dequant_mxfp4(codes, e8))


def _code_at(wq, K, n, k):
  """The layout of the code image, stated independently of the pack: a 32-row
  tile and a 64-k step are 1 KB, lane = (k-half)*32 + row holds 16 B, dword u
  is k16-chunk u, and element j of the lane's 8 sits in nibble j."""
  tile, row, step, kk = n // 32, n % 32, k // 64, k % 64
  u, half, j = kk // 16, (kk % 16) // 8, kk % 8
  off = ((tile * (K // 64) + step) * 64 + half * 32 + row) * 16 + u * 4 + j // 2
  byte = int(wq.reshape(-1)[off])
  return (byte >> 4) if j % 2 else (byte & 15)


def _scale_at(ws, K, n, k):
  """The scale image: per tile and 64-k step, 32 rows of 2 bytes, one per 32-block."""
  off = ((n // 32 * (K // 64) + k // 64) * 32 + n % 32) * 2 + (k % 64) // 32
  return int(ws.reshape(-1)[off])


def test_image_layouts(weights):
  w, codes, e8, _ = weights
  wq, ws, _ = ops.pack_decode_weight_mxfp4(w)
  K = 1024
  g = torch.Generator().manual_seed(2)
  picks = [(37, 93), (0, 0), (255, 1023), (31, 63), (32, 64)]
  picks += [(int(n), int(k)) for n, k in zip(torch.randint(0, 256, (300,), generator=g),
                                            torch.randint(0, K, (300,), generator=g))]
  for n, k in picks:
    assert _code_at(wq, K, n, k) == int(codes[n, k]), (n, k)
    assert _scale_at(ws, K, n, k) == int(e8[n, k // 32]), (n, k)
  # (n, k) = (37, 93) by hand: tile 1, row 5, step 1, k % 64 = 29 -> chunk 1, upper k-half,
  # element 5 -> lane 37, byte 4 + 2 of the lane, upper nibble; 32-block 0 of the step
  flat = wq.reshape(-1)
  assert int(flat[((1 * 16 + 1) * 64 + 37) * 16 + 6]) >> 4 == int(codes[37, 93])
  assert int(ws.reshape(-1)[((1 * 16 + 1) * 32 + 5) * 2]) == int(e8[37, 2])


# ---- routing

def test_w4_gemm_enabled_reads_the_environment(monkeypatch):
  monkeypatch.delenv("XOT_W4_GEMM", raising=False)
  monkeypatch.delenv("XOT_FP8_GEMM", raising=False)
  assert not ops.w4_gemm_enabled() and ops.decode_weight_format() == "bf16"
  monkeypatch.setenv("XOT_W4_GEMM", "1")
  assert ops.w4_gemm_enabled() and ops.decode_weight_format() == "mxfp4"
  monkeypatch.setenv("XOT_FP8_GEMM", "1")
  with pytest.raises(RuntimeError):
    ops.decode_weight_format()


@pytest.fixture
def w4(monkeypatch):
  """W4 mode on the CPU: pack_decode packs CPU weights, every 32-row x is a
  decode shape, the picks are empty and the two mxfp4 bindings record their calls."""
  from xotorch_amd.models import linear
  monkeypatch.setenv("XOT_W4_GEMM", "1")
  monkeypatch.delenv("XOT_FP8_GEMM", raising=False)
  monkeypatch.setattr(linear.XotLinear, "pack_decode", lambda self: self._pack() if self.packable() else None)
  monkeypatch.setattr(linear, "decode_rows", lambda x, K: x.numel() // K)
  monkeypatch.setattr(linear, "DECODE_PICKS", {})
  calls = []

  def gemm(x, wq, ws, E, N, bias=None):
    calls.append(("mxfp4", wq, ws, E, N, bias))
    return torch.zeros(list(x.shape[:-1]) + [N], dtype=x.dtype)

  def gemm_epilogue(x, wq, ws, N, bias, epilogue):
    calls.append(("mxfp4_epilogue", wq, ws, N, bias, epilogue))
    return epilogue[0], None

  monkeypatch.setattr(ops, "skinny_gemm_mxfp4", gemm)
  monkeypatch.setattr(ops, "skinny_gemm_mxfp4_epilogue", gemm_epilogue)
  return linear, calls


def _linear(linear, N=128, K=64):
  torch.manual_seed(3)
  lin = linear.XotLinear(K, N, bias=False).to(torch.bfloat16)
  return lin, lin.weight.detach().clone()


def test_packed_linear_calls_the_mxfp4_binding(w4):
  linear, calls = w4
  lin, w0 = _linear(linear)
  lin.pack_decode()
  wq, ws, w_dq = ops.pack_decode_weight_mxfp4(w0)
  assert torch.equal(lin.weight_packed_w4, wq) and torch.equal(lin.weight_scale_w4, ws)
  assert torch.equal(lin.weight.detach(), w_dq) and not torch.equal(w_dq, w0)  # weight now holds w_dq
  assert lin.weight_packed is None and lin.weight_packed_fp8 is None
  linear.DECODE_PICKS[("w4", 128, 64, 32)] = "mxfp4"
  x = torch.zeros(32, 1, 64, dtype=torch.bfloat16)
  with torch.no_grad():
    y = lin(x)
  assert y.shape == (32, 1, 128)
  assert [c[0] for c in calls] == ["mxfp4"]
  assert calls[0][1] is lin.weight_packed_w4 and calls[0][2] is lin.weight_scale_w4 and calls[0][3:5] == (1, 128)
  res = torch.ones(32, 1, 128, dtype=torch.bfloat16)
  with torch.no_grad():
    h, normed = lin(x, (res, None, 1e-5))
  assert [c[0] for c in calls] == ["mxfp4", "mxfp4_epilogue"] and h is res and normed is None
  lin.unpack_decode()
  assert lin.weight_packed_w4 is None and lin.weight_scale_w4 is None


def test_library_pick_keeps_the_dequantized_weight(w4):
  linear, calls = w4
  lin, _ = _linear(linear)
  lin.pack_decode()
  linear.DECODE_PICKS[("w4", 128, 64, 32)] = "blaslt"
  x = torch.randn(32, 64).to(torch.bfloat16)
  with torch.no_grad():
    y = lin(x)
  assert calls == []
  assert torch.equal(y, torch.nn.functional.linear(x, lin.weight))


TINY = {
  "model_type": "llama", "hidden_size": 128, "num_hidden_layers": 2,
  "num_attention_heads": 2, "num_key_value_heads": 1, "intermediate_size": 128,
  "vocab_size": 256, "rope_theta": 10000.0, "rms_norm_eps": 1e-5,
  "max_position_embeddings": 64, "tie_word_embeddings": False, "torch_dtype": "bfloat16",
}


def _tiny_model():
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import ShardedModel
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  cfg = config_from_hf(TINY, "tiny-w4")
  model = ShardedModel(cfg, Shard("tiny-w4", 0, 1, 2)).to(torch.bfloat16)
  random_init(model)
  return model.eval()


def test_pack_decode_weights_in_w4_mode(w4, monkeypatch):
  """Every group packs MXFP4 except lm_head, which keeps its weight and a
  bf16 pack; the byte count is 17/32 per quantized weight plus 2 per lm_head weight."""
  from xotorch_amd.models.linear import XotLinear
  monkeypatch.setenv("XOT_PACK", "all")  # the tiny down_proj is below the default's size rule
  monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
  monkeypatch.setattr(torch.cuda, "mem_get_info", lambda: (1 << 40, 1 << 40))
  model = _tiny_model()
  head0 = model.lm_head.weight.detach().clone()
  packed = model.pack_decode_weights(reserve_bytes=0)
  quantized = 0
  for name, mod in model.named_modules():
    if not isinstance(mod, XotLinear):
      continue
    if name == "lm_head":
      assert mod.weight_packed is not None and mod.weight_packed_w4 is None
      assert torch.equal(mod.weight.detach(), head0)
      assert torch.equal(mod.weight_packed, ops.pack_decode_weight(head0))
    else:
      assert mod.weight_packed_w4 is not None and mod.weight_packed is None, name
      assert mod.weight_packed_w4.numel() + mod.weight_scale_w4.numel() == mod.weight.numel() * 17 // 32
      codes, e8 = ops.unpack_decode_weight_mxfp4(mod.weight_packed_w4, mod.weight_scale_w4, *mod.weight.shape)
      assert torch.equal(mod.weight.detach().float(), ops.dequant_mxfp4(codes, e8)), name
      quantized += mod.weight.numel()
  assert quantized == 2 * (256 * 128 + 128 * 128 + 256 * 128 + 128 * 128)  # qkv, o, gate_up, down per layer
  assert packed == quantized * 17 // 32 + head0.numel() * 2


def test_partial_budget_counts_what_was_packed(w4, monkeypatch):
  """A budget that runs out inside the gate_up group: one of its two images is
  packed, nothing after it, and the count is what was packed, at 17/32."""
  from xotorch_amd.models.linear import XotLinear
  monkeypatch.setenv("XOT_PACK", "all")
  monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
  model = _tiny_model()
  mods = [m for m in model.modules() if isinstance(m, XotLinear)]

  def used():
    return sum((m.weight_packed_w4.numel() + m.weight_scale_w4.numel() if m.weight_packed_w4 is not None else 0)
               + (m.weight_packed.numel() * 2 if m.weight_packed is not None else 0) for m in mods)

  down, head, gate_up = 128 * 128 * 17 // 32, 256 * 128 * 2, 256 * 128 * 17 // 32
  budget = 2 * down + head + gate_up + gate_up // 2  # group order: down, lm_head, gate_up, qkv/o
  monkeypatch.setattr(torch.cuda, "mem_get_info", lambda: (budget - used(), 1 << 40))
  packed = model.pack_decode_weights(reserve_bytes=0)
  gu = [m.weight_packed_w4 is not None for n, m in model.named_modules() if n.endswith("gate_up_proj")]
  assert gu == [True, False]
  assert packed == used() == 2 * down + head + gate_up


def test_both_modes_together_raise_at_pack_time(w4, monkeypatch):
  linear, _ = w4
  monkeypatch.setenv("XOT_FP8_GEMM", "1")
  lin, w0 = _linear(linear)
  with pytest.raises(RuntimeError):
    lin.pack_decode()
  assert torch.equal(lin.weight.detach(), w0) and lin.weight_packed_w4 is None
  with pytest.raises(RuntimeError):
    _tiny_model().pack_decode_weights(reserve_bytes=0)


def test_mlp_takes_the_split_route_in_w4_mode(w4, monkeypatch):
  """No bf16 pack on down_proj: swiglu_packed, then the down projection with the epilogue."""
  linear, calls = w4
  from xotorch_amd.models import llama
  monkeypatch.setattr(llama, "decode_rows", lambda x, K: x.numel() // K)
  model = _tiny_model()
  mlp = model.layers["0"].mlp
  mlp.gate_up_proj.pack_decode()
  mlp.down_proj.pack_decode()
  linear.DECODE_PICKS[("w4", 256, 128, 32)] = "mxfp4"
  linear.DECODE_PICKS[("w4", 128, 128, 32)] = "mxfp4"
  x = torch.zeros(32, 1, 128, dtype=torch.bfloat16)
  res = torch.ones(32, 1, 128, dtype=torch.bfloat16)
  with torch.no_grad():
    h, normed = mlp(x, (res, None, 1e-5))
  assert [c[0] for c in calls] == ["mxfp4", "mxfp4_epilogue"]
  assert calls[1][1] is mlp.down_proj.weight_packed_w4 and h is res
  assert not any(k[0] == "fuse_swiglu" for k in linear.DECODE_PICKS)
