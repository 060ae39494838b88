"""head_dim 256 (gemma2-9b) through the packed-cache attention path: fused
append, fragment-packed cache (bf16 and fp8), MFMA decode with both split-KV
epilogues, MFMA prefill, the cache shapes, and a tiny gemma2 model eager and
under graph capture. Reference: ops/torch_ref.py in fp32; tolerances are the
ones the same kernels are held to at head_dim 128."""
import pytest
import torch

import attn_oracle as ao

pytestmark = pytest.mark.gpu

HD = 256


@pytest.fixture(scope="module")
def hip():
  from xotorch_amd import ops
  assert ops.hip_available(), f"HIP ext must be built: {ops._hip_load_error}"
  return ops


def rnd(*shape, scale=1.0, seed=0):
  """Random bf16 on the GPU from a seeded generator."""
  g = torch.Generator(device="cuda").manual_seed(seed)
  return (torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32) * scale).to(torch.bfloat16)


# Reference packers for the two fragment layouts at a general head dim: tests/attn_oracle.py
_pack_k, _pack_v, _unpack_k, _unpack_v = ao.pack_k, ao.pack_v, ao.unpack_k, ao.unpack_v


def _e4m3_bound(x, scale):
  """|dequant - x| bound for an e4m3 row quantized at `scale`: 3 mantissa bits
  (2^-4 relative), x itself a bf16 rounding of the quantized fp32 value
  (2^-8 relative), smallest subnormal 2^-9 in units of the scale."""
  return (2.0 ** -4 + 2.0 ** -8) * x.abs() + scale * 2.0 ** -9


def _packed_zeros(B, KVH, t32, dtype):
  kp = torch.zeros(B, KVH, t32 // 16, HD // 32, 64, 8, dtype=dtype, device="cuda")
  vp = torch.zeros(B, KVH, HD // 16, t32 // 32, 64, 8, dtype=dtype, device="cuda")
  return kp, vp


def _close(out, ref, tol):
  err = (out.float() - ref.float()).abs().max().item()
  print(f"max abs err {err:.4g} (ref max {ref.float().abs().max().item():.4g})")
  return torch.allclose(out.float(), ref.float(), atol=tol, rtol=tol), err


# ---------------- 1. append ----------------

def test_append_packed_and_plain(hip):
  """kp / vp are the reference packers of the plain caches the same call
  wrote; plain caches and rotated q match torch_ref."""
  from xotorch_amd.ops import _hip_ops, torch_ref
  B, S, H, KVH, T = 2, 48, 4, 2, 64
  qkv = rnd(B, S, (H + 2 * KVH) * HD, seed=61)
  qkv_ref = qkv.clone()
  cos, sin = torch_ref.rope_cos_sin(HD, T, 10000.0, device="cuda")
  kc = torch.zeros(B, KVH, T, HD, dtype=torch.bfloat16, device="cuda")
  vc = torch.zeros_like(kc)
  kc_ref, vc_ref = kc.clone(), vc.clone()
  kp, vp = _packed_zeros(B, KVH, T, torch.bfloat16)
  pos = torch.arange(S, dtype=torch.int32, device="cuda")
  _hip_ops.rope_qkv_append(qkv, cos, sin, pos, kc, vc, H, KVH, HD, kp, vp)
  assert torch.equal(kp, _pack_k(kc, T))
  assert torch.equal(vp, _pack_v(vc, T))
  torch_ref.rope_qkv_append(qkv_ref, cos, sin, pos, kc_ref, vc_ref, H, KVH, HD)
  assert _close(qkv, qkv_ref, 2e-2)[0]
  assert _close(kc, kc_ref, 2e-2)[0]
  assert torch.equal(vc, vc_ref)
  assert (kc[:, :, :S] != 0).any(dim=2).all(), "every one of the 256 k dims is written"


def test_append_per_row_positions(hip):
  """npos == B*S: batch row 0 sits at positions 15, 16 (a 16-position K tile
  edge), row 1 at 31, 32 (a 32-position V tile edge); every layout agrees and
  nothing else is written."""
  from xotorch_amd.ops import _hip_ops, torch_ref
  B, S, H, KVH, T = 2, 2, 4, 2, 64
  qkv = rnd(B, S, (H + 2 * KVH) * HD, seed=181)
  qkv_ref = qkv.clone()
  cos, sin = torch_ref.rope_cos_sin(HD, T, 1000000.0, device="cuda")
  kc = torch.zeros(B, KVH, T, HD, dtype=torch.bfloat16, device="cuda")
  vc = torch.zeros_like(kc)
  kc_ref, vc_ref = kc.clone(), vc.clone()
  kp, vp = _packed_zeros(B, KVH, T, torch.bfloat16)
  rows = [[15, 16], [31, 32]]
  pos = torch.tensor(rows, dtype=torch.int32, device="cuda").reshape(-1)
  _hip_ops.rope_qkv_append(qkv, cos, sin, pos, kc, vc, H, KVH, HD, kp, vp)
  assert torch.equal(kp, _pack_k(kc, T))
  assert torch.equal(vp, _pack_v(vc, T))
  for b, r in enumerate(rows):
    others = [t for t in range(T) if t not in r]
    assert (kc[b, :, others] == 0).all() and (vc[b, :, others] == 0).all()
    assert (kc[b, :, r] != 0).any() and (vc[b, :, r] != 0).any()
  torch_ref.rope_qkv_append(qkv_ref, cos, sin, pos, kc_ref, vc_ref, H, KVH, HD)
  assert _close(qkv, qkv_ref, 2e-2)[0]
  assert _close(kc, kc_ref, 2e-2)[0]
  assert torch.equal(vc, vc_ref)


def test_append_qk_norm(hip):
  """Per-head q/k RMSNorm over all 256 dims, fused before the rotation; 3e-2
  is what the same variant is held to at head_dim 128 (the reference rounds
  the normalised row to bf16 before rotating, the kernel does not)."""
  from xotorch_amd.ops import _hip_ops, torch_ref
  B, S, H, KVH, T, start = 2, 4, 4, 2, 32, 5
  qkv = rnd(B, S, (H + 2 * KVH) * HD, seed=101)
  qkv_ref = qkv.clone()
  cos, sin = torch_ref.rope_cos_sin(HD, T, 1000000.0, device="cuda")
  kc = torch.zeros(B, KVH, T, HD, dtype=torch.bfloat16, device="cuda")
  vc = torch.zeros_like(kc)
  kc_ref, vc_ref = kc.clone(), vc.clone()
  kp, vp = _packed_zeros(B, KVH, T, torch.bfloat16)
  qn = (rnd(HD, seed=102).float() * 0.2 + 1.0).to(torch.bfloat16)
  kn = (rnd(HD, seed=103).float() * 0.2 + 1.0).to(torch.bfloat16)
  pos = torch.arange(start, start + S, dtype=torch.int32, device="cuda")
  _hip_ops.rope_qkv_append(qkv, cos, sin, pos, kc, vc, H, KVH, HD, kp, vp, qn, kn, 1e-6)
  torch_ref.rope_qkv_append(qkv_ref, cos, sin, pos, kc_ref, vc_ref, H, KVH, HD, qn, kn, 1e-6)
  assert torch.equal(kp, _pack_k(kc, T))
  assert torch.equal(vp, _pack_v(vc, T))
  assert _close(qkv, qkv_ref, 3e-2)[0]
  assert _close(kc, kc_ref, 3e-2)[0]
  assert torch.equal(vc, vc_ref)


# ---------------- 2. fp8 append content ----------------

def test_fp8_append_content(hip):
  """Dequantized e4m3 bytes match the plain cache rows within the e4m3 bound,
  scales are rowmax/448 over all 256 dims, unwritten positions stay zero with
  scale 1."""
  from xotorch_amd.ops import _hip_ops
  from xotorch_amd.ops.torch_ref import rope_cos_sin
  B, S, H, KVH, T = 2, 40, 8, 4, 64
  qkv = rnd(B, S, (H + 2 * KVH) * HD, seed=141, scale=0.5)
  kc = torch.zeros(B, KVH, T, HD, dtype=torch.bfloat16, device="cuda")
  vc = torch.zeros_like(kc)
  kp8, vp8 = _packed_zeros(B, KVH, T, torch.uint8)
  ksc = torch.ones(B, KVH, T, dtype=torch.float32, device="cuda")
  vsc = torch.ones_like(ksc)
  cos, sin = rope_cos_sin(HD, T, 10000.0, device="cuda")
  pos = torch.arange(S, dtype=torch.int32, device="cuda")
  _hip_ops.rope_qkv_append(qkv, cos, sin, pos, kc, vc, H, KVH, HD, kp8, vp8,
                           k_scale=ksc, v_scale=vsc)
  for name, p8, sc, plain, unpack in (("k", kp8, ksc, kc, _unpack_k), ("v", vp8, vsc, vc, _unpack_v)):
    deq = unpack(p8.view(torch.float8_e4m3fn), T).float() * sc[..., None]
    x = plain.float()
    excess = ((deq - x).abs() - _e4m3_bound(x, sc[..., None]))[:, :, :S].max().item()
    rowmax = x[:, :, :S].abs().amax(dim=-1)
    srel = (sc[:, :, :S] * 448.0 / rowmax - 1.0).abs().max().item()
    print(f"{name}: max (err - bound) {excess:.4g}, scale rel err {srel:.4g}")
    assert excess <= 0.0, (name, excess)
    assert srel <= 2.0 ** -8, (name, srel)
    assert (unpack(p8, T)[:, :, S:] == 0).all() and (sc[:, :, S:] == 1.0).all()


# ---------------- 3. decode vs torch_ref ----------------

def _decode_inputs(B, H, KVH, T, seeds=(41, 42, 43)):
  q = rnd(B, 1, H, HD, seed=seeds[0])
  k = rnd(B, KVH, T, HD, seed=seeds[1])
  v = rnd(B, KVH, T, HD, seed=seeds[2])
  t32 = (T + 31) // 32 * 32
  return q, k, v, _pack_k(k, t32), _pack_v(v, t32)


@pytest.mark.parametrize("B,H,KVH,T,sl", [
  (2, 4, 2, 128, 100),    # nsplit 4: in-workgroup merge
  (3, 16, 8, 640, 576),   # gemma2-9b NQ=2, nsplit 16: workspace + attn_decode_merge<256>
  (1, 16, 16, 64, 33),    # NQ=1
  (1, 16, 1, 64, 50),     # NQ=16
])
def test_decode(hip, B, H, KVH, T, sl):
  from xotorch_amd.ops import _hip_ops, torch_ref
  q, k, v, kp, vp = _decode_inputs(B, H, KVH, T)
  sl_t = torch.full((B,), sl, dtype=torch.int32, device="cuda")
  out = _hip_ops.attn_decode_mfma(q, kp, vp, sl_t, T)
  ref = torch_ref.attn_decode(q, k, v, sl)
  ok, err = _close(out, ref, 3e-2)
  assert ok, err


def test_decode_ragged(hip):
  from xotorch_amd.ops import _hip_ops, torch_ref
  B, H, KVH, T = 4, 8, 4, 256
  q, k, v, kp, vp = _decode_inputs(B, H, KVH, T, seeds=(51, 52, 53))
  sls = [7, 64, 130, 256]
  sl_t = torch.tensor(sls, dtype=torch.int32, device="cuda")
  out = _hip_ops.attn_decode_mfma(q, kp, vp, sl_t, T)
  for b, s in enumerate(sls):
    ref = torch_ref.attn_decode(q[b:b + 1], k[b:b + 1, :, :s], v[b:b + 1, :, :s], s)
    ok, err = _close(out[b:b + 1], ref, 3e-2)
    assert ok, (b, err)


def test_decode_strided_q(hip):
  """q as the strided view into the packed qkv row (the fused-GEMM layout)."""
  from xotorch_amd.ops import _hip_ops, torch_ref
  B, H, KVH, T, sl = 2, 4, 2, 128, 100
  _, k, v, kp, vp = _decode_inputs(B, H, KVH, T)
  qkv = rnd(B, 1, (H + 2 * KVH) * HD, seed=44)
  q = qkv[:, :, : H * HD].view(B, 1, H, HD)
  assert not q.is_contiguous()
  sl_t = torch.full((B,), sl, dtype=torch.int32, device="cuda")
  out = _hip_ops.attn_decode_mfma(q, kp, vp, sl_t, T)
  ref = torch_ref.attn_decode(q.contiguous(), k, v, sl)
  ok, err = _close(out, ref, 3e-2)
  assert ok, err


@pytest.mark.parametrize("softcap,window", [(50.0, 0), (0.0, 40), (30.0, 40)])
def test_decode_softcap_window(hip, softcap, window):
  from xotorch_amd.ops import _hip_ops, torch_ref
  B, H, KVH, T, sl = 2, 8, 4, 128, 100
  scale = 1.0 / 16.0  # query_pre_attn_scalar = 256
  q, k, v, kp, vp = _decode_inputs(B, H, KVH, T, seeds=(81, 82, 83))
  sl_t = torch.full((B,), sl, dtype=torch.int32, device="cuda")
  out = _hip_ops.attn_decode_mfma(q, kp, vp, sl_t, T, scale, softcap, window)
  ref = torch_ref.attn_decode(q, k, v, sl, scale, softcap, window)
  ok, err = _close(out, ref, 3e-2)
  assert ok, err


# ---------------- 4 / 5. prefetch, fused merge, fp8 decode ----------------

@pytest.fixture(scope="module")
def caches256(hip):
  """One rope_qkv_append of 100 positions into T=128 caches (B=2, H=8, KVH=2),
  bf16-packed and fp8-packed, plus the decode query of the last position."""
  from xotorch_amd.ops import _hip_ops
  from xotorch_amd.ops.torch_ref import rope_cos_sin
  B, S, H, KVH, T = 2, 100, 8, 2, 128
  qkv = rnd(B, S, (H + 2 * KVH) * HD, seed=171, scale=0.5)
  qkv8 = qkv.clone()
  kc = torch.zeros(B, KVH, T, HD, dtype=torch.bfloat16, device="cuda")
  vc = torch.zeros_like(kc)
  kp, vp = _packed_zeros(B, KVH, T, torch.bfloat16)
  kp8, vp8 = _packed_zeros(B, KVH, T, torch.uint8)
  ksc = torch.ones(B, KVH, T, dtype=torch.float32, device="cuda")
  vsc = torch.ones_like(ksc)
  cos, sin = rope_cos_sin(HD, T, 10000.0, device="cuda")
  pos = torch.arange(S, dtype=torch.int32, device="cuda")
  _hip_ops.rope_qkv_append(qkv, cos, sin, pos, kc, vc, H, KVH, HD, kp, vp)
  _hip_ops.rope_qkv_append(qkv8, cos, sin, pos, kc.clone(), vc.clone(), H, KVH, HD, kp8, vp8,
                           k_scale=ksc, v_scale=vsc)
  q = qkv[:, -1:, : H * HD].view(B, 1, H, HD).contiguous()
  return dict(q=q, kc=kc, vc=vc, kp=kp, vp=vp, kp8=kp8, vp8=vp8, ksc=ksc, vsc=vsc, T=T)


def _run_decode(c, sl_t, fp8, *flags):
  from xotorch_amd.ops import _hip_ops
  if fp8:
    return _hip_ops.attn_decode_mfma(c["q"], c["kp8"], c["vp8"], sl_t, c["T"], *flags,
                                     k_scale=c["ksc"], v_scale=c["vsc"])
  return _hip_ops.attn_decode_mfma(c["q"], c["kp"], c["vp"], sl_t, c["T"], *flags)


def _check_ragged(c, out, sls, fp8):
  from xotorch_amd.ops import torch_ref
  for b, s in enumerate(sls):
    ref = torch_ref.attn_decode(c["q"][b:b + 1], c["kc"][b:b + 1, :, :s], c["vc"][b:b + 1, :, :s], s).float()
    o = out[b:b + 1].float()
    err = (o - ref).abs().max().item()
    print(f"fp8={fp8} b={b} sl={s} max abs err {err:.4g} ref max {ref.abs().max().item():.4g}")
    if fp8:
      assert err < 0.12 * max(ref.abs().max().item(), 1.0) + 0.05, (b, err)
    else:
      assert torch.allclose(o, ref, atol=3e-2, rtol=3e-2), (b, err)
  if fp8:
    assert ao.fp8_cache_worst_ratio(out, c["q"], c["kp8"], c["vp8"], c["ksc"], c["vsc"], sls) <= 1.0


@pytest.mark.parametrize("fp8", [False, True])
def test_decode_prefetch_off_equals_on(hip, caches256, monkeypatch, fp8):
  """seq_lens [33, 100] at T=128 -> nsplit 4, chunk 32: batch 0 has one full
  split, a one-position split and two empty splits."""
  sls = [33, 100]
  sl_t = torch.tensor(sls, dtype=torch.int32, device="cuda")
  monkeypatch.setenv("XOT_ATTN_PREFETCH", "0")
  off = _run_decode(caches256, sl_t, fp8)
  monkeypatch.delenv("XOT_ATTN_PREFETCH")
  on = _run_decode(caches256, sl_t, fp8)
  assert torch.equal(off, on)
  _check_ragged(caches256, on, sls, fp8)


@pytest.mark.parametrize("fp8", [False, True])
def test_decode_fused_merge_off_equals_on(hip, caches256, monkeypatch, fp8):
  """The in-workgroup merge and the workspace + attn_decode_merge<256> path
  give the same bits (same shape as the prefetch test: nsplit 4)."""
  sls = [33, 100]
  sl_t = torch.tensor(sls, dtype=torch.int32, device="cuda")
  monkeypatch.setenv("XOT_ATTN_FUSED_MERGE", "0")
  off = _run_decode(caches256, sl_t, fp8)
  monkeypatch.delenv("XOT_ATTN_FUSED_MERGE")
  on = _run_decode(caches256, sl_t, fp8)
  assert torch.equal(off, on)
  _check_ragged(caches256, on, sls, fp8)


@pytest.mark.parametrize("softcap,window", [(0.0, 0), (30.0, 40)])
def test_decode_fp8(hip, caches256, softcap, window):
  """bf16 packed path vs torch_ref at the bf16 tolerance; fp8 path vs torch_ref
  and vs the bf16 packed path at the fp8 bound."""
  from xotorch_amd.ops import torch_ref
  c = caches256
  sl = 100
  sl_t = torch.full((2,), sl, dtype=torch.int32, device="cuda")
  ref = torch_ref.attn_decode(c["q"], c["kc"], c["vc"], sl, None, softcap, window).float()
  b16 = _run_decode(c, sl_t, False, 0.0, softcap, window).float()
  f8 = _run_decode(c, sl_t, True, 0.0, softcap, window).float()
  ok, err = _close(b16, ref, 3e-2)
  assert ok, err
  bound = 0.12 * max(ref.abs().max().item(), 1.0) + 0.05
  for name, other in (("torch_ref", ref), ("bf16 packed", b16)):
    err = (f8 - other).abs().max().item()
    print(f"fp8 vs {name}: max abs err {err:.4g} (bound {bound:.4g})")
    assert err < bound, (name, err)
  assert ao.fp8_cache_worst_ratio(f8, c["q"], c["kp8"], c["vp8"], c["ksc"], c["vsc"], [sl, sl], softcap, window) <= 1.0


# ---------------- 6. prefill vs torch_ref ----------------

def _prefill_inputs(B, H, KVH, S, start, t32=None):
  total = start + S
  t32 = t32 or (total + 31) // 32 * 32
  q = rnd(B, S, H, HD, seed=91)
  k = rnd(B, KVH, total, HD, seed=92)
  v = rnd(B, KVH, total, HD, seed=93)
  return q, k, v, _pack_k(k, t32), _pack_v(v, t32)


@pytest.mark.parametrize("B,H,KVH,S,start", [
  (2, 4, 2, 128, 0),
  (1, 4, 2, 200, 0),   # partial last q block
  (1, 4, 2, 48, 32),   # a chunk at start_pos, cache pre-filled
])
def test_prefill(hip, B, H, KVH, S, start):
  from xotorch_amd.ops import _hip_ops, torch_ref
  q, k, v, kp, vp = _prefill_inputs(B, H, KVH, S, start)
  out = _hip_ops.attn_prefill_mfma(q, kp, vp, start)
  ref = torch_ref.attn_prefill(q, k, v, start, S)
  ok, err = _close(out, ref, 3e-2)
  assert ok, err


def test_prefill_strided_q(hip):
  from xotorch_amd.ops import _hip_ops, torch_ref
  B, S, H, KVH = 2, 80, 4, 2
  _, k, v, kp, vp = _prefill_inputs(B, H, KVH, S, 0)
  qkv = rnd(B, S, (H + 2 * KVH) * HD, seed=94)
  q = qkv[:, :, : H * HD].view(B, S, H, HD)
  assert not q.is_contiguous()
  out = _hip_ops.attn_prefill_mfma(q, kp, vp, 0)
  ref = torch_ref.attn_prefill(q.contiguous(), k, v, 0, S)
  ok, err = _close(out, ref, 3e-2)
  assert ok, err


@pytest.mark.parametrize("softcap,window,start", [(50.0, 0, 0), (0.0, 48, 0), (30.0, 48, 32)])
def test_prefill_softcap_window(hip, softcap, window, start):
  from xotorch_amd.ops import _hip_ops, torch_ref
  B, H, KVH, S = 2, 4, 2, 96
  scale = 1.0 / 16.0
  q, k, v, kp, vp = _prefill_inputs(B, H, KVH, S, start)
  out = _hip_ops.attn_prefill_mfma(q, kp, vp, start, scale, softcap, window)
  ref = torch_ref.attn_prefill(q, k, v, start, S, scale, softcap, window)
  ok, err = _close(out, ref, 3e-2)
  assert ok, err


def test_prefill_window_tile_skip(hip):
  """start_pos 96, window 48: the first kv tile lies wholly below every q
  row's window and is skipped (tp0 = 1); skipping changes nothing against the
  reference. S = 40 is no multiple of the 16-row sub-tile."""
  from xotorch_amd.ops import _hip_ops, torch_ref
  B, H, KVH, S, start, window = 1, 4, 2, 40, 96, 48
  scale = 1.0 / 16.0
  q, k, v, kp, vp = _prefill_inputs(B, H, KVH, S, start, t32=160)
  out = _hip_ops.attn_prefill_mfma(q, kp, vp, start, scale, 0.0, window)
  ref = torch_ref.attn_prefill(q, k, v, start, S, scale, 0.0, window)
  ok, err = _close(out, ref, 3e-2)
  assert ok, err


# ---------------- 7. cache ----------------

def test_cache_shapes(hip, monkeypatch):
  from xotorch_amd.engine.kvcache import ShardKVCache
  L, B, KVH, cap = 2, 3, 2, 50
  t32 = 64
  monkeypatch.delenv("XOT_FP8_KV", raising=False)
  kv = ShardKVCache(L, B, KVH, cap, HD, torch.bfloat16, "cuda")[0]
  assert kv.kp is not None and kv.vp is not None
  assert tuple(kv.kp.shape) == (B, KVH, t32 // 16, HD // 32, 64, 8) and kv.kp.dtype == torch.bfloat16
  assert tuple(kv.vp.shape) == (B, KVH, HD // 16, t32 // 32, 64, 8) and kv.vp.dtype == torch.bfloat16
  assert kv.ksc is None and kv.vsc is None
  monkeypatch.setenv("XOT_FP8_KV", "1")
  kv8 = ShardKVCache(L, B, KVH, cap, HD, torch.bfloat16, "cuda")[1]
  assert kv8.kp.dtype == torch.uint8 and kv8.vp.dtype == torch.uint8
  assert tuple(kv8.kp.shape) == tuple(kv.kp.shape) and tuple(kv8.vp.shape) == tuple(kv.vp.shape)
  assert tuple(kv8.ksc.shape) == (B, KVH, t32) and tuple(kv8.vsc.shape) == (B, KVH, t32)
  assert kv8.k.dtype == torch.bfloat16 and tuple(kv8.k.shape) == (B, KVH, cap, HD)
  r = kv8.rows(1, 3)
  assert all(t is not None and t.shape[0] == 2 for t in r)
  assert all(t.data_ptr() == full[1:].data_ptr() for t, full in zip(r, kv8))


# ---------------- 8 / 9. tiny gemma2 model ----------------

def _tiny_gemma2():
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.gemma2 import Gemma2Model
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  raw = dict(model_type="gemma2", vocab_size=256, hidden_size=256, intermediate_size=512,
             num_hidden_layers=4, num_attention_heads=4, num_key_value_heads=2, head_dim=HD,
             sliding_window=32, attn_logit_softcapping=50.0, final_logit_softcapping=30.0,
             query_pre_attn_scalar=256, rms_norm_eps=1e-6, rope_theta=10000.0,
             max_position_embeddings=128, tie_word_embeddings=True)
  cfg = config_from_hf(raw, "gemma2-tiny256")
  shard = Shard("gemma2-tiny256", 0, 3, 4)
  torch.manual_seed(5)
  m = Gemma2Model(cfg, shard).to("cuda").to(torch.bfloat16)
  random_init(m)
  m.reset_rope()
  m.eval()
  return cfg, shard, m


@pytest.fixture(scope="module")
def tiny_model(hip):
  """The tiny hd=256 gemma2 on the GPU and a 48-token prompt."""
  cfg, shard, m = _tiny_gemma2()
  B, S = 2, 48
  g = torch.Generator(device="cuda").manual_seed(7)
  toks = torch.randint(0, 256, (B, S), device="cuda", generator=g)
  return dict(cfg=cfg, shard=shard, m=m, toks=toks, B=B, S=S)


def _prefilled(t):
  """A fresh cache for the tiny model after its prompt's prefill -> (cache, logits)."""
  from xotorch_amd.engine.kvcache import ShardKVCache
  cache = ShardKVCache(4, t["B"], 2, t["S"] + 8, HD, torch.bfloat16, "cuda")
  with torch.inference_mode():
    pos = torch.arange(t["S"], dtype=torch.int32, device="cuda")
    logits = t["m"](t["toks"], caches=cache.caches, positions=pos, start_pos=0)
  return cache, logits


def test_model_matches_cpu_fp32(hip, tiny_model):
  from xotorch_amd.engine.kvcache import ShardKVCache
  from xotorch_amd.models.gemma2 import Gemma2Model
  t = tiny_model
  m, B, S = t["m"], t["B"], t["S"]
  cache, lg = _prefilled(t)
  # the HIP path was taken: packed copies exist and prefill wrote them
  for kv in cache.caches:
    assert kv.kp is not None and kv.vp is not None
    t32 = kv.kp.shape[2] * 16
    assert (_unpack_k(kv.kp, t32)[:, :, :S] != 0).any(dim=-1).all()
    assert (_unpack_v(kv.vp, t32)[:, :, :S] != 0).any(dim=-1).all()
    assert torch.equal(kv.kp, _pack_k(kv.k, t32)) and torch.equal(kv.vp, _pack_v(kv.v, t32))
  mc = Gemma2Model(t["cfg"], t["shard"]).float()
  mc.load_state_dict({k: v.float().cpu() for k, v in m.state_dict().items()}, strict=False)
  mc.reset_rope()
  mc.eval()
  cache_ref = ShardKVCache(4, B, 2, S + 8, HD, torch.float32, "cpu")
  with torch.inference_mode():
    lr = mc(t["toks"].cpu(), caches=cache_ref.caches, positions=torch.arange(S), start_pos=0)
    err = (lg.float().cpu() - lr.float()).abs().max().item()
    agree = (lg.float().cpu().argmax(-1) == lr.argmax(-1)).float().mean().item()
    print(f"prefill: max abs err {err:.4g}, argmax agreement {agree:.3f}")
    assert agree > 0.9
    assert torch.allclose(lg.float().cpu(), lr.float(), atol=0.6, rtol=0.1), err
    nxt = lg.argmax(-1, keepdim=True)
    sl = torch.full((B,), S + 1, dtype=torch.int32, device="cuda")
    lg2 = m(nxt, caches=cache.caches, positions=torch.tensor([S], dtype=torch.int32, device="cuda"),
            start_pos=S, is_decode=True, seq_lens=sl)
    lr2 = mc(nxt.cpu(), caches=cache_ref.caches, positions=torch.tensor([S]), start_pos=S, is_decode=True)
    err2 = (lg2.float().cpu() - lr2.float()).abs().max().item()
    print(f"decode: max abs err {err2:.4g}")
    assert torch.allclose(lg2.float().cpu(), lr2.float(), atol=0.6, rtol=0.1), err2
    assert (lg2.float().cpu().argmax(-1) == lr2.argmax(-1)).all()


def test_model_decode_step_graph_replay(hip, tiny_model):
  """The serve contract's decode step (start_pos = -1, per-row positions and
  lengths in device tensors) is captured once and replayed on fresh token,
  position and length contents: same bits as the eager step on those inputs."""
  t = tiny_model
  m, B, S = t["m"], t["B"], t["S"]
  cache, _ = _prefilled(t)
  tok = torch.zeros(B, 1, dtype=torch.int64, device="cuda")
  pos = torch.zeros(B, dtype=torch.int32, device="cuda")
  sl = torch.zeros(B, dtype=torch.int32, device="cuda")

  def step():
    return m(tok, caches=cache.caches, positions=pos, start_pos=-1, is_decode=True, seq_lens=sl)

  def fill(tokens, positions):
    tok.copy_(torch.tensor(tokens, device="cuda").view(B, 1))
    pos.copy_(torch.tensor(positions, dtype=torch.int32, device="cuda"))
    sl.copy_(pos + 1)

  with torch.inference_mode():
    fill([3, 200], [S, S])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
      step()  # eager warm-up outside capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
      captured = step()
    # fresh contents, rows at different positions
    fill([17, 91], [S + 1, S - 8])
    g.replay()
    got = captured.clone()
    want = step()
    torch.cuda.synchronize()
  assert torch.isfinite(got.float()).all()
  assert torch.equal(got, want)
