"""The packed decode GEMM's 256-row weight tile (XOT_SKINNY_BN=256) against
its 128-row tile (XOT_SKINNY_BN=128): the same bits, since the split-K plan
and each wave's MFMA order do not depend on the tile, and both within the
packed-GEMM tolerance of the fp32 product."""
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


def both_tiles(monkeypatch, fn):
  """fn() under XOT_SKINNY_BN=128 and =256 (the launcher reads it per call)."""
  out = []
  for bn in ("128", "256"):
    monkeypatch.setenv("XOT_SKINNY_BN", bn)
    out.append(fn())
  monkeypatch.delenv("XOT_SKINNY_BN")
  return out


def operands(M, N, K, bias):
  x = bt(M, K, scale=0.5, seed=M + N + 1)
  w = bt(N, K, scale=0.02, seed=K + 1)
  b = bt(N, seed=7) if bias else None
  ref = x.float() @ w.float().T
  if bias:
    ref = ref + b.float()
  return x, w, b, ref


def close(y, ref):
  return torch.allclose(y.float(), ref, atol=5e-2, rtol=5e-2)


SHAPES = {
  "a": (128, 256, 2048),        # one wide tile, nsplit 2
  "b": (128, 512, 1024),        # unsplit, two wide tiles
  "c": (256, 512, 4096),        # MT=8, nsplit 4
  "d": (128, 768, 4096 + 64),   # nsplit 4, kc 1088: BK=64 staging, 17 steps and a 14-step last split
  "f": (128, 4096, 1024),       # unsplit, bf16 direct store
  # shapes beyond the issue's table: the paths the bench runs and the staging corner cases
  "bk128": (128, 256, 34816),   # nsplit 16, kc 2176: BK=128 staging, 17 steps (odd: ends on image 0)
  "mt5": (160, 256, 2048),      # odd MT at BK=64: the last staging piece covers half the threads
  "mt6_bk128": (192, 256, 32768),  # MT=6 at BK=128
  "mt8_bk128": (256, 256, 32768),  # plan says BK=128; the wide tile stages BK=64 at MT >= 7
}


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("case", list(SHAPES))
def test_wide_tile_same_bits(hip, monkeypatch, case, bias):
  M, N, K = SHAPES[case]
  x, w, b, ref = operands(M, N, K, bias)
  wp = hip.pack_decode_weight(w)
  y128, y256 = both_tiles(monkeypatch, lambda: hip.skinny_gemm_packed(x, wp, N, b))
  assert torch.equal(y128, y256), (y128.float() - y256.float()).abs().max()
  assert close(y256, ref), (y256.float() - ref).abs().max()
  assert torch.equal(hip.skinny_gemm_packed(x, wp, N, b), y128)  # knob unset: whichever tile, the same bits


def test_n_not_multiple_of_256_stays_on_narrow_tile(hip, monkeypatch):
  """case e: N=384 is not eligible, the knob changes nothing."""
  M, N, K = 128, 384, 2048
  x, w, _, ref = operands(M, N, K, False)
  wp = hip.pack_decode_weight(w)
  y128, y256 = both_tiles(monkeypatch, lambda: hip.skinny_gemm_packed(x, wp, N, None))
  assert torch.equal(y128, y256)
  assert close(y256, ref), (y256.float() - ref).abs().max()


def test_m64_untouched(hip, monkeypatch):
  M, N, K = 64, 512, 4096
  x, w, _, ref = operands(M, N, K, False)
  wp = hip.pack_decode_weight(w)
  y128, y256 = both_tiles(monkeypatch, lambda: hip.skinny_gemm_packed(x, wp, N, None))
  assert torch.equal(y128, y256)
  assert close(y256, ref), (y256.float() - ref).abs().max()


def test_knob_is_read_per_call(hip, monkeypatch):
  """A value other than 128 / 256 is refused, on an eligible shape, at the call."""
  x, w, _, _ = operands(128, 256, 1024, False)
  wp = hip.pack_decode_weight(w)
  monkeypatch.setenv("XOT_SKINNY_BN", "64")
  with pytest.raises(RuntimeError):
    hip.skinny_gemm_packed(x, wp, 256, None)
  monkeypatch.delenv("XOT_SKINNY_BN")
  hip.skinny_gemm_packed(x, wp, 256, None)


@pytest.mark.parametrize("norm", [False, True])
def test_epilogue_entry(hip, monkeypatch, norm):
  M, N, K = 128, 512, 4096
  x, w, _, ref = operands(M, N, K, False)
  wp = hip.pack_decode_weight(w)
  res = bt(M, N, scale=0.5, seed=3)
  nw = (1.0 + bt(N, scale=0.1, seed=4).float()).to(torch.bfloat16) if norm else None
  (h128, n128), (h256, n256) = both_tiles(
    monkeypatch, lambda: hip.skinny_gemm_packed_epilogue(x, wp, N, None, (res, nw, 1e-5)))
  assert torch.equal(h128, h256)
  assert close(h256, ref + res.float()), (h256.float() - ref - res.float()).abs().max()
  if norm:
    assert torch.equal(n128, n256)
    hf = h256.float()
    nref = hf * torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + 1e-5) * nw.float()
    assert close(n256, nref), (n256.float() - nref).abs().max()
  else:
    assert n128 is None and n256 is None


def test_swiglu_staging_entry(hip, monkeypatch):
  M, I, N = 128, 2048, 256
  gu = bt(M, 2 * I, scale=1.0, seed=5)
  w = bt(N, I, scale=0.02, seed=6)
  wp = hip.pack_decode_weight(w)
  y128, y256 = both_tiles(monkeypatch, lambda: hip.skinny_gemm_packed_swiglu(gu, wp, N, None))
  assert torch.equal(y128, y256)
  g, u = gu[:, :I].float(), gu[:, I:].float()
  act = (torch.nn.functional.silu(g) * u).to(torch.bfloat16)
  ref = act.float() @ w.float().T
  assert close(y256, ref), (y256.float() - ref).abs().max()


def test_grouped_entry(hip, monkeypatch):
  E, C, K, N = 2, 128, 2048, 256
  x = bt(E, C, K, scale=0.5, seed=11)
  ws = [bt(N, K, scale=0.05, seed=100 + e) for e in range(E)]
  wp = torch.stack([hip.pack_decode_weight(w) for w in ws]).contiguous()
  y128, y256 = both_tiles(monkeypatch, lambda: hip.skinny_gemm_grouped(x, wp, E, N))
  assert torch.equal(y128, y256)
  for e in range(E):
    ref = x[e].float() @ ws[e].float().T
    assert close(y256[e], ref), (e, (y256[e].float() - ref).abs().max())
