"""Decode GEMM routing of XotLinear and MLP against the direct binding (or
library) calls each route stands for, bit for bit. Routes are forced by
seeding the auto-pick dict, never by timing."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS = 1e-5
K, N = 512, 256      # XotLinear(512 -> 256): the smallest packable shapes
D, I = 256, 512      # MLP: gate_up 256 -> 1024, down 512 -> 256


def bt(*shape, scale=1.0, seed=0):
  g = torch.Generator(device="cuda").manual_seed(seed)
  return (torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32) * scale).to(torch.bfloat16)


@pytest.fixture(scope="module")
def hipmod():
  from xotorch_amd import ops
  assert ops.hip_available(), f"HIP ext must be built: {ops._hip_load_error}"
  from xotorch_amd.ops import _hip_ops
  return _hip_ops


@pytest.fixture
def picks():
  """The auto-pick dict, empty for the test and restored after it."""
  from xotorch_amd.models.linear import DECODE_PICKS
  saved = dict(DECODE_PICKS)
  DECODE_PICKS.clear()
  yield DECODE_PICKS
  DECODE_PICKS.clear()
  DECODE_PICKS.update(saved)


def _linear(bias):
  from xotorch_amd.models.llama import XotLinear
  torch.manual_seed(5)
  m = XotLinear(K, N, bias=bias).to("cuda", torch.bfloat16)
  m.pack_decode()
  assert m.weight_packed is not None
  return m


def _route_gemm(hipmod, route, x, m):
  if route == "packed":
    return hipmod.skinny_gemm_packed(x, m.weight_packed, N, m.bias)
  if route == "xreg":
    return hipmod.skinny_gemm_packed_xreg(x, m.weight_packed, N, m.bias)
  return F.linear(x, m.weight, m.bias)


def _epilogue_args(M, norm, seed):
  return bt(M, 1, N, seed=seed), (bt(N, seed=seed + 1) if norm else None)


def _check_pair(got, want):
  assert isinstance(got, tuple) and len(got) == 2
  assert torch.equal(got[0], want[0]), (got[0].float() - want[0].float()).abs().max().item()
  if want[1] is None:
    assert got[1] is None
  else:
    assert torch.equal(got[1], want[1]), (got[1].float() - want[1].float()).abs().max().item()


# ---------------- XotLinear: one seeded route per call ----------------

@pytest.mark.parametrize("M", [32, 64])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("route", ["blaslt", "packed", "xreg"])
def test_linear_route_equals_direct_call(hipmod, picks, route, bias, M):
  m = _linear(bias)
  x = bt(M, 1, K, scale=0.5, seed=M)
  picks[(N, K, M)] = route
  with torch.inference_mode():
    got = m(x)
    want = _route_gemm(hipmod, route, x, m)
  assert got.shape == (M, 1, N)
  assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
  assert picks == {(N, K, M): route}


@pytest.mark.parametrize("M", [32, 64])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("route", ["blaslt", "packed", "xreg"])
def test_linear_route_with_epilogue(hipmod, picks, route, bias, norm, M):
  from xotorch_amd import ops
  m = _linear(bias)
  x = bt(M, 1, K, scale=0.5, seed=M + 1)
  res, w = _epilogue_args(M, norm, seed=M + 2)
  picks[(N, K, M)] = route
  with torch.inference_mode():
    got = m(x, (res, w, EPS))
    if route == "packed":  # the epilogue runs inside the kernel's split-K combine
      out = hipmod.skinny_gemm_packed_epilogue(x, m.weight_packed, N, m.bias, res, w, EPS, 0.0)
      want = (out[0], out[1] if norm else None)
    else:
      y = _route_gemm(hipmod, route, x, m)
      want = ops.add_rmsnorm(y, res.view(y.shape), w, EPS)
  _check_pair(got, want)


def _noncontiguous(M):
  return bt(M, 1, 2 * K, scale=0.5, seed=9)[..., :K]


@pytest.mark.parametrize("make_x", [
  lambda: bt(31, 1, K, scale=0.5, seed=31),     # below the 32-row tile
  lambda: bt(48, 1, K, scale=0.5, seed=48),     # no multiple of 32
  lambda: bt(288, 1, K, scale=0.5, seed=288),   # above the decode range
  lambda: _noncontiguous(32),
], ids=["M31", "M48", "M288", "noncontiguous"])
def test_linear_falls_through_to_library(picks, make_x):
  m = _linear(True)
  x = make_x()
  with torch.inference_mode():
    got = m(x)
    want = F.linear(x, m.weight, m.bias)
  assert torch.equal(got, want)
  assert picks == {}  # no decode route was even considered


def test_linear_under_grad_falls_through_to_library(picks):
  m = _linear(True)
  x = bt(32, 1, K, scale=0.5, seed=3).requires_grad_()
  with torch.enable_grad():
    got = m(x)
    want = F.linear(x, m.weight, m.bias)
  assert got.requires_grad
  assert torch.equal(got, want)
  assert picks == {}


def test_linear_fp8_route_equals_direct_call(hipmod, picks, monkeypatch):
  from xotorch_amd.models.llama import XotLinear
  monkeypatch.setenv("XOT_FP8_GEMM", "1")
  M = 32
  torch.manual_seed(6)
  m = XotLinear(K, N, bias=True).to("cuda", torch.bfloat16)
  m.pack_decode()
  assert m.weight_packed_fp8 is not None and m.weight_packed is None
  x = bt(M, 1, K, scale=0.5, seed=4)
  with torch.inference_mode():
    got = m(x)
    x8, sx = hipmod.quant_fp8_rows(x.view(M, K))
    want = hipmod.skinny_gemm_fp8(x8, sx, m.weight_packed_fp8, m.weight_scale, 1, N, m.bias)
  assert got.shape == (M, 1, N)
  assert torch.equal(got, want.view(M, 1, N))
  assert picks == {}


def test_linear_under_capture_takes_packed_and_caches_nothing(hipmod, picks):
  m = _linear(True)
  M = 96  # a key no other test seeds
  x = bt(M, 1, K, scale=0.5, seed=5)
  with torch.inference_mode():
    want = hipmod.skinny_gemm_packed(x, m.weight_packed, N, m.bias)  # also loads the kernel
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
      got = m(x)
    g.replay()
    torch.cuda.synchronize()
  assert torch.equal(got, want)
  assert picks == {}


# ---------------- MLP: fused SwiGLU + down projection vs split ----------------

@pytest.fixture(scope="module")
def mlp():
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import MLP
  from xotorch_amd.models.registry import builtin_config
  cfg = config_from_hf(dict(builtin_config("dummy"), hidden_size=D, intermediate_size=I), "dummy")
  torch.manual_seed(8)
  m = MLP(cfg).to("cuda", torch.bfloat16)
  m.gate_up_proj.pack_decode()
  m.down_proj.pack_decode()
  assert m.gate_up_proj.weight_packed is not None and m.down_proj.weight_packed is not None
  return m


def _mlp_chain(hipmod, mlp, x, route, epilogue):
  """The launches the seeded routes stand for, called on the bindings."""
  M = x.shape[0]
  wp = mlp.down_proj.weight_packed
  gu = hipmod.skinny_gemm_packed(x, mlp.gate_up_proj.weight_packed, 2 * I, None)
  if route == "fused":
    if epilogue is None:
      return hipmod.skinny_gemm_packed_swiglu(gu, wp, D, None).view(M, 1, D)
    res, w, eps = epilogue
    out = hipmod.skinny_gemm_packed_swiglu_epilogue(gu, wp, D, None, res, w, eps, 0.0)
  else:
    h = hipmod.swiglu_packed(gu)
    if epilogue is None:
      return hipmod.skinny_gemm_packed(h, wp, D, None)
    res, w, eps = epilogue
    out = hipmod.skinny_gemm_packed_epilogue(h, wp, D, None, res, w, eps, 0.0)
  return out[0], (out[1] if w is not None else None)


def _seed_mlp(picks, M, route):
  picks[(2 * I, D, M)] = "packed"           # gate_up projection
  picks[(D, I, M)] = "packed"               # down projection (split route)
  picks[("fuse_swiglu", D, I, M)] = route


@pytest.mark.parametrize("epi", ["none", "norm", "add_only"])
@pytest.mark.parametrize("route", ["fused", "split"])
def test_mlp_route_equals_direct_chain(hipmod, picks, mlp, route, epi):
  M = 32
  x = bt(M, 1, D, scale=0.5, seed=12)
  epilogue = None
  if epi != "none":
    res = bt(M, 1, D, seed=13)
    epilogue = (res, bt(D, seed=14) if epi == "norm" else None, EPS)
  _seed_mlp(picks, M, route)
  seeded = dict(picks)
  with torch.inference_mode():
    got = mlp(x, epilogue)
    want = _mlp_chain(hipmod, mlp, x, route, epilogue)
  if epilogue is None:
    assert got.shape == (M, 1, D)
    assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()
  else:
    _check_pair(got, want)
  assert picks == seeded


@pytest.mark.parametrize("epi", [False, True])
def test_mlp_fuse_switch_off_takes_split(hipmod, picks, mlp, monkeypatch, epi):
  M = 32
  x = bt(M, 1, D, scale=0.5, seed=15)
  epilogue = (bt(M, 1, D, seed=16), bt(D, seed=17), EPS) if epi else None
  _seed_mlp(picks, M, "fused")
  monkeypatch.setenv("XOT_FUSE_SWIGLU", "0")
  with torch.inference_mode():
    got = mlp(x, epilogue)
    want = _mlp_chain(hipmod, mlp, x, "split", epilogue)
  if epi:
    _check_pair(got, want)
  else:
    assert torch.equal(got, want)
