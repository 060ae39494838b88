"""Decode GEMMs against the integer oracle of tests/gemm_oracle.py: one launch
through the binding per case, compared on the CPU. Exact cases must equal the
CPU reference bit for bit whatever tile, BK, split count or split order the
launcher picks; real cases and the GLU store must stay inside the derived
bound. The variant is forced with the knobs the launcher reads per call, and
the split count is asserted, so a case cannot run another instance unnoticed."""
import pytest
import torch

import gemm_oracle as go

pytestmark = pytest.mark.gpu

KNOBS = ("XOT_SKINNY_TARGET", "XOT_SKINNY_BK64", "XOT_SKINNY_BN")


@pytest.fixture(scope="module")
def hip():
  from xotorch_amd import ops
  assert ops.hip_available(), f"HIP ext must be built: {ops._hip_load_error}"
  return ops


def _set_knobs(hip, monkeypatch, sp):
  for k in KNOBS:
    monkeypatch.delenv(k, raising=False)
  monkeypatch.setenv("XOT_SKINNY_TARGET", str(sp.target))
  if sp.bk64:
    monkeypatch.setenv("XOT_SKINNY_BK64", "1")
  if sp.bn:
    monkeypatch.setenv("XOT_SKINNY_BN", str(sp.bn))
  pl = sp.plan
  if sp.op == "glu" or sp.K % 64:
    # the GLU launcher never splits; the unpacked kernel's K % 64 != 0 cases run
    # at target 0, which no K splits, and the binding plans 64-aligned K only
    assert pl.nsplit == 1 and (sp.op == "glu" or sp.target == 0)
  else:
    # the binding plans for one expert; at target 0 and BIG the expert count does not enter
    assert sp.E == 1 or sp.target in (0, go.BIG)
    assert hip.skinny_plan_nsplit(sp.N, sp.K) == pl.nsplit, sp.name
  return pl


def _launch(hip, c):
  sp = c.spec
  mod = hip._gpu()
  a = [t.cuda() for t in go.launch_args(c)]
  bias = c.bias.to(torch.bfloat16).cuda() if c.bias is not None else None
  N, E = sp.N, sp.E
  if sp.op == "plain":
    return mod.skinny_gemm(a[0], a[1], bias)
  if sp.op == "packed":
    return mod.skinny_gemm_packed(a[0], a[1], N, bias)
  if sp.op == "xreg":
    return mod.skinny_gemm_packed_xreg(a[0], a[1], N, bias)
  if sp.op == "grouped":
    return mod.skinny_gemm_grouped(a[0], a[1], E, N)
  if sp.op == "swiglu":
    return mod.skinny_gemm_packed_swiglu(a[0], a[1], N, bias)
  if sp.op == "glu":
    return mod.skinny_gemm_packed_glu(a[0], a[1], N)
  if sp.op == "fp8":
    return mod.skinny_gemm_fp8(a[0], a[1], a[2], a[3], E, N, bias)
  if sp.op == "mxfp4":
    return mod.skinny_gemm_mxfp4(a[0], a[1], a[2], E, N, bias)
  res = c.res.to(torch.bfloat16).cuda()
  fn = hip.skinny_gemm_packed_epilogue if sp.op == "epilogue" else hip.skinny_gemm_packed_swiglu_epilogue
  h, normed = fn(a[0], a[1], N, bias, (res, None, 1e-6))
  assert normed is None
  return h


@pytest.mark.parametrize("sp", go.SPECS, ids=lambda s: s.name)
def test_gemm_matches_the_oracle(hip, monkeypatch, sp):
  _set_knobs(hip, monkeypatch, sp)
  c = go.build_case(sp)
  got = _launch(hip, c)
  assert got.dtype == torch.bfloat16 and got.numel() == c.ref.numel()
  go.check(c, got)
