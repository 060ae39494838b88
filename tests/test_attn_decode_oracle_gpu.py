"""Decode attention against the fp64 oracle (tests/attn_oracle.py): every
kernel family and cache dtype, one launch per case over a batch of ragged
rows from the edges / tiles / scores / plain input families, held to the
derived bound: max |out - ref| / bound <= 1. tests/test_attn_oracle_cpu.py
shows, for the same cases, that a kernel wrong by one position, one half-tile,
one split, a factor sqrt 2 in the scale, a missing softcap, a missing rope
tail or a neighbour's K scale lands at >= 4."""
import pytest
import torch

import attn_oracle as ao

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_ops():
  from xotorch_amd import ops
  assert ops.hip_available(), f"HIP ext must be built: {ops._hip_load_error}"
  from xotorch_amd.ops import _hip_ops
  return _hip_ops


def launch(hip_ops, c):
  """One launch of the case's kernel through its binding; out as [B, H, Dv]."""
  sp = c.spec
  d = ao.device_inputs(c)
  if sp.kernel == "valu":
    out = hip_ops.attn_decode(d["q"], d["kc"], d["vc"], d["seq_lens"])
  elif sp.kernel == "mfma":
    out = hip_ops.attn_decode_mfma(d["q"], d["kp"], d["vp"], d["seq_lens"], sp.T, 0.0, sp.softcap, sp.window,
                                   k_scale=d.get("k_scale"), v_scale=d.get("v_scale"))
  else:
    out = hip_ops.attn_decode_mla(d["q"], d["kp"], d["vp"], d["seq_lens"], sp.scale,
                                  d.get("q_scale"), d.get("k_scale"))
  torch.cuda.synchronize()
  return out.float().cpu().reshape(len(c.fam), sp.H, sp.dv)


def check(c, out):
  ref = ao.reference(c)
  r = ao.ratio(c, ref, out)
  print(ao.report(c, r))
  assert torch.isfinite(out).all()
  worst = r.amax((1, 2))
  assert worst.max() <= 1.0, [(f, int(s), round(float(x), 2))
                              for f, s, x in zip(c.fam, c.seq_lens, worst) if x > 1.0]


@pytest.mark.parametrize("sp", ao.SPECS, ids=lambda s: s.name)
def test_decode_within_bound(hip_ops, sp):
  c = ao.build_case(sp)
  check(c, launch(hip_ops, c))


@pytest.mark.parametrize("sp", ao.ZERO_SPECS, ids=lambda s: s.name)
def test_zero_length_row(hip_ops, sp):
  """A row with seq_len 0 (the ring resets lengths to zero) returns exact
  zeros, no NaN, and leaves its neighbours within the bound."""
  c = ao.build_case(sp)
  out = launch(hip_ops, c)
  assert c.seq_lens.tolist() == [40, 0, 97]
  assert (out[1] == 0).all(), out[1].abs().max()
  check(c, out)


def test_mfma_binding_checks_head_ratio(hip_ops):
  """A wave scores at most 16 query heads per kv head: the binding refuses
  more, and an H that KVH does not divide, instead of leaving rows unwritten."""
  T, hd = 32, 128
  kp = torch.zeros(1, 1, T // 16, hd // 32, 64, 8, dtype=torch.bfloat16, device="cuda")
  vp = torch.zeros(1, 1, hd // 16, T // 32, 64, 8, dtype=torch.bfloat16, device="cuda")
  sl = torch.ones(1, dtype=torch.int32, device="cuda")
  q = lambda H: torch.zeros(1, 1, H, hd, dtype=torch.bfloat16, device="cuda")
  with pytest.raises(RuntimeError, match="16 query heads per kv head"):
    hip_ops.attn_decode_mfma(q(17), kp, vp, sl, T)
  kp2, vp2 = kp.expand(1, 2, -1, -1, -1, -1).contiguous(), vp.expand(1, 2, -1, -1, -1, -1).contiguous()
  with pytest.raises(RuntimeError, match="multiple of KVH"):
    hip_ops.attn_decode_mfma(q(5), kp2, vp2, sl, T)
  assert hip_ops.attn_decode_mfma(q(16), kp, vp, sl, T).shape == (1, 1, 16, hd)
