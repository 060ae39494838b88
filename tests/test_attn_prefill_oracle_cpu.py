"""The prefill-attention oracle checked on the CPU, for every case the GPU file
runs: the inputs are sharp enough that a kernel wrong by one position, one
half-tile, one tile, the scale, the softcap or the kv head lands far outside
the error bound at every row it concerns, and the bound is wide enough for the
error a correct kernel makes (a torch fp32 emulation of the kernel's loop)."""
import pytest
import torch

import attn_oracle as ao


@pytest.mark.parametrize("sp", ao.PREFILL_SPECS, ids=lambda s: s.name)
def test_reference_is_consistent(sp):
  """Finite everywhere although the cache is poisoned past T, row 0 at start 0
  returns V[0], and the limits family gives the row's last position and (under a
  window) its first one a share of the softmax that does not fall with length."""
  c = ao.prefill_case(sp)
  assert torch.isfinite(c.ref).all() and torch.isfinite(c.bound).all() and (c.bound > 0).all()
  assert c.kc.shape == (4 * sp.B + sp.extra_batch, sp.KVH, sp.cap, sp.hd) and sp.cap % 32 == 0 and sp.T <= sp.cap
  assert (c.kc[:, :, sp.T:].abs() > 1e29).all() and (c.vc[4 * sp.B:].abs() > 1e29).all()
  if sp.start == 0:
    v0 = c.v[:, :, 0].repeat_interleave(sp.H // sp.KVH, dim=1)
    assert torch.equal(c.ref[:, 0], v0)


@pytest.mark.parametrize("sp", ao.PREFILL_SPECS, ids=lambda s: s.name)
def test_mutations_land_clear_of_the_bound(sp):
  """Every applicable mutation of the reference moves at least one element of
  every (row, head) it applies to by >= 4 x bound: a kernel that is wrong in
  that way cannot pass the GPU test, which holds a correct one to 1 x."""
  c = ao.prefill_case(sp)
  seen, weakest = set(), {}
  for name, fam, kw, rows in ao.prefill_mutations(c):
    if not rows.any():
      continue
    b = c.rows(fam)
    moved = ((c.reference(fam, **kw) - c.ref[b]).abs() / c.bound[b]).amax(-1)[:, rows]   # [B, rows, H]
    worst = moved.min().item()
    kind = name.split(" ")[0] if name.startswith("half-tile") else name
    seen.add(kind)
    weakest[(kind, fam)] = min(worst, weakest.get((kind, fam), float("inf")))
    assert worst >= 4.0, (name, fam, worst, (sp.start + rows.nonzero().flatten()[(moved < 4.0).any(0).any(-1)]).tolist())
  for (kind, fam), x in weakest.items():
    print(f"{sp.name}: {kind} ({fam}): weakest (row, head) moves {x:.1f} x bound")
  want = {"limit-1", "first tile", "scale*sqrt2"}
  want |= {"limit+1"} if sp.S > 1 else set()
  want |= {"half-tile"} if sp.T >= 16 else set()
  want |= {"window start+1", "window start-1"} if sp.window else set()
  want |= {"no softcap"} if sp.softcap else set()
  want |= {"neighbouring kv head"} if sp.KVH > 1 else set()
  assert seen >= want, want - seen


@pytest.mark.parametrize("sp", ao.PREFILL_SPECS, ids=lambda s: s.name)
def test_emulated_kernel_stays_inside_the_bound(sp):
  """The kernel's loop in fp32 (32-position tiles, online softmax with alpha
  and the -inf guard, P rounded once to bf16, fp32 PV accumulation, the final
  divide and bf16 rounding) stays <= 1 x bound on every family: a correct
  kernel can pass the GPU test on these inputs."""
  c = ao.prefill_case(sp)
  r = (ao.prefill_emulate(c).double() - c.ref).abs() / c.bound
  per_fam = {f: r[c.rows(f)].max().item() for f in ao.PF_FAMILIES}
  print(f"{sp.name}: emulator worst err/bound " + " ".join(f"{f} {x:.3f}" for f, x in per_fam.items()))
  assert max(per_fam.values()) <= 1.0, per_fam
