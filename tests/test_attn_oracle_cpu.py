"""The decode-attention oracle checked on the CPU, for every case the GPU file
runs: the inputs are sharp enough that a wrong kernel lands far outside the
error bound, and the bound is wide enough for the error a correct fp8 kernel
must make (and no wider than what the whole-tile s_pv defect makes)."""
import pytest
import torch

import attn_oracle as ao

ALL = ao.SPECS + ao.ZERO_SPECS


@pytest.fixture(scope="module")
def built():
  """case and its unmutated reference, built once per spec"""
  cache = {}
  def get(sp):
    if sp.name not in cache:
      c = ao.build_case(sp)
      cache[sp.name] = (c, ao.reference(c))
    return cache[sp.name]
  return get


def test_packers_roundtrip_and_layout():
  """pack/unpack are inverses, and the packed images put (d, pos) where the
  layout comment says, checked element by element on a small tensor."""
  t32, hd = 64, 64
  x = torch.arange(2 * 1 * t32 * hd, dtype=torch.float32).view(2, 1, t32, hd)
  kp, vp = ao.pack_k(x, t32), ao.pack_v(x, t32)
  assert torch.equal(ao.unpack_k(kp, t32), x) and torch.equal(ao.unpack_v(vp, t32), x)
  for pos in (0, 5, 17, 40, 63):
    for d in (0, 7, 8, 31, 33, 63):
      assert kp[1, 0, pos >> 4, d >> 5, ((d & 31) >> 3) * 16 + (pos & 15), d & 7] == x[1, 0, pos, d]
      assert vp[1, 0, d >> 4, pos >> 5, ((pos & 31) >> 3) * 16 + (d & 15), pos & 7] == x[1, 0, pos, d]
  lat, rot = torch.randn(2, 40, 512), torch.randn(2, 40, 64)
  kp, vp = ao.mla_pack(lat, rot, t32)
  assert kp.shape == (2, t32 // 16, 18, 64, 8) and vp.shape == (2, 32, t32 // 32, 64, 8)
  full = torch.cat([lat, rot], -1)
  for pos in (0, 17, 39):
    for d in (0, 100, 511, 512, 575):
      assert kp[0, pos >> 4, d >> 5, ((d & 31) >> 3) * 16 + (pos & 15), d & 7] == full[0, pos, d]
      if d < 512:
        assert vp[0, d >> 4, pos >> 5, ((pos & 31) >> 3) * 16 + (d & 15), pos & 7] == full[0, pos, d]
  assert (kp[:, 40 >> 4:, :, :, :][:, 1:] == 0).all()  # positions 48.. were never written


def test_split_geometry_covers_both_epilogues():
  """The cases reach the in-workgroup merge (nsplit <= 4), the workspace
  merge, and splits that lie wholly past the longest row."""
  geo = {sp.name: ao.split_geometry(sp.kernel, len(sp.lens) * len(sp.families), sp.H, sp.KVH, sp.T)
         for sp in ao.SPECS}
  assert geo["mfma128-bf16-T128"] == (4, 32)
  assert geo["mfma128-bf16-T256"] == (8, 32)
  assert geo["mfma256-fp8-T1024"] == (32, 32)
  assert geo["mla-fp8-H20-T1024"] == (64, 32)   # splits 32..63 are empty
  assert geo["valu64-bf16-T128"] == (1, 128)
  # two tiles per split: the tile-to-tile carry, into either merge
  assert geo["mfma128-fp8-T128-B128"] == (2, 64)
  assert geo["mfma256-fp8-T2048"] == (32, 64)
  assert geo["mla-fp8-H16-T4096"] == (64, 64)


@pytest.mark.parametrize("sp", ALL, ids=lambda s: s.name)
def test_reference_is_consistent(built, sp):
  """Weights sum to one on live rows, zero-length rows give exact zeros, and
  the scores family reads back its score gap as the ratio of its two blocks."""
  c, ref = built(sp)
  live = c.seq_lens > 0
  assert torch.allclose(ref.w.sum(-1)[live], torch.ones_like(ref.L[live]), atol=1e-12)
  assert (ref.out[~live] == 0).all() and (ref.absw[~live] == 0).all()
  assert torch.isfinite(ref.out).all() and torch.isfinite(ao.bound(c, ref)).all()
  if "scores" in sp.families:
    rows = (c.rows("scores") | c.rows("capped")) & (c.seq_lens - c.lo >= 2)
    p1 = c.seq_lens - 1
    p2 = c.lo + (c.seq_lens - 1 - c.lo) // 2
    b = torch.arange(len(c.fam))
    gap = (ref.s[b, :, p1] - ref.s[b, :, p2])[rows]
    if not sp.softcap:
      # ln 9 up to the bf16 / e4m3 rounding of the marker rows
      assert (gap - ao.GAP).abs().max() < (0.6 if sp.fp8 else 0.1), gap
    wr = (ref.w[b, :, p1] / ref.w[b, :, p2])[rows]
    assert torch.allclose(wr, torch.exp(gap), rtol=1e-9)


@pytest.mark.parametrize("sp", ALL, ids=lambda s: s.name)
def test_mutations_land_clear_of_the_bound(built, sp):
  """Every applicable mutation of the reference moves at least one element of
  every (row, head) it applies to by >= 4 x bound: a kernel that is wrong in
  that way cannot pass the GPU test, which holds a correct one to 1 x."""
  c, ref = built(sp)
  bnd = ao.bound(c, ref)
  for name, kw, rows in ao.mutations(c):
    if not rows.any():
      continue
    mut = ao.reference(c, **kw)
    moved = ((mut.out - ref.out).abs() / bnd.clamp_min(1e-300)).amax(-1)   # [B, H]
    worst = moved[rows].min().item()
    print(f"{sp.name}: {name}: {int(rows.sum())} rows, weakest (row, head) moves {worst:.1f} x bound")
    assert worst >= 4.0, (name, worst, c.seq_lens[rows][moved[rows].amin(-1) < 4.0].tolist())
  families = set(sp.families)
  assert {n for n, _, r in ao.mutations(c) if r.any()} >= (
    {"sl+1", "sl-1"} if families == {"edges"} else {"sl+1", "sl-1", "half-tile (last)", "split", "scale*sqrt2"})


@pytest.mark.parametrize("sp", [s for s in ALL if s.fp8], ids=lambda s: s.name)
def test_fp8_emulator_against_the_bound(built, sp):
  """The tile loop with e4m3 P stays inside the bound when s_pv is taken over
  the visible positions, and leaves it on a fresh cache (scales 1.0 past the
  length) when s_pv is taken over the whole tile, seq_len % 32 != 0 and the
  last tile carries a fair share of the weight."""
  c, ref = built(sp)
  vis_r = ao.ratio(c, ref, ao.emulate_fp8(c, ref, whole_tile=False)).amax((1, 2))
  whole_r = ao.ratio(c, ref, ao.emulate_fp8(c, ref, whole_tile=True)).amax((1, 2))
  print(f"{sp.name}: visible-only s_pv worst {vis_r.max():.3f}; whole-tile worst {whole_r.max():.3f}")
  assert vis_r.max() <= 1.0, (vis_r.max().item(), c.seq_lens[vis_r > 1.0].tolist())
  # Shown by the plain rows: their last tile holds V of ordinary size (scales
  # about 0.004 against the 1.0 past the length), which leaves its P' one or
  # two significant bits, a relative error of 1/4 to 1; the marker blocks of
  # the other families carry scales large enough to keep P' normal. The plain
  # rows' weights are spread widely (scores of std 1), so a tile's share of the
  # weight is about its share of the positions: once the last tile holds an
  # eighth of them, about 1/8 of the weight errs by 1/4 or more, against the
  # bound's 1/16 of everything. That is an estimate for these seeded rows, not
  # a theorem; a tail with a smaller share (seq_len 100 or 1000) stays inside.
  tail = c.seq_lens - torch.maximum(c.lo, c.seq_lens // 32 * 32)
  partial = c.rows("plain") & (c.seq_lens % 32 != 0) & (tail * 8 >= c.seq_lens - c.lo)
  full = c.seq_lens % 32 == 0
  assert (whole_r[partial] > 1.0).all(), (c.seq_lens[partial][whole_r[partial] <= 1.0].tolist())
  assert torch.equal(whole_r[full], vis_r[full])


@pytest.mark.parametrize("sp", [s for s in ALL if "ramp" in s.families], ids=lambda s: s.name)
def test_tile_carry_lands_clear_of_the_bound(built, sp):
  """The cases with two tiles per split: the exact tile loop equals the
  reference, and one that leaves alpha (or, fp8, rfac) out of the accumulator
  rescale moves every head of every ramp row that holds a whole odd tile after
  the even one of its split by >= 4 x bound."""
  c, ref = built(sp)
  nsplit, chunk = ao.split_geometry(sp.kernel, len(c.fam), sp.H, sp.KVH, sp.T)
  assert chunk >= 64
  rows = (c.rows("ramp") & (c.seq_lens >= 64)).nonzero().flatten().tolist()
  assert rows
  bnd = ao.bound(c, ref)
  exact = ao.emulate_tiles(c, ref, rows=rows)
  assert ((exact - ref.out).abs()[rows] <= 1e-9 * (1 + ref.absw[rows])).all()
  for kw in [dict(drop_alpha=True)] + ([dict(drop_rfac=True)] if sp.fp8 else []):
    wrong = ao.emulate_tiles(c, ref, rows=rows, **kw)
    moved = ((wrong - ref.out).abs() / bnd.clamp_min(1e-300)).amax(-1)[rows]
    print(f"{sp.name}: {kw}: weakest (row, head) moves {moved.min():.1f} x bound")
    assert moved.min() >= 4.0, (kw, moved.min().item())
