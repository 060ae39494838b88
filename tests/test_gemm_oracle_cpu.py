"""The decode-GEMM oracle checked against itself, without a GPU: every case of
the GPU matrix satisfies the builder's conditions, every mutation shows in
every output tile it applies to, and the weight packers put an element that
encodes its own (n, k) where the layout comments say it goes."""
import collections

import pytest
import torch

import gemm_oracle as go
from xotorch_amd import ops

WEAKEST = collections.defaultdict(lambda: 1.0)  # (family, mutation) -> smallest visible share of a tile


@pytest.mark.parametrize("sp", go.SPECS, ids=lambda s: s.name)
def test_case_conditions_and_mutation_margins(sp):
  c = go.build_case(sp)  # asserts |ref| <= 256, ref == bf16(ref), integer sums, <= 512 non-zeros per row
  pl = sp.plan
  assert c.ref.abs().max() > 0
  if sp.family == "exact":
    # one non-zero in every (16-k chunk, 32-row m-tile) cell of x
    cells = (c.x != 0).view(sp.E * sp.M // 32, 32, sp.K // 16, 16).any(dim=3).any(dim=1)
    assert cells.all()
    # the cancelling pairs: equal weight columns in different chunks and, when split, different splits
    k1, k2 = c.extra["pairs"]
    assert torch.equal(c.w[:, :, k1], c.w[:, :, k2]) and ((k1 // 16) != (k2 // 16)).all()
    if pl.nsplit > 1:
      assert ((k1 // pl.kc) != (k2 // pl.kc)).all()
    A = 256.0 if sp.op == "fp8" else 4096.0
    big = c.x.abs() == A
    assert (big.sum(1) >= 2).all() and (big.sum(1) % 2 == 0).all()
    assert torch.equal(go.sums(c, c.x * big), torch.zeros_like(c.S))  # the pairs add zero
  else:
    assert sp.K <= 256 or pl.nsplit > 1
    assert (go.bound(c) > 0).all()
  names = set()
  for name, mut, where in go.mutations(c):
    names.add(name)
    if sp.family == "real" and name in go.REAL_BLIND:
      continue
    frac = go.tile_fraction(c, go.visible(c, mut))
    assert frac.shape == where.shape and where.any()
    assert (frac[where] > 0).all(), (sp.name, name, int((frac[where] == 0).sum()), int(where.sum()))
    key = ("glu" if sp.op == "glu" else sp.family, name.split(" (")[0])
    WEAKEST[key] = min(WEAKEST[key], float(frac[where].min()))
  assert ("split dropped" in names) == (pl.nsplit > 1) and ("bias dropped" in names) == sp.bias


def test_weakest_sensitivity_report():
  """Prints, per family and mutation, the smallest share of an affected output
  tile that the defect moves (docs/KERNELS.md quotes this table). Runs after
  the parametrized test in file order; empty when that test was deselected."""
  for (fam, name), v in sorted(WEAKEST.items()):
    print(f"weakest {fam:5s} {name:28s} {v:.4f}")
    assert v > 0


def test_matrix_reaches_every_instance():
  """The variant matrix names every (MT, NW, BK, SPLIT) the packed launcher can pick."""
  got = {(s.M // 32, s.plan.nw, s.plan.bk, s.plan.nsplit > 1) for s in go.SPECS if s.op == "packed"}
  want = set()
  for mt in range(1, 9):
    for nw in ((4, 8) if mt >= 4 else (4,)):
      for bk in (64, 128):
        if nw == 8 and mt >= 7 and bk == 128:
          continue  # the wide tile stages BK=64 at MT >= 7
        want |= {(mt, nw, bk, False), (mt, nw, bk, True)}
  assert got == want, (sorted(want - got), sorted(got - want))
  steps = {(s.plan.bk, s.plan.nsplit > 1, ((min(s.plan.kc, s.K)) // s.plan.bk) % 2) for s in go.SPECS if s.op == "packed"}
  assert steps == {(bk, sp, odd) for bk in (64, 128) for sp in (False, True) for odd in (0, 1)}
  assert max(s.plan.nsplit for s in go.SPECS) == 16
  assert {s.plan.nsplit for s in go.SPECS if s.op == "glu"} == {1}


def test_plan_restates_the_known_shapes():
  assert go.plan("packed", 128, 8192, 57344) == go.Plan(1, 8192, 128, 8)   # gate_up at 70B: unsplit, wide
  assert go.plan("packed", 32, 28672, 8192).nsplit == 8                    # down: 64 tiles x 8 splits reach 384 blocks
  assert go.plan("packed", 32, 2112, 256, target=go.BIG) == go.Plan(2, 1088, 64, 4)
  assert go.plan("plain", 32, 4416, 256, target=go.BIG) == go.Plan(4, 1104, 64, 4)
  assert go.plan("packed", 224, 2048, 256, target=0, bn=256) == go.Plan(1, 2048, 64, 8)
  assert go.plan("packed", 192, 2048, 256, target=0, bn=256) == go.Plan(1, 2048, 128, 8)


# ---- the packers, against a plain restatement of their layout comments

def _nk(N, K):
  n = torch.arange(N)[:, None].expand(N, K)
  k = torch.arange(K)[None, :].expand(N, K)
  return n, k


def test_pack_decode_weight_layout():
  N, K = 96, 192
  n, k = _nk(N, K)
  wp = ops.pack_decode_weight((n * K + k).contiguous())
  assert wp.shape == (N // 32, K // 16, 2, 32, 8)  # [.., k-half, n-row, 8]: lane = (k-half) * 32 + n-row
  # [N/32][K/16][lane][8], lane = (k-half) * 32 + n-row: element j of lane l of fragment (a, b)
  a, b, l, j = torch.meshgrid(torch.arange(N // 32), torch.arange(K // 16), torch.arange(64), torch.arange(8), indexing="ij")
  assert torch.equal(wp.view(N // 32, K // 16, 64, 8), (a * 32 + l % 32) * K + b * 16 + (l // 32) * 8 + j)


def test_pack_decode_weight_glu_layout():
  I, K = 128, 128
  N = 2 * I
  n, k = _nk(N, K)
  wp = ops.pack_decode_weight_glu((n * K + k).contiguous())
  a, b, l, j = torch.meshgrid(torch.arange(N // 32), torch.arange(K // 16), torch.arange(64), torch.arange(8), indexing="ij")
  # packed row r = 32 a + l % 32; p = (r % 32) // 16, w = r % 16; column c = 16 a + 8 p + w % 8,
  # the gate row c when w < 8, else the up row I + c
  r = l % 32
  col = 16 * a + 8 * (r // 16) + r % 8
  row = torch.where(r % 16 < 8, col, I + col)
  assert torch.equal(wp.view(N // 32, K // 16, 64, 8), row * K + b * 16 + (l // 32) * 8 + j)
  assert torch.equal(wp, ops.pack_decode_weight((n * K + k)[ops.glu_interleave_perm(I)].contiguous()))


def test_pack_decode_weight_fp8_layout():
  N, K = 64, 256
  n, k = _nk(N, K)
  # positive e4m3 codes 0 .. 126 that depend on (n, k); 126 (= 448) once per row, so the row scale is exactly 1
  code = ((n * 31 + k * 17) % 126).to(torch.uint8)
  code[torch.arange(N), torch.arange(N) * 3 % K] = 126
  w = code.view(torch.float8_e4m3fn).float()
  wp8, sw = ops.pack_decode_weight_fp8(w)
  assert torch.equal(sw, torch.ones(N)) and wp8.dtype == torch.uint8 and wp8.numel() == N * K
  a, b, l, j = torch.meshgrid(torch.arange(N // 32), torch.arange(K // 16), torch.arange(64), torch.arange(8), indexing="ij")
  assert torch.equal(wp8.view(N // 32, K // 16, 64, 8), code[a * 32 + l % 32, b * 16 + (l // 32) * 8 + j])
  # the oracle's own fp8 image is this permute
  sp = go.Spec("fp8", 32, 64, 128)
  c = go.build_case(sp)
  _, _, mine, _ = go.launch_args(c)
  theirs, s = ops.pack_decode_weight_fp8(c.w[0].float() * 448.0)  # +-448: scale exactly 1
  assert torch.equal(s, torch.ones(128))
  assert torch.equal((mine[0].view(torch.float8_e4m3fn).float() * 448.0), theirs.view(torch.float8_e4m3fn).float())
