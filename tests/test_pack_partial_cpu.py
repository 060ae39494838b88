"""pack_group_partial: the module-by-module pack loop stops at the budget."""
import torch

from xotorch_amd.models.llama import pack_group_partial


class StubLinear:
  def __init__(self, n, k):
    self.weight = torch.empty(n, k, device="meta")
    self.packed = False

  def pack_decode(self):
    self.packed = True


class FakeHBM:
  """Free-memory function of a device on which every pack takes its bytes."""

  def __init__(self, free, grp, bytes_per):
    self.free, self.grp, self.bytes_per, self.reads = free, grp, bytes_per, 0

  def __call__(self):
    self.reads += 1
    return self.free - sum(m.weight.numel() * self.bytes_per for m in self.grp if m.packed)


def test_stops_at_the_budget():
  grp = [StubLinear(128, 64) for _ in range(10)]  # 16 KiB each in bf16
  one = 128 * 64 * 2
  reserve = 100 * one
  hbm = FakeHBM(reserve + 3 * one + one // 2, grp, 2)  # room for three and a half
  assert pack_group_partial(grp, 2, reserve, hbm) == 3
  assert [m.packed for m in grp] == [True] * 3 + [False] * 7
  assert hbm.reads == 4  # read again before every module, the refused one included
  assert hbm() - reserve < one  # what is left would not have held another


def test_exact_fit_packs_and_reserve_stays_free():
  grp = [StubLinear(256, 64), StubLinear(128, 64), StubLinear(128, 64)]
  reserve = 1 << 20
  hbm = FakeHBM(reserve + (256 + 128) * 64 * 2, grp, 2)
  assert pack_group_partial(grp, 2, reserve, hbm) == 2
  assert hbm() == reserve


def test_nothing_fits_and_everything_fits():
  grp = [StubLinear(128, 64) for _ in range(4)]
  assert pack_group_partial(grp, 2, 1 << 20, FakeHBM(1 << 20, grp, 2)) == 0
  assert not any(m.packed for m in grp)
  assert pack_group_partial(grp, 1, 0, FakeHBM(4 * 128 * 64, grp, 1)) == 4  # fp8: one byte per weight
  assert all(m.packed for m in grp)
