"""ops.sample on the GPU (sample_rows_kernel) against the float64 definition
(torch_ref.sample_kept): the drawn token lies in the reference's kept set and
its CDF interval holds u within EPS.

EPS = 2^-16, from the kernel's arithmetic, in units of the kept mass W' (>= 1:
the row max has w = 1 and is always kept). A weight is w = expf(d) with
d = (l - max) * (1 / T) in fp32: three roundings and the reciprocal, each
<= 2^-24 relative, so |d| * 4 * 2^-24 on the argument, where |d| <= 28 for any
element with mass; expf is documented to 1 ulp, 2^-23 relative. Together
delta = (2 + 112) * 2^-24 per weight, hence per partial sum. Masses are
truncated to 2^-40 and summed as integers, exactly: at most V * 2^-40 <= 2^-23
in all (V <= 2^17), which also covers the skipped elements below 2^-40. The
kernel picks t with C'_{t-1} <= u * W'' < C'_t on its own sums, each within
delta of the reference's, so the reference's interval holds u * W' within
(2 * delta + 2^-23) * W' = 230 * 2^-24 * W' < 2^-16 * W'.
"""
import pytest
import torch

from xotorch_amd import ops
from xotorch_amd.ops import torch_ref

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -16
U_MAX = 1.0 - 2.0 ** -24  # the largest float32 below 1
SHAPES = [1000, 32768 + 17, 128256]
DTYPES = [torch.bfloat16, torch.float32]


def _run_and_check(logits, temp, top_k, top_p, u, family):
  """Two launches agree; every row's token against the reference."""
  args = [t.cuda() for t in (logits, temp, top_k, top_p, u)]
  tok = ops.sample(*args[:4], u=args[4]).cpu()
  assert torch.equal(tok, ops.sample(*args[:4], u=args[4]).cpu())
  keep, w, greedy = torch_ref.sample_kept(logits, temp, top_k, top_p)
  c = (w * keep).cumsum(-1)
  total, target = c[:, -1], u.double() * c[:, -1]
  hi = c.gather(1, tok[:, None])[:, 0]
  lo = hi - (w * keep).gather(1, tok[:, None])[:, 0]
  excess = (torch.maximum(lo - target, target - hi).clamp_min(0) / total)[~greedy]
  print(f"{family} V={logits.shape[1]} {logits.dtype}: worst excess {excess.max().item():.3e} (EPS {EPS:.3e})")
  assert torch.equal(tok[greedy], logits.argmax(-1)[greedy])
  assert keep.gather(1, tok[:, None])[~greedy].all()
  assert (excess <= EPS).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", SHAPES)
def test_ladder_and_mixed_rows(V, dtype):
  """40 live tokens on 10 rungs of 4 (ties at the k-th value and on the top-p
  class), the rest 40 lower after the temperature 0.5; live tokens at both row
  ends, on both sides of the kernel's 16 B unit, wave tile and 16-tile round
  (rows of an odd V start at every alignment) and at random places. Each weighs
  over 1 %: one token wrongly kept or dropped moves every interval far beyond
  EPS. 60 rows = top-k / top-p / both / neither x 15 u with 0 and U_MAX, and 3
  greedy rows (temperature 0 and 1e-4, the maximum tied four ways) in the launch."""
  g = torch.Generator().manual_seed(V)
  fixed = [0, 1, 3, 4, 7, 8, 255, 256, 511, 512, 513, 1023, 1024, 4095, 4096, 8191, 8192, V - 2, V - 1]
  live = sorted({i for i in fixed if 0 <= i < V})
  while len(live) < 40:
    live = sorted(set(live) | {int(torch.randint(V, (1,), generator=g))})
  row = torch.full((V,), -20.0)
  rungs = (2.0 - 0.0625 * torch.arange(10)).repeat(4)
  row[torch.tensor(live)] = rungs[torch.randperm(40, generator=g)]
  settings = [(10, 0.0), (0, 0.5), (10, 0.5), (0, 0.0)]  # k = 10: inside the third rung's tie run
  us = torch.cat([torch.tensor([0.0, U_MAX]), torch.rand(13, generator=g)])
  B = 63
  logits = row.to(dtype).repeat(B, 1)
  assert torch.equal(logits.float()[0], row)  # exact in bf16
  temp = torch.full((B,), 0.5)
  temp[60:] = torch.tensor([0.0, 1e-4, 1e-4])
  top_k = torch.tensor([s[0] for s in settings], dtype=torch.int32).repeat_interleave(15)
  top_p = torch.tensor([s[1] for s in settings]).repeat_interleave(15)
  top_k, top_p = torch.cat([top_k, top_k[:3]]), torch.cat([top_p, top_p[:3]])
  u = torch.cat([us.repeat(4), us[:3]])
  # in the reference alone, no value class within 2^-10 * W_k of the top-p cut
  keep, w, _ = torch_ref.sample_kept(logits[::15][:4], temp[::15][:4], top_k[::15][:4], top_p[::15][:4])
  for r, (k, p) in enumerate(settings):
    if p:
      w_k = w[r][row >= row.sort(descending=True).values[(k or V) - 1]].sum()
      for v in row.unique():
        assert abs(w[r][row > v].sum() - p * w_k) > 2.0 ** -10 * w_k
  assert [int(x) for x in keep.sum(-1)] == [12, 16, 8, V]
  _run_and_check(logits, temp, top_k, top_p, u, "ladder")


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", SHAPES)
def test_plain_rows(V, dtype, B):
  """Random logits of std 2; temperature, top-k and top-p differ row by row. The
  flat tail's intervals are narrower than EPS: membership and the inequality."""
  g = torch.Generator().manual_seed(V + B)
  logits = (2.0 * torch.randn(B, V, generator=g)).to(dtype)
  r = torch.arange(B)
  temp = torch.where(r % 2 == 0, 0.3, 1.0)
  top_k = torch.where((r // 2) % 2 == 0, 35, 0).to(torch.int32)
  top_p = torch.where((r // 4) % 2 == 0, 0.9, 0.0)
  _run_and_check(logits, temp, top_k, top_p, torch.rand(B, generator=g), "plain")
