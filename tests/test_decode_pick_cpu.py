"""The decode auto-pick rule and the sorted MoE prefill, on the CPU: the timer
and the capture query are patched and the pick function is driven directly."""
import pytest
import torch


@pytest.fixture
def pick(monkeypatch):
  """auto_pick with an empty cache, a timer that returns what the contender
  returns, and a switchable capture query; counts the timer's calls."""
  from xotorch_amd.models import linear
  state = {"timed": 0, "capturing": False}

  def fake_time(fn):
    state["timed"] += 1
    return fn()

  monkeypatch.setattr(linear, "DECODE_PICKS", {})
  monkeypatch.setattr(linear, "_time_us", fake_time)
  monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: state["capturing"])
  return linear, state


def _gemm_race(linear, key, blaslt, packed, xreg):
  return linear.auto_pick(key, "gemm", "NKM", 0.95, lambda: [
    ("blaslt", lambda: blaslt), ("packed", lambda: packed), ("xreg", lambda: xreg)])


def _swiglu_race(linear, key, split, fused):
  return linear.auto_pick(key, "swiglu-fuse", "NIM", 0.98, lambda: [
    ("split", lambda: split), ("fused", lambda: fused)])


@pytest.mark.parametrize("times,want", [
  ((100, 96, 90), "xreg"),     # packed misses the 5 % margin, xreg clears it
  ((100, 94, 94), "packed"),   # a tie with the best so far does not displace it
  ((100, 96, 96), "blaslt"),   # faster, but inside the margin
  ((100, 94, 93), "xreg"),
])
def test_gemm_race(pick, times, want):
  linear, state = pick
  key = (256, 512, 32)
  assert _gemm_race(linear, key, *times) == want
  assert linear.DECODE_PICKS == {key: want}
  assert state["timed"] == 3


@pytest.mark.parametrize("split,fused,want", [(100, 98, "split"), (100, 97.9, "fused")])
def test_swiglu_race(pick, split, fused, want):
  linear, state = pick
  key = ("fuse_swiglu", 256, 512, 32)
  assert _swiglu_race(linear, key, split, fused) == want
  assert linear.DECODE_PICKS == {key: want}
  assert state["timed"] == 2


def test_second_call_does_not_time_again(pick):
  linear, state = pick
  key = (256, 512, 64)
  assert _gemm_race(linear, key, 100, 50, 60) == "packed"
  assert state["timed"] == 3
  assert _gemm_race(linear, key, 100, 200, 10) == "packed"  # cached: the new times are never read
  assert state["timed"] == 3


def test_seeded_key_is_not_raced(pick):
  linear, state = pick
  linear.DECODE_PICKS[(256, 512, 32)] = "blaslt"
  assert _gemm_race(linear, (256, 512, 32), 100, 1, 1) == "blaslt"
  assert state["timed"] == 0


def test_capture_takes_first_challenger_and_caches_nothing(pick):
  linear, state = pick
  state["capturing"] = True
  assert _gemm_race(linear, (256, 512, 32), 1, 100, 50) == "packed"
  assert _swiglu_race(linear, ("fuse_swiglu", 256, 512, 32), 1, 100) == "fused"
  assert state["timed"] == 0
  assert linear.DECODE_PICKS == {}


def test_debug_line_names_shape_times_and_choice(pick, monkeypatch, capsys):
  linear, _ = pick
  monkeypatch.setenv("XOT_DEBUG", "1")
  _gemm_race(linear, (256, 512, 32), 100, 96, 90)
  _swiglu_race(linear, ("fuse_swiglu", 256, 512, 32), 100, 97.9)
  out = capsys.readouterr().out.splitlines()
  assert out == [
    "[xot] gemm auto-pick N=256 K=512 M=32: packed 96.0 us / xreg 90.0 us vs blaslt 100.0 us -> xreg",
    "[xot] swiglu-fuse auto-pick N=256 I=512 M=32: fused 97.9 us vs split 100.0 us -> fused",
  ]


def test_decode_rows_is_zero_off_the_gpu():
  from xotorch_amd.models.linear import decode_rows
  assert decode_rows(torch.zeros(32, 1, 64, dtype=torch.bfloat16), 64) == 0


def test_sorted_expert_prefill_matches_where_loop():
  """The sorted prefill against the per-expert where loop (MoEMLP.forward's
  CPU path) on the tiny Mixtral block of the CPU MoE tests."""
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import MoEMLP
  from xotorch_amd.models.moe import sorted_expert_prefill
  from xotorch_amd.models.registry import builtin_config

  raw = dict(builtin_config("mixtral-8x7b"))
  raw.update(hidden_size=64, intermediate_size=128, num_hidden_layers=2,
             num_attention_heads=4, num_key_value_heads=2)
  cfg = config_from_hf(raw, "mixtral-tiny")
  torch.manual_seed(0)
  moe = MoEMLP(cfg).eval()
  x = torch.randn(3, 7, 64)
  flat = x.view(-1, 64)
  with torch.no_grad():
    ref = moe(x)  # CPU -> where loop
    weights, selected = moe._route(flat)
    got = sorted_expert_prefill(flat, weights, selected, moe.experts)
  assert got.shape == (21, 64) and got.dtype == torch.float32
  # fp32 throughout: the two differ in the order index_add_ sums a token's k
  # terms and in the batch each expert GEMM sees, a few ulp of values O(0.1)
  assert torch.allclose(ref, got.view(3, 7, 64), atol=1e-5, rtol=1e-5), (ref - got.view(3, 7, 64)).abs().max()
