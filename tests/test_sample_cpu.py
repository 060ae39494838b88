"""The torch twin of the sampling kernel (torch_ref.sample) and the admit
header's sampling word."""
import pytest
import torch

from xotorch_amd.ops import torch_ref
from xotorch_amd.serve_ring import pack_sample_word, unpack_sample_word


@pytest.mark.parametrize("top_k,top_p", [(7, 0.0), (0, 0.6), (7, 0.6)])
def test_kept_set_equals_softmax_sample_filter_without_ties(top_k, top_p):
  """On tie-free rows the class rule and softmax_sample's sorted rule keep the
  same set: a token softmax_sample can never return is one it filtered."""
  B, V, temp = 6, 50, 0.7
  logits = torch.randn(B, V, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * 2
  keep, _, _ = torch_ref.sample_kept(logits, torch.full((B,), temp), torch.full((B,), top_k, dtype=torch.int32),
                                     torch.full((B,), top_p))
  # softmax_sample's filter, replayed on its own float32 arithmetic
  x = logits.float() / temp
  if top_k:
    x = torch.where(x < torch.topk(x, top_k).values[:, -1:], float("-inf"), x)
  if top_p:
    sx, idx = torch.sort(x, descending=True)
    pr = torch.softmax(sx, -1)
    x = torch.full_like(x, float("-inf")).scatter(-1, idx, sx.masked_fill(pr.cumsum(-1) - pr > top_p, float("-inf")))
  assert torch.equal(keep, x > float("-inf"))


@pytest.mark.parametrize("u,want", [(0.0, 1), (0.22, 1), (0.23, 2), (0.55, 2), (0.56, 3), (0.999, 3)])
def test_inverse_cdf_draw_on_four_tokens(u, want):
  """Weights 0.1, 0.2, 0.3, 0.4; top-k 3 drops index 0. The kept masses 0.2,
  0.3, 0.4 in index order over W' = 0.9 put the edges at u = 2/9 and 5/9."""
  logits = torch.tensor([[0.1, 0.2, 0.3, 0.4]], dtype=torch.float64).log()
  tok = torch_ref.sample(logits, torch.tensor([1.0]), torch.tensor([3], dtype=torch.int32),
                         torch.tensor([0.0]), torch.tensor([u], dtype=torch.float64))
  assert int(tok[0]) == want


def test_sample_word_round_trip():
  assert pack_sample_word(0.6) == int(0.6 * 1000) and pack_sample_word(0.0) == 0
  assert unpack_sample_word(pack_sample_word(0.6)) == (0.6, 0.0, 0)
  assert unpack_sample_word(pack_sample_word(0.8, 0.5, 4)) == (0.8, 0.5, 4)
  assert unpack_sample_word(pack_sample_word(1.25, 1.0, 0)) == (1.25, 0.0, 0)  # top_p 1 is off
