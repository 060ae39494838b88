"""ops.attn_train off the GPU: the expression the llama-family training forward
has always run, bit for bit and with its gradients; the geometry test and the knob."""
import pytest
import torch
import torch.nn.functional as F

from xotorch_amd import ops


def _old_forward_nocache_lines(q, k, v):
  rep = q.shape[2] // k.shape[2]
  out = F.scaled_dot_product_attention(
    q.transpose(1, 2).float(),
    k.transpose(1, 2).repeat_interleave(rep, dim=1).float(),
    v.transpose(1, 2).repeat_interleave(rep, dim=1).float(),
    is_causal=True,
  ).to(q.dtype)
  return out.transpose(1, 2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attn_train_cpu_is_the_old_expression(dtype):
  g = torch.Generator().manual_seed(5)
  B, S, H, KVH, hd = 2, 37, 4, 2, 64
  qkv = torch.randn(B, S, (H + 2 * KVH) * hd, generator=g).to(dtype)
  dout = torch.randn(B, S, H, hd, generator=g).to(dtype)
  res = []
  for fn in (ops.attn_train, _old_forward_nocache_lines):
    x = qkv.clone().requires_grad_(True)
    q, k, v = (t.reshape(B, S, -1, hd) for t in torch.split(x, [H * hd, KVH * hd, KVH * hd], dim=-1))
    out = fn(q, k, v)
    res.append((out, torch.autograd.grad(out, x, dout)[0]))
  assert res[0][0].shape == (B, S, H, hd) and res[0][0].dtype == dtype
  assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_attn_train_fits_and_knob(monkeypatch):
  assert ops.attn_train_fits(32, 8, 64) and ops.attn_train_fits(32, 8, 128)
  assert not ops.attn_train_fits(32, 8, 256) and not ops.attn_train_fits(32, 8, 96)
  assert not ops.attn_train_fits(6, 4, 128)
  monkeypatch.delenv("XOT_TRAIN_ATTN", raising=False)
  assert not ops.attn_train_enabled()
  monkeypatch.setenv("XOT_TRAIN_ATTN", "1")
  assert ops.attn_train_enabled()
