"""fp8-KV prefill attention (attn_prefill_mfma over the e4m3 packed cache and
its per-position scales): the kernel against an fp64 reference under the
derived bf16-P bound of tests/attn_oracle.py, and the model route on a
packed-only fp8 cache against today's plain-cache route."""
import pytest
import torch

from attn_oracle import pack_k, pack_v, prefill_reference

pytestmark = pytest.mark.gpu


def _reference(q, k, v, start_pos, scale, softcap, window):
  """fp64 over q's bf16 values and the dequantised k / v [B, KVH, T, hd] -> (ref, bound), [B, S, H, hd]."""
  B, S = q.shape[:2]
  end = (start_pos + 1 + torch.arange(S)).expand(B, S)
  return prefill_reference(q, k, v, end, scale, softcap, window)


@pytest.mark.parametrize("hd,B,H,KVH,S,start_pos,softcap,window", [
  (128, 1, 1, 1, 16, 0, 0.0, 0),       # one sub-tile, one tile
  (128, 2, 4, 2, 130, 0, 0.0, 0),      # second q block holding 2 rows, GQA, batch stride
  (128, 2, 2, 1, 48, 40, 0.0, 0),      # chunk offset that is no multiple of 32
  (128, 1, 2, 2, 33, 95, 0.0, 0),      # T = 128: full last tile
  (128, 1, 4, 2, 100, 30, 30.0, 40),   # tile skipping at the window start
  (256, 2, 4, 2, 70, 0, 0.0, 0),       # 64-row q blocks, NT = 1
  (256, 1, 2, 1, 40, 50, 30.0, 40),    # gemma2-9b flags
])
def test_attn_prefill_fp8_vs_fp64(hd, B, H, KVH, S, start_pos, softcap, window):
  from xotorch_amd import ops
  T = start_pos + S
  cap = (T + 31) // 32 * 32 + 32  # at least one whole tile beyond T
  g = torch.Generator().manual_seed(1000 * S + start_pos + hd)
  e4m3 = lambda x: x.clamp(-448, 448).to(torch.float8_e4m3fn)
  # codes of std 112 (saturating at 4 sigma); per-position scales over a 4x range: K rows of
  # magnitude 1..4 against q of std 0.5, V magnitudes about 0.5. From T on: poison.
  k8 = e4m3(112 * torch.randn(B, KVH, cap, hd, generator=g))
  v8 = e4m3(112 * torch.randn(B, KVH, cap, hd, generator=g))
  ksc = (4.0 ** torch.rand(B, KVH, cap, generator=g)) / 112
  vsc = (4.0 ** torch.rand(B, KVH, cap, generator=g)) / 448
  for codes, sc in ((k8, ksc), (v8, vsc)):
    codes.view(torch.uint8)[:, :, T:] = 0x7E
    sc[:, :, T:] = 1e30
  q = (0.5 * torch.randn(B, S, H, hd, generator=g)).bfloat16()
  scale = hd ** -0.5
  deq = lambda codes, sc: codes[:, :, :T].float().double() * sc[:, :, :T, None].double()
  ref, bound = _reference(q, deq(k8, ksc), deq(v8, vsc), start_pos, scale, softcap, window)
  off = lambda sc: sc[:, :, :T].roll(1, -1)  # every live position takes a live neighbour's scale
  for name, kx, vx in (("k_scale", deq(k8, off(ksc)), deq(v8, vsc)), ("v_scale", deq(k8, ksc), deq(v8, off(vsc)))):
    moved, _ = _reference(q, kx, vx, start_pos, scale, softcap, window)
    assert ((moved - ref).abs() / bound).max() > 4, f"inputs cannot tell a {name} read one position off"
  qkv = torch.zeros(B, S, H + 2, hd, dtype=torch.bfloat16)  # q as the strided view the models pass
  qkv[:, :, :H] = q
  out = ops.attn_prefill(qkv.cuda()[:, :, :H], None, None, start_pos, S,
                         pack_k(k8.view(torch.uint8), cap).cuda(), pack_v(v8.view(torch.uint8), cap).cuda(),
                         scale=scale, softcap=softcap, window=window, k_scale=ksc.cuda(), v_scale=vsc.cuda())
  assert out.shape == (B, S, H, hd) and out.dtype == torch.bfloat16
  ratio = ((out.cpu().double() - ref).abs() / bound).max().item()
  print(f"attn_prefill fp8-KV hd={hd} B={B} H={H}/{KVH} S={S} start_pos={start_pos} softcap={softcap} "
        f"window={window}: worst err / bound {ratio:.3f}")
  assert ratio <= 1, ratio


@pytest.mark.parametrize("plain", [False, True])
def test_llama_fp8_kv_prefill_route(monkeypatch, plain):
  """Tiny 2-layer hd-128 llama under XOT_FP8_KV=1: prefill of 40 tokens, a
  30-token chunk at start_pos 40 and one decode step with XOT_FP8_KV_PREFILL=1
  (packed-only cache, and plain tensors kept) against XOT_FP8_KV_PREFILL=0,
  today's route over the plain bf16 cache."""
  from xotorch_amd import ops
  from xotorch_amd.engine.kvcache import ShardKVCache
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import ShardedModel
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  raw = dict(model_type="llama", vocab_size=512, hidden_size=256, intermediate_size=512,
             num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
             head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=128)
  cfg = config_from_hf(raw, "fp8kv-tiny")
  torch.manual_seed(9)
  m = ShardedModel(cfg, Shard("fp8kv-tiny", 0, 1, 2)).to("cuda").to(torch.bfloat16)
  random_init(m)
  m.reset_rope()
  m.eval()
  B, chunks = 2, ((0, 40), (40, 30))
  toks = torch.randint(0, 512, (B, 70), device="cuda")
  assert ops.hip_available()
  scaled_calls = []
  kernel = ops._hip.attn_prefill_mfma
  monkeypatch.setattr(ops._hip, "attn_prefill_mfma",
                      lambda *a: scaled_calls.append(len(a) == 9 and a[7] is not None and a[8] is not None) or kernel(*a))

  def run(knob, plain):
    monkeypatch.setenv("XOT_FP8_KV", "1")
    monkeypatch.setenv("XOT_FP8_KV_PREFILL", knob)
    cache = ShardKVCache(2, B, 2, 96, 128, torch.bfloat16, "cuda", plain=plain)
    with torch.inference_mode():
      logits = torch.cat([m(toks[:, s0:s0 + n], caches=cache.caches, start_pos=s0,
                            positions=torch.arange(s0, s0 + n, dtype=torch.int32, device="cuda"))
                          for s0, n in chunks], dim=1)
      nxt = toks[:, :1]
      dec = m(nxt, caches=cache.caches, positions=torch.tensor([70], dtype=torch.int32, device="cuda"), start_pos=70,
              is_decode=True, seq_lens=torch.full((B,), 71, dtype=torch.int32, device="cuda"))
    return cache, logits.float(), dec.float()

  cache, logits, dec = run("1", plain)
  kv = cache.caches[0]
  assert (kv.k is None) == (kv.v is None) == (not plain)
  if not plain:  # 1 byte per element and one fp32 scale per (kv head, position), for K and for V
    assert cache.nbytes() == 2 * 2 * B * 2 * 96 * (128 + 4)
  assert kv.kp.dtype == torch.uint8 and kv.ksc is not None and kv.vsc is not None
  assert scaled_calls == [True] * 4, "2 layers x 2 chunks must take the fp8-KV prefill kernel"
  cache0, logits0, dec0 = run("0", False)  # plain=False is ignored without the knob
  assert cache0.caches[0].k is not None and len(scaled_calls) == 4
  assert (logits.argmax(-1) == logits0.argmax(-1)).all()
  assert torch.allclose(dec, dec0, atol=0.5, rtol=0.1), (dec - dec0).abs().max()
