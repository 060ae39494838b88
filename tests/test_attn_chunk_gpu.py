"""Split-KV chunk attention (attn_chunk_mfma: a short query chunk at an offset,
all query heads of a kv head as MFMA rows, split over the KV length) against
an fp64 reference, its refusals, and the XOT_ATTN_CHUNK route of a model.

Bound: the bf16-P bound of tests/attn_oracle.py as the fp8 prefill test states
it (P rounded once to bf16, V scale folded in before that rounding), with the
split-KV merge added to the accumulation term: the merge rescales each of the
nsplit partials once and adds them (nsplit fp32 roundings on O and on L), then
divides and the kernel stored the partial (2 more), so 2^-24 (2 T + 16)
becomes 2^-24 (2 T + 16 + nsplit + 2). No constant is fitted to kernel output.

Worst err / bound measured on the MI355X, bf16 / fp8 cache, in case order:
0.00/0.64, 0.55/0.65, 0.52/0.67, 0.37/0.49, 0.71/0.74, 0.41/0.54, 0.45/0.73, 0.52/0.60;
several tiles per wave 0.38/0.47."""
import pytest
import torch

from attn_oracle import pack_k, pack_v, prefill_reference

pytestmark = pytest.mark.gpu


def _reference(q, k, v, q_start, scale, softcap, window, nsplit, shift=0):
  """fp64 over q's bf16 values and the k / v [B, KVH, T, hd] the kernel reads; row s of sequence b
  sees [end - window, end) with end = q_start[b] + s + 1 + shift -> (ref, bound), [B, S, H, hd]."""
  end = torch.tensor(q_start)[:, None] + torch.arange(q.shape[1])[None, :] + 1 + shift  # [B, S]
  return prefill_reference(q, k, v, end, scale, softcap, window, extra_acc=nsplit + 2)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("hd,B,H,KVH,S,q_start,cap,softcap,window,nsplit", [
  (128, 1, 1, 1, 1, 0, 32, 0.0, 0, 1),         # one row, one position, direct store
  (128, 1, 4, 2, 5, 0, 32, 0.0, 0, 1),         # R = 10: rows that see 1..5 positions, clamped rows
  (128, 2, 8, 2, 5, 29, 256, 0.0, 0, 8),       # R = 20: limits straddle a tile edge, empty splits
  (128, 1, 8, 1, 8, 100, 256, 0.0, 0, 8),      # R = 64, NTQ = 4
  (128, 2, 6, 2, 7, (5, 90), 128, 0.0, 0, 4),  # G = 3, per-sequence offsets
  (128, 1, 4, 2, 6, 70, 128, 30.0, 40, 4),     # window starts straddle a tile edge
  (256, 2, 4, 2, 8, 50, 128, 0.0, 0, 4),       # hd 256, R = 16
  (256, 1, 8, 2, 8, 27, 128, 30.0, 40, 4),     # hd 256 at R = 32, gemma2 flags
])
def test_attn_chunk_vs_fp64(monkeypatch, fp8, hd, B, H, KVH, S, q_start, cap, softcap, window, nsplit):
  _check_case(monkeypatch, fp8, hd, B, H, KVH, S, q_start, cap, softcap, window, nsplit)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_attn_chunk_several_tiles_per_wave(monkeypatch, fp8):
  """XOT_ATTN_CHUNK_NSPLIT=2 over a live range [51, 205) that starts at tile 1: three tiles per wave, so
  the running (m, l), the accumulator rescale and the K prefetch carry state (the rule's chunks above are
  one tile each), and the chunks start at a non-zero base."""
  monkeypatch.setenv("XOT_ATTN_CHUNK_NSPLIT", "2")
  _check_case(monkeypatch, fp8, 128, 1, 8, 2, 5, 200, 256, 0.0, 150, 2)


def _check_case(monkeypatch, fp8, hd, B, H, KVH, S, q_start, cap, softcap, window, nsplit):
  from xotorch_amd import ops
  assert ops.hip_available()
  starts = list(q_start) if isinstance(q_start, tuple) else [q_start] * B
  T = max(starts) + S  # from T to the capacity: poison
  g = torch.Generator().manual_seed(1000 * S + starts[-1] + hd)
  q = (0.5 * torch.randn(B, S, H, hd, generator=g)).bfloat16()
  if fp8:  # codes of std 112 and per-position scales over a 4x range, as the fp8 prefill test
    e4m3 = lambda x: x.clamp(-448, 448).to(torch.float8_e4m3fn)
    k8, v8 = (e4m3(112 * torch.randn(B, KVH, cap, hd, generator=g)) for _ in range(2))
    ksc = (4.0 ** torch.rand(B, KVH, cap, generator=g)) / 112
    vsc = (4.0 ** torch.rand(B, KVH, cap, generator=g)) / 448
    for codes, sc in ((k8, ksc), (v8, vsc)):
      codes.view(torch.uint8)[:, :, T:] = 0x7E
      sc[:, :, T:] = 1e30
    k, v = (c[:, :, :T].float().double() * sc[:, :, :T, None].double() for c, sc in ((k8, ksc), (v8, vsc)))
    kp, vp = pack_k(k8.view(torch.uint8), cap).cuda(), pack_v(v8.view(torch.uint8), cap).cuda()
    scales = dict(k_scale=ksc.cuda(), v_scale=vsc.cuda())
  else:
    kb, vb = ((std * torch.randn(B, KVH, cap, hd, generator=g)).bfloat16() for std in (2.5, 0.5))
    sign = torch.where(torch.rand(B, KVH, cap - T, hd, generator=g) < 0.5, -1e30, 1e30).bfloat16()
    kb[:, :, T:], vb[:, :, T:] = sign, sign
    k, v = kb[:, :, :T].double(), vb[:, :, :T].double()
    kp, vp = pack_k(kb, cap).cuda(), pack_v(vb, cap).cuda()
    scales = {}
  scale = hd ** -0.5
  ref, bound = _reference(q, k, v, starts, scale, softcap, window, nsplit)
  if T > 1:
    moved, _ = _reference(q, k, v, starts, scale, softcap, window, nsplit, shift=-1)
    assert ((moved - ref).abs() / bound).max() > 4, "inputs cannot tell a limit read one position early"
  assert ops._hip.attn_chunk_nsplit(B, KVH, cap) == nsplit
  calls = []
  kernel = ops._hip.attn_chunk_mfma
  monkeypatch.setattr(ops._hip, "attn_chunk_mfma", lambda *a: calls.append(1) or kernel(*a))
  monkeypatch.setattr(ops._hip, "attn_prefill_mfma", lambda *a: pytest.fail("the prefill kernel served the chunk"))
  monkeypatch.setenv("XOT_ATTN_CHUNK", "1")
  qkv = torch.zeros(B, S, H + 2, hd, dtype=torch.bfloat16)  # q as the strided view the models pass
  qkv[:, :, :H] = q
  qv = qkv.cuda()[:, :, :H]
  if isinstance(q_start, tuple):
    out = ops.attn_chunk(qv, kp, vp, torch.tensor(starts, dtype=torch.int32, device="cuda"),
                         scale=scale, softcap=softcap, window=window, **scales)
  else:
    out = ops.attn_prefill(qv, None, None, q_start, S, kp, vp, scale=scale, softcap=softcap, window=window, **scales)
  assert calls == [1] and out.shape == (B, S, H, hd) and out.dtype == torch.bfloat16
  ratio = ((out.cpu().double() - ref).abs() / bound).max().item()
  print(f"attn_chunk {'fp8' if fp8 else 'bf16'} hd={hd} B={B} H={H}/{KVH} S={S} q_start={q_start} cap={cap} "
        f"softcap={softcap} window={window} nsplit={nsplit}: worst err / bound {ratio:.3f}")
  assert ratio <= 1, ratio


def _packed_cache(B, KVH, cap, hd, dtype=torch.bfloat16):
  mk = lambda: torch.randn(B, KVH, cap, hd).to(dtype) if dtype == torch.bfloat16 else torch.zeros(B, KVH, cap, hd, dtype=dtype)
  return pack_k(mk(), cap).cuda(), pack_v(mk(), cap).cuda()


@pytest.mark.parametrize("S,H,KVH,hd,cache_hd,dtype", [
  (65, 1, 1, 128, 128, torch.bfloat16),  # R = 65 at hd 128
  (33, 1, 1, 256, 256, torch.bfloat16),  # R = 33 at hd 256
  (1, 1, 1, 64, 128, torch.bfloat16),    # hd 64
  (1, 3, 2, 128, 128, torch.bfloat16),   # H % KVH != 0
  (1, 2, 2, 128, 128, torch.uint8),      # e4m3 copies without scales
], ids=["rows65", "rows33-hd256", "hd64", "heads", "no-scales"])
def test_attn_chunk_refuses(S, H, KVH, hd, cache_hd, dtype):
  from xotorch_amd import ops
  kp, vp = _packed_cache(1, KVH, 96, cache_hd, dtype)
  q = torch.zeros(1, S, H, hd, dtype=torch.bfloat16, device="cuda")
  with pytest.raises(RuntimeError):
    ops.attn_chunk(q, kp, vp, 0)


def test_attn_prefill_long_chunk_keeps_prefill_kernel(monkeypatch):
  """S = 130 does not fit: with the knob on attn_prefill still runs the prefill kernel, bit for bit."""
  from xotorch_amd import ops
  torch.manual_seed(3)
  kp, vp = _packed_cache(1, 1, 160, 128)
  q = torch.randn(1, 130, 2, 128, device="cuda").bfloat16()
  assert not ops.attn_chunk_fits(130, 2, 1, 128) and ops.attn_chunk_fits(5, 64, 8, 128)
  monkeypatch.setenv("XOT_ATTN_CHUNK", "0")
  off = ops.attn_prefill(q, None, None, 0, 130, kp, vp)
  monkeypatch.setenv("XOT_ATTN_CHUNK", "1")
  monkeypatch.setattr(ops._hip, "attn_chunk_mfma", lambda *a: pytest.fail("the chunk kernel took S = 130"))
  assert torch.equal(ops.attn_prefill(q, None, None, 0, 130, kp, vp), off)


def test_llama_chunk_route(monkeypatch):
  """Tiny 2-layer hd-128 llama: 60 tokens prefilled, then a 5-token chunk at start_pos 60 with
  XOT_ATTN_CHUNK=1 (both layers on the chunk kernel) against XOT_ATTN_CHUNK=0 (none)."""
  from xotorch_amd import ops
  from xotorch_amd.engine.kvcache import ShardKVCache
  from xotorch_amd.models.config import config_from_hf
  from xotorch_amd.models.llama import ShardedModel
  from xotorch_amd.models.weights import random_init
  from xotorch_amd.shard import Shard
  raw = dict(model_type="llama", vocab_size=512, hidden_size=256, intermediate_size=512,
             num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
             head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0, max_position_embeddings=128)
  cfg = config_from_hf(raw, "chunk-tiny")
  torch.manual_seed(9)
  m = ShardedModel(cfg, Shard("chunk-tiny", 0, 1, 2)).to("cuda").to(torch.bfloat16)
  random_init(m)
  m.reset_rope()
  m.eval()
  B = 2
  toks = torch.randint(0, 512, (B, 65), device="cuda")
  calls = []
  kernel = ops._hip.attn_chunk_mfma
  monkeypatch.setattr(ops._hip, "attn_chunk_mfma", lambda *a: calls.append(1) or kernel(*a))

  def run(knob):
    cache = ShardKVCache(2, B, 2, 96, 128, torch.bfloat16, "cuda")
    step = lambda s0, n: m(toks[:, s0:s0 + n], caches=cache.caches, start_pos=s0,
                           positions=torch.arange(s0, s0 + n, dtype=torch.int32, device="cuda"))
    with torch.inference_mode():
      monkeypatch.setenv("XOT_ATTN_CHUNK", "0")
      step(0, 60)
      monkeypatch.setenv("XOT_ATTN_CHUNK", knob)
      return step(60, 5).float()

  on = run("1")
  assert calls == [1, 1], "both layers must take the chunk kernel"
  off = run("0")
  assert calls == [1, 1]
  assert (on.argmax(-1) == off.argmax(-1)).all()
  assert torch.allclose(on, off, atol=0.5, rtol=0.1), (on - off).abs().max()
