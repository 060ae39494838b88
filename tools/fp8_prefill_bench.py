"""Kernel timings of docs/PERF.md, "fp8-KV prefill attention": the fp8-KV
prefill kernel against the bf16 MFMA prefill kernel and the plain-cache route
that fp8-KV prefill takes without XOT_FP8_KV_PREFILL=1 (sdpa, or the eager
softcap / window path). Device events around ITERS calls (EAGER_ITERS on the
eager path) after 3 warm-up calls, the routes alternating, 5 samples each;
one JSON line per shape.

  python tools/fp8_prefill_bench.py
"""
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from xotorch_amd import ops  # noqa: E402
from xotorch_amd.ops import torch_ref  # noqa: E402

ITERS, EAGER_ITERS, SAMPLES = 200, 10, 5


def pack_k(k):  # [B, KVH, T, hd], T % 32 == 0 -> [B, KVH, T/16, hd/32, 64, 8]
  B, KVH, T, hd = k.shape
  return k.view(B, KVH, T // 16, 16, hd // 32, 4, 8).permute(0, 1, 2, 4, 5, 3, 6).contiguous().view(
    B, KVH, T // 16, hd // 32, 64, 8)


def pack_v(v):  # -> [B, KVH, hd/16, T/32, 64, 8]
  B, KVH, T, hd = v.shape
  return v.view(B, KVH, T // 32, 4, 8, hd // 16, 16).permute(0, 1, 5, 2, 3, 6, 4).contiguous().view(
    B, KVH, hd // 16, T // 32, 64, 8)


def timed(fn, iters):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(iters):
    fn()
  end.record()
  torch.cuda.synchronize()
  return start.elapsed_time(end) / iters


def shape(name, B, S, H, KVH, hd, softcap, window):
  hip = ops._hip
  g = torch.Generator(device="cuda").manual_seed(3)
  scale = hd ** -0.5
  k = torch.randn(B, KVH, S, hd, device="cuda", generator=g).bfloat16()
  v = (0.5 * torch.randn(B, KVH, S, hd, device="cuda", generator=g)).bfloat16()
  q = torch.randn(B, S, H, hd, device="cuda", generator=g).bfloat16()
  ksc = (k.float().abs().amax(-1).clamp_min(1e-12) / 448).contiguous()
  vsc = (v.float().abs().amax(-1).clamp_min(1e-12) / 448).contiguous()
  k8 = (k.float() / ksc[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
  v8 = (v.float() / vsc[..., None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
  kp, vp, kp8, vp8 = pack_k(k), pack_v(v), pack_k(k8), pack_v(v8)
  routes = {
    "fp8_kv_kernel": lambda: hip.attn_prefill_mfma(q, kp8, vp8, 0, scale, softcap, window, ksc, vsc),
    "bf16_kernel": lambda: hip.attn_prefill_mfma(q, kp, vp, 0, scale, softcap, window),
  }
  if not softcap and not window:
    routes["sdpa_plain"] = lambda: ops.attn_prefill(q, k, v, 0, S, None, None, scale=scale)
  else:
    routes["eager_plain"] = lambda: torch_ref.attn_prefill(q, k, v, 0, S, scale, softcap, window)
  # the two kernels differ by the e4m3 quantisation of K and V only
  o8, ob = routes["fp8_kv_kernel"]().float(), routes["bf16_kernel"]().float()
  res = {"shape": name, "max_abs_diff_fp8_vs_bf16_kernel": (o8 - ob).abs().max().item(),
         "mean_abs_out": ob.abs().mean().item()}
  del o8, ob
  samples = {n: [] for n in routes}
  for n, f in routes.items():
    try:
      for _ in range(3):
        f()
      torch.cuda.synchronize()
    except torch.OutOfMemoryError:
      samples[n] = "out of memory"
      torch.cuda.empty_cache()
  for _ in range(SAMPLES):
    for n, f in routes.items():
      if not isinstance(samples[n], str):
        samples[n].append(timed(f, EAGER_ITERS if n == "eager_plain" else ITERS))
  for n, ts in samples.items():
    res[n + "_ms"] = ts if isinstance(ts, str) else {"median": sorted(ts)[len(ts) // 2], "min": min(ts), "max": max(ts)}
  print(json.dumps(res), flush=True)


if __name__ == "__main__":
  assert torch.cuda.is_available() and ops.hip_available(), "needs a GPU and the built HIP extension"
  shape("70b B=64 S=512 H=64 KVH=8 hd=128", 64, 512, 64, 8, 128, 0.0, 0)
  shape("gemma2-9b B=64 S=512 H=16 KVH=8 hd=256", 64, 512, 16, 8, 256, 0.0, 0)
  shape("gemma2-9b B=64 S=512 H=16 KVH=8 hd=256 softcap=50 window=4096", 64, 512, 16, 8, 256, 50.0, 4096)
