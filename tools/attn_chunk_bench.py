#!/usr/bin/env python3
"""Short-chunk attention behind a long cache: ops.attn_prefill on the prefill
kernel (XOT_ATTN_CHUNK=0) against the split-KV chunk kernel (XOT_ATTN_CHUNK=1),
both in this process, alternating, on the same seeded inputs; then the chunk
kernel under XOT_ATTN_CHUNK_NSPLIT = 1 .. 32 for the shapes of --sweep.
Every shape runs in a cache that just holds it ("tight") and in a preallocated
one of --capacity positions, as the serve and speculative caches are.

Time per call = device events around a window of back-to-back launches, at
least `--calls` of them and at least `--window-ms` long, median of `--samples`
such windows taken alternately for the two routes. Back-to-back calls on one
K/V set are warm-cache figures for both routes (the set can stay in L2 / MALL).
Prints one markdown table row per shape (docs/PERF.md keeps a run)."""
import argparse
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from xotorch_amd import ops


def inputs(hd, B, H, KVH, S, start, fp8, cap=0):
  cap = max(cap, (start + S + 31) // 32 * 32)
  g = torch.Generator(device="cuda").manual_seed(start + S + H)
  q = (0.5 * torch.randn(B, S, H + 2 * KVH, hd, device="cuda", generator=g)).bfloat16()[:, :, :H]
  shapes = ((B, KVH, cap // 16, hd // 32, 64, 8), (B, KVH, hd // 16, cap // 32, 64, 8))
  if fp8:
    kp, vp = (torch.randn(s, device="cuda", generator=g).mul(112).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
              for s in shapes)
    sc = dict(k_scale=torch.rand(B, KVH, cap, device="cuda", generator=g) / 50 + 0.01,
              v_scale=torch.rand(B, KVH, cap, device="cuda", generator=g) / 400 + 0.001)
  else:
    kp, vp = (torch.randn(s, device="cuda", generator=g).mul(std).bfloat16() for s, std in zip(shapes, (2.5, 0.5)))
    sc = {}
  return (lambda: ops.attn_prefill(q, None, None, start, S, kp, vp, **sc)), cap


def window_us(call, calls):
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(calls):
    call()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) * 1e3 / calls


def measure(call, settings, calls, samples, window_ms):
  """settings: list of env dicts; -> (median us per setting, outputs)."""
  outs, times, ncalls = [], [[] for _ in settings], []
  for env in settings:  # warm every route, and size its window
    os.environ.update(env)
    for _ in range(5):
      out = call()
    outs.append(out.float())
    ncalls.append(max(calls, int(window_ms * 1e3 / window_us(call, 10)) + 1))
  for _ in range(samples):
    for i, env in enumerate(settings):
      os.environ.update(env)
      times[i].append(window_us(call, ncalls[i]))
  return [statistics.median(t) for t in times], outs


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--calls", type=int, default=50)
  p.add_argument("--samples", type=int, default=7)
  p.add_argument("--window-ms", type=float, default=50.0)
  p.add_argument("--capacity", type=int, default=32768, help="positions of the preallocated cache")
  p.add_argument("--sweep", action="store_true", help="also sweep XOT_ATTN_CHUNK_NSPLIT at S=5")
  args = p.parse_args()
  assert torch.cuda.is_available() and ops.hip_available(), "needs the GPU and the built extension"
  os.environ.pop("XOT_ATTN_CHUNK_NSPLIT", None)
  print("| cache | capacity | hd | H/KVH | S | B | start_pos | prefill kernel us | chunk kernel us | ratio | max abs diff |")
  print("|---|---|---|---|---|---|---|---|---|---|---|")
  heads = ((128, 64, 8), (128, 32, 8), (256, 16, 8))
  for fp8 in (False, True):
    for hd, H, KVH in heads:
      for S in (5, 8):
        for B in (1, 8):
          for start in (512, 4096, 16384):
            if not ops.attn_chunk_fits(S, H, KVH, hd):
              continue
            for cap in (0, args.capacity):
              call, _ = inputs(hd, B, H, KVH, S, start, fp8, cap)
              (t_old, t_new), (o_old, o_new) = measure(call, [{"XOT_ATTN_CHUNK": "0"}, {"XOT_ATTN_CHUNK": "1"}],
                                                       args.calls, args.samples, args.window_ms)
              print(f"| {'fp8' if fp8 else 'bf16'} | {cap or 'tight'} | {hd} | {H}/{KVH} | {S} | {B} | {start} | {t_old:.1f} | "
                    f"{t_new:.1f} | {t_old / t_new:.2f}x | {(o_old - o_new).abs().max().item():.4f} |", flush=True)
              del call
  if args.sweep:
    print(f"\ncapacity {args.capacity}\n\n| cache | hd | H/KVH | S | B | start_pos | rule | " + " | ".join(f"nsplit {n} us" for n in (1, 2, 4, 8, 16, 32)) + " |")
    print("|" + "---|" * 13)
    os.environ["XOT_ATTN_CHUNK"] = "1"
    for fp8, (hd, H, KVH), B, start in [(f, h, b, s) for f in (False, True) for h in heads for b in (1, 8)
                                        for s in (512, 4096, 16384)]:
      call, cap = inputs(hd, B, H, KVH, 5, start, fp8, args.capacity)
      os.environ.pop("XOT_ATTN_CHUNK_NSPLIT", None)
      rule = ops._gpu().attn_chunk_nsplit(B, KVH, cap)
      ts, _ = measure(call, [{"XOT_ATTN_CHUNK_NSPLIT": str(n)} for n in (1, 2, 4, 8, 16, 32)], args.calls, 5, args.window_ms)
      print(f"| {'fp8' if fp8 else 'bf16'} | {hd} | {H}/{KVH} | 5 | {B} | {start} | {rule} | "
            + " | ".join(f"{t:.1f}" for t in ts) + " |", flush=True)


if __name__ == "__main__":
  main()
