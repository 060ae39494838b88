#!/usr/bin/env python3
"""Decode-GEMM shape race: hipBLASLt (TunableOp) vs packed-LDS (v2, on its
128-row and its 256-row weight tile) vs packed-xreg (v3) vs the MXFP4
weight-only kernel on the 70B/8B decode shapes at M=32/64/128/256. The 256-row
tile exists for M >= 128 and N % 256 == 0; elsewhere XOT_SKINNY_BN=256 runs the
128-row tile and the two columns agree. The mxfp4 column runs the weight
quantized to MXFP4 (its own default tile); TB/s always counts the bf16 bytes
of the weight, so the mxfp4 figure is bf16-equivalent, not bytes moved.
Every gate_up shape also gets a "+swiglu" row per M: the packed GEMM plus
swiglu_packed, the GEMM with SwiGLU in its store (GLU-interleaved pack), and
hipBLASLt plus swiglu_packed; the fused result is checked equal to the
two-step one before it is timed.

Run on a GPU box:
  python tools/gemm_decode_bench.py [--check-only]
"""
import argparse
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from xotorch_amd import ops
from xotorch_amd.ops import _load_hip

SHAPES = [
  # (name, N, K)  — 70B decode shapes + lm_head; 8B qkv/gate_up for reference
  ("qkv70",     10240, 8192),
  ("o70",        8192, 8192),
  ("gate_up70", 57344, 8192),
  ("down70",     8192, 28672),
  ("lm_head",  128256, 8192),
  ("qkv8",       6144, 4096),
  ("gate_up8",  28672, 4096),
]


def time_us(fn, reps=20, rounds=5):
  fn()
  torch.cuda.synchronize()
  best = float("inf")
  for _ in range(rounds):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
      fn()
    e.record()
    e.synchronize()
    best = min(best, s.elapsed_time(e) * 1000.0 / reps)
  return best


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--check-only", action="store_true")
  p.add_argument("--ms", type=str, default="32,64,128,256")
  p.add_argument("--shapes", type=str, default="", help="comma-separated shape names (default: all)")
  args = p.parse_args()
  hip = _load_hip()
  assert hip is not None, "HIP extension missing"
  dev = "cuda"
  torch.manual_seed(7)
  print(f"{'shape':<10} {'M':>4} {'blaslt':>9} {'pk-bn128':>9} {'pk-bn256':>9} {'pk-bk64':>9} {'xreg':>9} {'mxfp4':>9}"
        "  best bf16 (TB/s of weight stream) | mxfp4 (bf16-equivalent TB/s, speedup over best bf16)")
  wanted = [n for n in args.shapes.split(",") if n]
  for name, N, K in SHAPES:
    if wanted and name not in wanted:
      continue
    w = (torch.randn(N, K, device=dev) / K**0.5).to(torch.bfloat16)
    wp = ops.pack_decode_weight(w)
    wbytes = N * K * 2
    wq, ws, w_dq = ops.pack_decode_weight_mxfp4(w)
    wp_dq = ops.pack_decode_weight(w_dq)
    del w_dq
    for M in [int(m) for m in args.ms.split(",")]:
      x = (torch.randn(M, K, device=dev) / 4).to(torch.bfloat16)
      ref = torch.nn.functional.linear(x, w)
      yp = hip.skinny_gemm_packed(x, wp, N, None)
      yx = hip.skinny_gemm_packed_xreg(x, wp, N, None)
      for tag, y in (("packed", yp), ("xreg", yx)):
        err = (y.float() - ref.float()).abs().max().item()
        scale = ref.float().abs().max().item()
        assert err < 0.02 * max(scale, 1.0) + 0.05, f"{name} M={M} {tag}: err {err} scale {scale}"
      # mxfp4: no tolerance, the bits of the bf16 kernel on the dequantized weight
      y4 = hip.skinny_gemm_mxfp4(x, wq, ws, 1, N, None)
      assert torch.equal(y4, hip.skinny_gemm_packed(x, wp_dq, N, None)), f"{name} M={M} mxfp4: bits differ"
      glu_row = name.startswith("gate_up") and hip.skinny_plan_nsplit(N, K) == 1
      if glu_row:
        wg = ops.pack_decode_weight_glu(w)
        two_step = lambda: hip.swiglu_packed(hip.skinny_gemm_packed(x, wp, N, None))
        fused = lambda: hip.skinny_gemm_packed_glu(x, wg, N)
        assert torch.equal(fused(), two_step()), f"{name} M={M} fused SwiGLU store: bits differ"
      if args.check_only:
        print(f"{name:<10} {M:>4} ok")
        continue
      if glu_row:
        t_two, t_fused = time_us(two_step), time_us(fused)
        t_lib = time_us(lambda: hip.swiglu_packed(torch.nn.functional.linear(x, w)))
        print(f"{name:<10} {M:>4} +swiglu: packed {t_two:.1f} us, fused store {t_fused:.1f} us, "
              f"blaslt {t_lib:.1f} us", flush=True)
        del wg
      t_bl = time_us(lambda: torch.nn.functional.linear(x, w))
      os.environ["XOT_SKINNY_BN"] = "128"
      t_pk = time_us(lambda: hip.skinny_gemm_packed(x, wp, N, None))
      os.environ["XOT_SKINNY_BN"] = "256"
      t_pw = time_us(lambda: hip.skinny_gemm_packed(x, wp, N, None))
      del os.environ["XOT_SKINNY_BN"]
      os.environ["XOT_SKINNY_BK64"] = "1"
      t_p64 = time_us(lambda: hip.skinny_gemm_packed(x, wp, N, None))
      del os.environ["XOT_SKINNY_BK64"]
      t_xr = time_us(lambda: hip.skinny_gemm_packed_xreg(x, wp, N, None))
      t_w4 = time_us(lambda: hip.skinny_gemm_mxfp4(x, wq, ws, 1, N, None))
      best = min(t_bl, t_pk, t_pw, t_p64, t_xr)
      tbps = wbytes / best / 1e6
      win = {t_bl: "blaslt", t_pk: "pk-bn128", t_pw: "pk-bn256", t_p64: "pk-bk64", t_xr: "xreg"}[best]
      print(f"{name:<10} {M:>4} {t_bl:>9.1f} {t_pk:>9.1f} {t_pw:>9.1f} {t_p64:>9.1f} {t_xr:>9.1f} {t_w4:>9.1f}"
            f"  {win} {tbps:.2f} TB/s | {wbytes / t_w4 / 1e6:.2f} TB/s x{best / t_w4:.2f}", flush=True)
    del w, wp, wq, ws, wp_dq
    torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
