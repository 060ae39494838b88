#!/usr/bin/env python3
"""The routed MoE block above 256 tokens, router to combine, on given fp32 gate
logits: today's route (torch softmax / top-k, moe.sorted_expert_prefill over
per-expert library GEMMs, one host sync) against the ragged route
(ops.moe_route, moe.moe_prefill: moe_plan, two moe_gemm_ragged launches,
moe_combine), both in this process, alternating, on the same seeded inputs.
Shapes are the registry's (mixtral-8x7b, qwen3-moe, deepseek-v2-lite; softmax
routing for all three, the router is not what differs), T = 512, 2048, 8192,
with uniform random routing and a skewed one: half of every token's k choices
fall on a tenth of the experts.

Time per call as tools/attn_chunk_bench.py takes it: device events around a
window of back-to-back calls that ends in a synchronise, `--samples` windows per
route taken alternately; the table has the median and the (max - min) / median
spread. FLOP/s = 2 * A * 3 * D * I over the median; weight bytes = what either
route must read at least once, 3 * D * I * 2 B per expert that has a row. A
route is called faster when its slowest sample beats the other's fastest.
Prints one markdown table row per case (docs/PERF.md keeps a run)."""
import argparse
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from tools.attn_chunk_bench import window_us
from xotorch_amd import ops
from xotorch_amd.models import moe

MODELS = {"mixtral-8x7b": (8, 2, 4096, 14336), "qwen3-moe": (128, 8, 2048, 768), "deepseek-v2-lite": (64, 6, 2048, 1408)}


def logits_for(T, E, k, skewed, g):
  """fp32 [T, E] whose top-k is decided: uniform = k random experts per token;
  skewed = k / 2 of them among the first round(E / 10) experts."""
  score = torch.rand(T, E, device="cuda", generator=g)
  if skewed:
    hot = max(1, round(E / 10))
    kh = min(k // 2, hot)
    pick = torch.cat([score[:, :hot].topk(kh).indices, hot + score[:, hot:].topk(k - kh).indices], dim=1)
  else:
    pick = score.topk(k).indices
  return torch.randn(T, E, device="cuda", generator=g).scatter_(1, pick, 8.0 + score.gather(1, pick))


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--models", default=",".join(MODELS))
  p.add_argument("--tokens", default="512,2048,8192")
  p.add_argument("--samples", type=int, default=3)
  p.add_argument("--window-ms", type=float, default=40.0)
  args = p.parse_args()
  assert torch.cuda.is_available() and ops.hip_available(), "needs the GPU and the built extension"
  lin = torch.nn.functional.linear
  print("| model | T | routing | live experts | weight MB | sorted per-expert ms (spread) | ragged ms (spread) | "
        "sorted TFLOP/s | ragged TFLOP/s | faster | max abs diff |")
  print("|" + "---|" * 11)
  for name in args.models.split(","):
    E, k, D, I = MODELS[name]
    g = torch.Generator(device="cuda").manual_seed(E + I)
    rnd = lambda *s, std: (std * torch.randn(*s, device="cuda", generator=g)).bfloat16()
    wgu = [rnd(2 * I, D, std=D ** -0.5) for _ in range(E)]
    wd = [rnd(D, I, std=I ** -0.5) for _ in range(E)]
    wp_gu = torch.stack([ops.pack_decode_weight(w) for w in wgu]).contiguous()
    wp_d = torch.stack([ops.pack_decode_weight(w) for w in wd]).contiguous()
    experts = [lambda xe, e=e: lin(ops.swiglu_packed(lin(xe, wgu[e])), wd[e]) for e in range(E)]
    for T in (int(t) for t in args.tokens.split(",")):
      flat = rnd(T, D, std=1.0)
      for skewed in (False, True):
        logits = logits_for(T, E, k, skewed, g)

        def old():
          w, sel = torch.topk(torch.softmax(logits, dim=-1), k, dim=-1)
          return moe.sorted_expert_prefill(flat, w / w.sum(dim=-1, keepdim=True), sel, experts).bfloat16()

        def new():
          sel, w = ops.moe_route(logits, None, k, 0)
          return moe.moe_prefill(flat, sel, w, E, I, wp_gu, wp_d)

        with torch.inference_mode():
          outs, calls, times = [], [], ([], [])
          for f in (old, new):  # warm, and size the window
            for _ in range(3):
              out = f()
            outs.append(out.float())
            calls.append(max(3, int(args.window_ms * 1e3 / window_us(f, 3)) + 1))
          for _ in range(args.samples):
            for i, f in enumerate((old, new)):
              times[i].append(window_us(f, calls[i]) / 1e3)
        live = int((torch.bincount(logits.topk(k).indices.flatten(), minlength=E) > 0).sum())
        med = [statistics.median(t) for t in times]
        flops = 2.0 * T * k * 3 * D * I
        faster = "sorted" if max(times[0]) < min(times[1]) else "ragged" if max(times[1]) < min(times[0]) else "tie"
        cell = lambda i: f"{med[i]:.3f} ({100 * (max(times[i]) - min(times[i])) / med[i]:.0f} %)"
        print(f"| {name} | {T} | {'skewed' if skewed else 'uniform'} | {live} | {live * 3 * D * I * 2 / 1e6:.0f} | "
              f"{cell(0)} | {cell(1)} | {flops / med[0] / 1e9:.0f} | {flops / med[1] / 1e9:.0f} | {faster} | "
              f"{(outs[0] - outs[1]).abs().max().item():.4f} |", flush=True)
    del wgu, wd, wp_gu, wp_d, experts


if __name__ == "__main__":
  main()
