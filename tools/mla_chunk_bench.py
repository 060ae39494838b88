#!/usr/bin/env python3
"""A short DeepSeek (MLA) chunk behind a long latent cache, per layer and
without o_proj, which both routes share: today's route (rope q, expand the live
cache through kv_b_proj, attn_prefill_mla) against the absorbed route (q_lat
einsum, mla_q_prep, attn_chunk_mla and its merge, out einsum), both in this
process, alternating, on the same seeded inputs; then the absorbed route under
XOT_MLA_CHUNK_NSPLIT = 1 .. 64 at B = 1 (--sweep).

Time per call as tools/attn_chunk_bench.py takes it: device events around a
window of back-to-back calls, median of --samples windows taken alternately.
Back-to-back calls on one cache are warm-cache figures for both routes.
Prints one markdown table row per shape (docs/PERF.md keeps a run)."""
import argparse
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch

from tools.attn_chunk_bench import measure
from xotorch_amd import ops
from xotorch_amd.models.deepseek_v3 import _rope

NOPE, ROPE, VD, LAT = 128, 64, 128, 512
SCALE = (NOPE + ROPE) ** -0.5


def routes(B, H, S, start, cap):
  g = torch.Generator(device="cuda").manual_seed(start + S + H)
  rnd = lambda *s, std=1.0: (std * torch.randn(*s, device="cuda", generator=g)).bfloat16()
  q = rnd(B, S, H, NOPE + ROPE)
  W = rnd(H * (NOPE + VD), LAT, std=LAT ** -0.5)
  lat_c, rot_c = rnd(B, 1, cap, LAT), rnd(B, 1, cap, ROPE)
  kp, vp = torch.empty(B, cap // 16, 18, 64, 8, device="cuda", dtype=torch.bfloat16), \
    torch.empty(B, 32, cap // 32, 64, 8, device="cuda", dtype=torch.bfloat16)
  ops._gpu().mla_append(lat_c[:, 0].contiguous(), rot_c[:, 0].contiguous(),
                        torch.arange(cap, dtype=torch.int32, device="cuda"), kp, vp)
  pos = torch.arange(start, start + S, dtype=torch.int32, device="cuda")
  ang = pos.float()[:, None] * (10000.0 ** (-torch.arange(0, ROPE, 2, device="cuda").float() / ROPE))[None, :]
  cos_t, sin_t = torch.zeros(cap, ROPE // 2, device="cuda"), torch.zeros(cap, ROPE // 2, device="cuda")
  cos_t[start:start + S], sin_t[start:start + S] = ang.cos(), ang.sin()
  Wh = W.view(H, NOPE + VD, LAT)
  w_k, w_v = Wh[:, :NOPE].contiguous(), Wh[:, NOPE:].contiguous()
  total = start + S

  def expand():
    q_rot = _rope(q[..., NOPE:], cos_t[pos.long()], sin_t[pos.long()], True)
    kvx = torch.nn.functional.linear(lat_c[:, 0, :total], W).view(B, total, H, NOPE + VD)
    return ops.attn_prefill_mla(torch.cat([q[..., :NOPE], q_rot], dim=-1), kvx, rot_c, start, SCALE)

  def absorbed():
    q_lat = torch.einsum("bshn,hnl->bshl", q[..., :NOPE], w_k)
    qf = ops.mla_q_prep(q, q_lat.contiguous(), cos_t, sin_t, pos, NOPE, True, False)[0].view(B, S, H, -1)
    out_lat = ops.attn_chunk_mla(qf, kp, vp, start, SCALE)
    return torch.einsum("bshl,hdl->bshd", out_lat, w_v)

  return expand, absorbed


def main():
  p = argparse.ArgumentParser()
  p.add_argument("--calls", type=int, default=5)
  p.add_argument("--samples", type=int, default=5)
  p.add_argument("--window-ms", type=float, default=30.0)
  p.add_argument("--capacity", type=int, default=32768, help="positions of the preallocated latent cache")
  p.add_argument("--sweep", action="store_true", help="also sweep XOT_MLA_CHUNK_NSPLIT at B = 1")
  args = p.parse_args()
  assert torch.cuda.is_available() and ops.hip_available(), "needs the GPU and the built extension"
  os.environ.pop("XOT_MLA_CHUNK_NSPLIT", None)
  S, cap = 5, args.capacity
  print("| H | S | B | start_pos | nsplit | kv_b expansion + attn_prefill_mla us | absorbed chunk route us | ratio | max abs diff |")
  print("|---|---|---|---|---|---|---|---|---|")
  for H in (16, 128):
    for B in (1, 8):
      for start in (512, 4096, 16384):
        expand, absorbed = routes(B, H, S, start, cap)
        both = lambda: (expand if os.environ["MLA_BENCH_ROUTE"] == "0" else absorbed)()
        (t_old, t_new), (o_old, o_new) = measure(both, [{"MLA_BENCH_ROUTE": "0"}, {"MLA_BENCH_ROUTE": "1"}],
                                                 args.calls, args.samples, args.window_ms)
        print(f"| {H} | {S} | {B} | {start} | {ops._gpu().attn_chunk_mla_nsplit(B, H, S, cap)} | {t_old:.1f} | {t_new:.1f} | "
              f"{t_old / t_new:.2f}x | {(o_old - o_new).abs().max().item():.4f} |", flush=True)
        del expand, absorbed, both
  if args.sweep:
    ns = (1, 2, 4, 8, 16, 32, 64)
    print(f"\ncapacity {cap}, B = 1, S = {S}\n\n| H | start_pos | rule | " + " | ".join(f"nsplit {n} us" for n in ns) + " |")
    print("|" + "---|" * (3 + len(ns)))
    for H in (16, 128):
      for start in (512, 4096, 16384):
        _, absorbed = routes(1, H, S, start, cap)
        os.environ.pop("XOT_MLA_CHUNK_NSPLIT", None)
        rule = ops._gpu().attn_chunk_mla_nsplit(1, H, S, cap)
        ts, _ = measure(absorbed, [{"XOT_MLA_CHUNK_NSPLIT": str(n)} for n in ns], args.calls, args.samples, args.window_ms)
        print(f"| {H} | {start} | {rule} | " + " | ".join(f"{t:.1f}" for t in ts) + " |", flush=True)
    os.environ.pop("XOT_MLA_CHUNK_NSPLIT", None)


if __name__ == "__main__":
  main()
