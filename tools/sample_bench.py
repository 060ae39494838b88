"""What the serve tick's sampling costs on a [slots, V] bf16 logits buffer, three
routes alternated: (a) the per-slot ops.softmax_sample loop of
RingSlotWorker._sample_all, (b) one batched torch_ref.softmax_sample call,
(c) torch.rand + one ops.sample launch (XOT_HIP_SAMPLE=1). Then the kernel
alone against one read of the buffer at the measured stream rate.

  python tools/sample_bench.py [--slots 63] [--vocab 128256] [--samples 7] [--iters 20]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from xotorch_amd import ops
from xotorch_amd.ops import torch_ref


def timed(fn, iters):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(iters):
    fn()
  torch.cuda.synchronize()
  return (time.perf_counter() - t0) / iters * 1e6


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--slots", type=int, default=63)
  ap.add_argument("--vocab", type=int, default=128256)
  ap.add_argument("--samples", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  a = ap.parse_args()
  assert torch.cuda.is_available() and ops.hip_available(), "needs the GPU and the HIP extension"
  B, V = a.slots, a.vocab
  gen = torch.Generator(device="cuda").manual_seed(1234)
  logits = (2.0 * torch.randn(B, V, device="cuda", generator=gen)).to(torch.bfloat16)
  temp = torch.full((B,), 0.6, device="cuda")
  top_k = torch.full((B,), 35, dtype=torch.int32, device="cuda")
  u, out = torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda")
  for p in (0.0, 0.9):
    top_p = torch.full((B,), p, device="cuda")

    def loop():
      toks = logits.argmax(dim=-1).clone()
      for i in range(B):
        toks[i] = ops.softmax_sample(logits[i:i + 1], temperature=0.6, top_k=35, top_p=p)[0]
      out.copy_(toks)

    def batched():
      out.copy_(torch_ref.softmax_sample(logits, 0.6, 35, None, p))

    def kernel():
      torch.rand(B, generator=gen, out=u)
      ops.sample(logits, temp, top_k, top_p, u=u, out=out)

    routes = {"(a) per-slot loop": loop, "(b) batched torch": batched, "(c) ops.sample": kernel}
    for fn in routes.values():  # warm up every route
      timed(fn, 2)
    got = {n: [] for n in routes}
    for _ in range(a.samples):
      for n, fn in routes.items():
        got[n].append(timed(fn, a.iters))
    print(f"temp 0.6, top_k 35, top_p {p}: [{B}, {V}] bf16, us per tick's sampling")
    for n, v in got.items():
      print(f"  {n:20s} median {statistics.median(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f}   "
            + " ".join(f"{x:.1f}" for x in v))
    alone = [timed(lambda: ops.sample(logits, temp, top_k, top_p, u=u, out=out), 200) for _ in range(a.samples)]
    print(f"  kernel alone         median {statistics.median(alone):9.1f}  min {min(alone):9.1f}  max {max(alone):9.1f}")
  src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
  dst = torch.empty_like(src)
  rate = statistics.median(2 * src.numel() / timed(lambda: dst.copy_(src), 20) for _ in range(a.samples))  # bytes / us
  print(f"stream rate (256 MiB copy, read + write): {rate / 1e6:.2f} TB/s; one read of the "
        f"{logits.numel() * 2 / 1e6:.1f} MB buffer at that rate: {logits.numel() * 2 / rate:.1f} us")


if __name__ == "__main__":
  main()
