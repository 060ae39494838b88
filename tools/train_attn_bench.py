"""Forward plus backward of causal GQA training attention alone: the
ops.attn_train kernel route against torch_ref.attn_train (fp32 sdpa over K / V
expanded per query head, what XOT_TRAIN_ATTN=0 runs) on the same bf16 inputs,
q / k / v being slices of one packed qkv tensor as in the model.

  python tools/train_attn_bench.py

Device events around `iters` forward + backward calls after 3 warm-up calls,
the routes alternating, three samples each, and torch.cuda.max_memory_allocated
above the resident inputs for one call of each route; one JSON line per shape.
A route that runs out of memory is reported as such. Needs a GPU and the built
extension; the figures in docs/PERF.md come from it."""
import json
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from xotorch_amd import ops
from xotorch_amd.ops import torch_ref

SHAPES = ((8, 512, 32, 8, 128), (4, 2048, 32, 8, 128), (8, 2048, 32, 8, 64), (1, 8192, 32, 8, 128))  # (B, S, H, KVH, hd)


def step(route, q, k, v, do):
  out = route(q, k, v)
  return (out,) + torch.autograd.grad(out, (q, k, v), do)


def timed(fn, iters):
  for _ in range(3):
    fn()
  ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
  ev[0].record()
  for _ in range(iters):
    fn()
  ev[1].record()
  torch.cuda.synchronize()
  return round(ev[0].elapsed_time(ev[1]) / iters, 4)


def peak_mib(fn):
  torch.cuda.synchronize()
  torch.cuda.empty_cache()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  fn()
  torch.cuda.synchronize()
  return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def main():
  assert torch.cuda.is_available() and ops.hip_available(), "needs a GPU and the built extension"
  for B, S, H, KVH, hd in SHAPES:
    torch.manual_seed(0)
    qkv = torch.randn(B, S, (H + 2 * KVH) * hd, device="cuda", dtype=torch.bfloat16).requires_grad_(True)
    q, k, v = (x.reshape(B, S, -1, hd) for x in torch.split(qkv, [H * hd, KVH * hd, KVH * hd], dim=-1))
    do = torch.randn(B, S, H, hd, device="cuda", dtype=torch.bfloat16)
    kernel = lambda: step(ops.attn_train, q, k, v, do)
    sdpa = lambda: step(torch_ref.attn_train, q, k, v, do)
    row = {"B": B, "S": S, "H": H, "KVH": KVH, "hd": hd, "kernel_route_ms": [], "sdpa_route_ms": [],
           "kernel_route_peak_mib": peak_mib(kernel)}
    try:
      row["sdpa_route_peak_mib"] = peak_mib(sdpa)
      row["maxdiff_kernel_sdpa"] = [round((a.float() - b.float()).abs().max().item(), 5) for a, b in zip(kernel(), sdpa())]
      iters = max(3, min(50, int(2 ** 26 / (B * S * S))))
      for _ in range(3):  # alternate the routes, keep every sample
        row["sdpa_route_ms"].append(timed(sdpa, iters))
        row["kernel_route_ms"].append(timed(kernel, iters))
    except torch.cuda.OutOfMemoryError:
      row["sdpa_route_ms"] = "out of memory"
      torch.cuda.empty_cache()
      row["kernel_route_ms"] = [timed(kernel, 10) for _ in range(3)]
    print(json.dumps(row), flush=True)
    del qkv, q, k, v, do
    torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
