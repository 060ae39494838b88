"""Forward plus backward of causal MLA training attention alone (nope 128 / rope
64 / v 128): the ops.attn_train_mla kernel route against
torch_ref.attn_train_mla (the explicit fp32 expression, what XOT_TRAIN_ATTN=0
runs) on the same bf16 inputs, kvx being the per-head view of a
[B, S, H * 256] tensor as in the model.

  python tools/train_attn_mla_bench.py

Measured as tools/train_attn_bench.py measures the GQA kernels (its timed and
peak_mib): device events after 3 warm-up calls, the routes alternating, three
samples each; one JSON line per shape. Needs a GPU and the built extension; the
figures in docs/PERF.md come from it."""
import json
import torch
from train_attn_bench import peak_mib, timed
from xotorch_amd import ops
from xotorch_amd.ops import torch_ref

SHAPES = ((8, 512, 16), (4, 2048, 16), (1, 4096, 16), (2, 2048, 128))  # (B, S, H): v2-lite has 16 heads, v3 128
SCALE = 192 ** -0.5


def step(route, q, kvx, rot, do):
  out = route(q, kvx, rot, SCALE)
  return (out,) + torch.autograd.grad(out, (q, kvx, rot), do)


def main():
  assert torch.cuda.is_available() and ops.hip_available(), "needs a GPU and the built extension"
  for B, S, H in SHAPES:
    torch.manual_seed(0)
    q, kvw, rot = (torch.randn(B, S, w, device="cuda", dtype=torch.bfloat16).requires_grad_(True) for w in (H * 192, H * 256, 64))
    q, kvx = q.view(B, S, H, 192), kvw.view(B, S, H, 256)
    do = torch.randn(B, S, H, 128, device="cuda", dtype=torch.bfloat16)
    kernel = lambda: step(ops.attn_train_mla, q, kvx, rot, do)
    ref = lambda: step(torch_ref.attn_train_mla, q, kvx, rot, do)
    row = {"B": B, "S": S, "H": H, "kernel_route_ms": [], "torch_route_ms": [], "kernel_route_peak_mib": peak_mib(kernel)}
    try:
      row["torch_route_peak_mib"] = peak_mib(ref)
      row["maxdiff_kernel_torch"] = [round((a.float() - b.float()).abs().max().item(), 5) for a, b in zip(kernel(), ref())]
      iters = max(3, min(50, int(2 ** 26 / (B * S * S))))
      for _ in range(3):  # alternate the routes, keep every sample
        row["torch_route_ms"].append(timed(ref, iters))
        row["kernel_route_ms"].append(timed(kernel, iters))
    except torch.cuda.OutOfMemoryError:
      row["torch_route_ms"] = "out of memory"
      torch.cuda.empty_cache()
      row["kernel_route_ms"] = [timed(kernel, 10) for _ in range(3)]
    print(json.dumps(row), flush=True)
    del q, kvw, kvx, rot, do
    torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
