"""Attention part of one deepseek-v2-lite layer (H=16, nope 128 / rope 64 /
v 128): the attn_prefill_mla route against the torch route of
MLAttention._prefill_absorbed, from after kv_b_proj to before o_proj.

  python tools/mla_prefill_bench.py

Device events around 10 (torch) or 100 (kernel) calls after 3 warm-up calls,
the routes alternating, three samples each; one JSON line per shape. Needs a
GPU and the built extension; the figures in docs/PERF.md come from it."""
import json
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
from xotorch_amd import ops

H, NOPE, ROPE, VD = 16, 128, 64, 128
SCALE = (NOPE + ROPE) ** -0.5
SHAPES = ((64, 512, 0), (8, 4096, 0), (64, 512, 1536))  # (B, S, start_pos)


def torch_route(q_pass, q_rot, kvx, rot_c, start_pos, S):
  """The lines of _prefill_absorbed that XOT_MLA_PREFILL=0 runs."""
  B, total = kvx.shape[0], start_pos + S
  rot = rot_c[:, 0, :total]
  k = torch.cat([kvx[..., :NOPE], rot[:, :, None, :].expand(B, total, H, -1)], dim=-1)
  k = k.permute(0, 2, 1, 3)
  v = kvx[..., NOPE:].permute(0, 2, 1, 3)
  q = torch.cat([q_pass, q_rot], dim=-1).permute(0, 2, 1, 3)
  outs = []
  for s0 in range(0, S, 128):
    qc = q[:, :, s0:s0 + 128]
    t_end = start_pos + s0 + qc.shape[2]
    sc = torch.matmul(qc, k[:, :, :t_end].transpose(-1, -2)).float() * SCALE
    qi = torch.arange(start_pos + s0, t_end, device="cuda")
    sc.masked_fill_(qi[:, None] < torch.arange(t_end, device="cuda")[None, :], float("-inf"))
    outs.append(torch.matmul(sc.softmax(-1).to(torch.bfloat16), v[:, :, :t_end]))
  return torch.cat(outs, dim=2).permute(0, 2, 1, 3).reshape(B, S, H * VD)


def kernel_route(q_pass, q_rot, kvx, rot_c, start_pos, S):
  q = torch.cat([q_pass, q_rot], dim=-1)
  return ops.attn_prefill_mla(q, kvx, rot_c, start_pos, SCALE).view(kvx.shape[0], S, H * VD)


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


def main():
  assert torch.cuda.is_available() and ops.hip_available(), "needs a GPU and the built extension"
  for B, S, sp in SHAPES:
    T = sp + S
    torch.manual_seed(0)
    qfull = torch.randn(B, S, H, NOPE + ROPE, device="cuda", dtype=torch.bfloat16)
    q_pass, q_rot = qfull[..., :NOPE], qfull[..., NOPE:].contiguous()
    kvx = (torch.randn(B, T, H * (NOPE + VD), device="cuda", dtype=torch.bfloat16) * 0.7).view(B, T, H, NOPE + VD)
    rot_c = torch.randn(B, 1, T + 64, ROPE, device="cuda", dtype=torch.bfloat16)
    args = (q_pass, q_rot, kvx, rot_c, sp, S)
    diff = (kernel_route(*args).float() - torch_route(*args).float()).abs().max().item()
    row = {"B": B, "S": S, "start_pos": sp, "maxdiff_kernel_torch": diff,
           "torch_route_ms": [], "kernel_route_ms": [], "kernel_only_ms": []}
    for _ in range(3):  # alternate the versions, keep every sample
      row["torch_route_ms"].append(timed(lambda: torch_route(*args), 10))
      row["kernel_route_ms"].append(timed(lambda: kernel_route(*args), 100))
      row["kernel_only_ms"].append(timed(lambda: ops.attn_prefill_mla(qfull, kvx, rot_c, sp, SCALE), 100))
    print(json.dumps(row), flush=True)
    del qfull, q_pass, q_rot, kvx, rot_c, args
    torch.cuda.empty_cache()


if __name__ == "__main__":
  main()
