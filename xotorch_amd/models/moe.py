"""What the routed MoE blocks (llama.MoEMLP, deepseek_v3.DsMoE) share after
routing: the static-capacity decode pipeline and the sorted prefill."""
from __future__ import annotations

import torch

from xotorch_amd import ops


def moe_decode(flat, selected, weights, E: int, I: int, experts, wp_gate_up=None, wp_down=None,
               scales=None, mxfp4: bool = False):
  """Static-shape (hipGraph-capturable) routed experts on flat [T, D] with
  expert ids / weights [T, k]: assignments are sorted by expert, every expert
  gets the fixed capacity C (top-k experts are distinct per token, so one
  expert receives at most T assignments: lossless), padded slots weigh 0.
  With stacked packs [E, ...] each expert GEMM is ONE grouped launch, bf16 or
  (scales = (sw_gate_up, sw_down)) fp8, or MXFP4 weight-only (mxfp4: the packs
  are the stacked code images and scales the stacked e8m0 images); without,
  experts[e] runs on its slice.
  Returns [T, D]: bf16 from the HIP combine, fp32 from the torch one."""
  T, D = flat.shape
  C = max(32, -(-T // 32) * 32)
  dev = flat.device
  hip = flat.is_cuda and ops.hip_available()
  if hip:
    # single-launch counting sort + deterministic combine (the argsort/cumsum/
    # index_add torch glue below was the measured top MoE decode cost)
    gather_tok, inv_pos = ops.moe_build(selected.to(torch.int32).contiguous(), E, C)
    gather_tok = gather_tok.long()
  else:
    A = selected.numel()
    expert_of = selected.reshape(A)
    token_of = torch.arange(T, device=dev).repeat_interleave(selected.shape[1])
    order = torch.argsort(expert_of)                        # static shape [A]
    sorted_token = token_of[order]
    sorted_w = weights.reshape(A)[order]
    counts = (expert_of.unsqueeze(0) == torch.arange(E, device=dev).unsqueeze(1)).sum(1)
    offsets = torch.cumsum(counts, 0) - counts              # exclusive prefix
    c_idx = torch.arange(C, device=dev)
    pos_c = (offsets.unsqueeze(1) + c_idx.unsqueeze(0)).clamp(max=A - 1)  # [E, C]
    valid = c_idx.unsqueeze(0) < counts.unsqueeze(1)
    gather_tok = sorted_token[pos_c.reshape(-1)]            # [E*C]
    scale = torch.where(valid, sorted_w[pos_c], torch.zeros((), dtype=sorted_w.dtype, device=dev))
  xg = flat[gather_tok]                                     # [E*C, D]
  if wp_gate_up is None or torch.is_grad_enabled():
    y = torch.cat([experts[e](xe) for e, xe in enumerate(xg.view(E, C, D))], dim=0)
  elif mxfp4:
    gu = ops.skinny_gemm_mxfp4(xg.view(E, C, D), wp_gate_up, scales[0], E, 2 * I)
    h = ops.swiglu_packed(gu.view(E * C, 2 * I))
    y = ops.skinny_gemm_mxfp4(h.view(E, C, I), wp_down, scales[1], E, D)
  elif scales is not None:
    x8, sx = ops.quant_fp8_rows(xg)
    gu = ops.skinny_gemm_fp8(x8, sx, wp_gate_up, scales[0].view(-1), E, 2 * I)
    h8, sh = ops.quant_fp8_rows(ops.swiglu_packed(gu.view(E * C, 2 * I)))
    y = ops.skinny_gemm_fp8(h8, sh, wp_down, scales[1].view(-1), E, D)
  else:
    gu = ops.skinny_gemm_grouped(xg.view(E, C, D), wp_gate_up, E, 2 * I)
    h = ops.swiglu_packed(gu.view(E * C, 2 * I))
    y = ops.skinny_gemm_grouped(h.view(E, C, I), wp_down, E, D)
  y = y.view(E * C, D)
  if hip:
    return ops.moe_combine(y.to(torch.bfloat16).contiguous(), inv_pos, weights.float().contiguous())
  out = torch.zeros(T, D, dtype=torch.float32, device=dev)
  out.index_add_(0, gather_tok, y.float() * scale.reshape(-1, 1))
  return out


def sorted_expert_prefill(flat, weights, selected, experts):
  """Dynamic-shape routed experts for prefill: sort the token-expert pairs
  ONCE and run each expert on a contiguous slice (one argsort + one gather
  instead of E where/eq scans; one host sync for the counts) -> fp32 [T, D]."""
  T, D = flat.shape
  expert_of = selected.reshape(-1)
  order = torch.argsort(expert_of)
  tok_sorted = torch.arange(T, device=flat.device).repeat_interleave(selected.shape[1])[order]
  w_sorted = weights.reshape(-1)[order]
  counts = torch.bincount(expert_of, minlength=len(experts)).cpu().tolist()
  ys = [experts[e](xe) for e, xe in enumerate(torch.split(flat[tok_sorted], counts)) if len(xe)]
  y = torch.cat(ys, dim=0).float() * w_sorted[:, None].float()
  out = torch.zeros(T, D, dtype=torch.float32, device=flat.device)
  out.index_add_(0, tok_sorted, y)
  return out


def expert_loop(flat, weights, selected, experts):
  """The reference's dynamic gather loop (llm_utils.py:502-590), autograd-safe:
  the CPU and training path -> fp32 [T, D]."""
  out = torch.zeros_like(flat, dtype=torch.float32)
  for e, expert in enumerate(experts):
    tok, k_idx = torch.where(selected == e)
    if tok.numel():
      out.index_add_(0, tok, expert(flat[tok]).float() * weights[tok, k_idx, None])
  return out
