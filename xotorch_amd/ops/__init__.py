"""Op dispatch: hand-written CDNA4 HIP kernels on GPU, torch reference on CPU.

The HIP extension (`xotorch_amd.ops.hip`, built in-tree by
`xotorch_amd/ops/build.py` / `__graft_entry__.build()`) owns the per-token
hot path on MI355X. On a GPU box the HIP path is MANDATORY: if a CUDA tensor
reaches an op and the extension is missing, we raise rather than silently
falling back to eager PyTorch (set XOT_ALLOW_EAGER=1 to override for
debugging/ablation only).
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from xotorch_amd.ops import torch_ref

_hip = None
_hip_load_error: Optional[Exception] = None


def _load_hip():
  global _hip, _hip_load_error
  if _hip is not None or _hip_load_error is not None:
    return _hip
  try:
    import importlib
    _hip = importlib.import_module("xotorch_amd.ops._hip_ops")
  except Exception as e:  # extension not built
    _hip_load_error = e
    _hip = None
  return _hip


def hip_available() -> bool:
  return _load_hip() is not None


def _use_hip(*tensors: torch.Tensor) -> bool:
  t = tensors[0]
  if not t.is_cuda:
    return False
  if torch.is_grad_enabled() and any(x.requires_grad for x in tensors):
    # training path: HIP kernels are inference-only (no autograd); the torch
    # ops are differentiable. Inference runs on the HIP kernels.
    return False
  if _load_hip() is not None:
    return True
  if os.getenv("XOT_ALLOW_EAGER", "0") == "1":
    return False
  raise RuntimeError(
    "xotorch_amd HIP extension is not built but a CUDA tensor reached the op "
    f"dispatch (load error: {_hip_load_error}). Build it with "
    "`python -c \"import __graft_entry__; __graft_entry__.build()\"` or set "
    "XOT_ALLOW_EAGER=1 to explicitly allow the eager fallback."
  )


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float, w_bias: float = 0.0) -> torch.Tensor:
  """w_bias=1.0 gives the gemma convention (scale by 1 + w, fp32 math)."""
  if _use_hip(x, weight) and x.dtype == torch.bfloat16:
    return _hip.rmsnorm(x, weight, eps, w_bias)
  return torch_ref.rmsnorm(x, weight, eps, w_bias)


def rmsnorm_residual(
  x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float,
  w_bias: float = 0.0
) -> Tuple[torch.Tensor, torch.Tensor]:
  if _use_hip(x, residual, weight) and x.dtype == torch.bfloat16:
    return _hip.rmsnorm_residual(x, residual, weight, eps, w_bias)
  return torch_ref.rmsnorm_residual(x, residual, weight, eps, w_bias)


def add_rmsnorm(
  y: torch.Tensor, residual: torch.Tensor, weight: Optional[torch.Tensor], eps: float,
  w_bias: float = 0.0
) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
  """(h' = y + residual, rmsnorm(h')) in one launch — the layer's closing
  residual add fused with the norm that follows it; the norm reads the
  rounded h'. weight=None gives (h', None)."""
  tensors = (y, residual) if weight is None else (y, residual, weight)
  if _use_hip(*tensors) and y.dtype == torch.bfloat16:
    out = _hip.add_rmsnorm(y.contiguous(), residual.contiguous(), weight, eps, w_bias)
    return out[0], (out[1] if weight is not None else None)
  return torch_ref.add_rmsnorm(y, residual, weight, eps, w_bias)


def fuse_epilogue_enabled() -> bool:
  """XOT_FUSE_EPILOGUE (default 1, read per call): carry the next layer's
  input norm in the down-projection's row epilogue; 0 keeps the separate
  combine, add and norm launches."""
  return os.getenv("XOT_FUSE_EPILOGUE", "1") != "0"


def mfma_attn_enabled() -> bool:
  """XOT_MFMA_ATTN (default 1, read per call): fragment-packed KV cache
  copies and the MFMA attention kernels that stream them."""
  return os.getenv("XOT_MFMA_ATTN", "1") == "1"


# head dims the fragment-packed GQA cache copies, the fused append into them
# and the MFMA attention kernels are built for (hip_ops.hip GQA_PACKED_HD)
PACKED_HEAD_DIMS = (128, 256)


def gqa_packed_kv(head_dim: int, dtype: torch.dtype) -> bool:
  """Whether a GPU GQA cache of this head dim and dtype carries the packed
  second copies of K and V, which double its residency."""
  return head_dim in PACKED_HEAD_DIMS and dtype == torch.bfloat16 and mfma_attn_enabled()


def _need_plain_cache(op: str, k_cache, why: str):
  """A packed-only KV cache (ShardKVCache(plain=False)) has no [B, KVH, T, hd]
  tensors: a route that reads them is an error, never a silent fallback."""
  if k_cache is None:
    raise RuntimeError(
      f"{op}: this call needs the plain KV cache, but the cache was built without it "
      f"(plain=False): {why}. Build the cache with plain=True (XOT_KV_PLAIN=1 on the ring path).")


def rope_apply(q, k, cos, sin, positions):
  """Standalone RoPE (training / oracle paths). On the GPU inference hot
  path RoPE is fused into rope_qkv_append — there is deliberately no
  separate HIP kernel for this op."""
  return torch_ref.rope_apply(q, k, cos, sin, positions)


def rope_qkv_append(qkv, cos, sin, positions, k_cache, v_cache, n_heads: int, n_kv_heads: int,
                    head_dim: int, kp=None, vp=None, q_norm=None, k_norm=None,
                    norm_eps: float = 1e-6, k_scale=None, v_scale=None):
  """Fused on the packed qkv GEMM output [B,S,(H+2KVH)*hd]: (optionally
  per-head-RMSNorm q/k — qwen3), RoPE-rotate the q heads in place, rotate k
  heads into the cache, copy v heads into the cache. When the MFMA-packed
  cache copies (kp, vp) exist they are appended too.
  """
  if _use_hip(qkv) and qkv.dtype == torch.bfloat16:
    # k_cache / v_cache None: a packed-only cache, the kernel skips the plain stores
    _hip.rope_qkv_append(qkv, cos, sin, positions, k_cache, v_cache, n_heads, n_kv_heads, head_dim,
                         kp, vp, q_norm, k_norm, norm_eps, k_scale, v_scale)
    return
  _need_plain_cache("rope_qkv_append", k_cache, "the torch path appends to the plain cache")
  torch_ref.rope_qkv_append(qkv, cos, sin, positions, k_cache, v_cache, n_heads, n_kv_heads,
                            head_dim, q_norm, k_norm, norm_eps)


def attn_prefill(q, k_cache, v_cache, start_pos: int, s_len: int, kp=None, vp=None,
                 scale=None, softcap: float = 0.0, window: int = 0):
  if q.is_cuda and q.dtype == torch.bfloat16 and kp is not None and q.shape[3] in PACKED_HEAD_DIMS \
     and kp.dtype == torch.bfloat16 and mfma_attn_enabled() and _use_hip(q):
    # causal flash-forward on matrix cores, streaming the MFMA-packed cache;
    # softcap/window run gemma2 semantics inside the same kernel (fp8-KV
    # mode keeps prefill on the plain bf16 cache via the sdpa path below)
    return _hip.attn_prefill_mfma(q, kp, vp, start_pos, scale or 0.0, softcap, window)
  _need_plain_cache("attn_prefill", k_cache,
                    "only the MFMA prefill kernel (XOT_MFMA_ATTN=1, bf16 packed copies, head_dim 128 or 256) "
                    "reads the packed copies")
  if q.is_cuda and not softcap and not window:
    # fallback: sdpa (rocm flash/mem-efficient backends) in model dtype with
    # native GQA — hd outside PACKED_HEAD_DIMS or unpacked-cache path
    import torch.nn.functional as F
    B, S, H, hd = q.shape
    total = start_pos + s_len
    qh = q.transpose(1, 2)
    k = k_cache[:, :, :total]
    v = v_cache[:, :, :total]
    if start_pos == 0:
      out = F.scaled_dot_product_attention(qh, k, v, is_causal=True, enable_gqa=True, scale=scale)
    else:
      mask = torch.ones(S, total, dtype=torch.bool, device=q.device).tril(diagonal=start_pos)
      out = F.scaled_dot_product_attention(qh, k, v, attn_mask=mask, enable_gqa=True, scale=scale)
    return out.transpose(1, 2).contiguous()
  return torch_ref.attn_prefill(q, k_cache, v_cache, start_pos, s_len, scale, softcap, window)


def attn_decode(q, k_cache, v_cache, seq_len, kp=None, vp=None,
                scale=None, softcap: float = 0.0, window: int = 0,
                k_scale=None, v_scale=None):
  """seq_len: int or int32 device tensor [B] (per-sequence lengths).
  With MFMA-packed cache copies (kp, vp) the flash-decoding kernel scores on
  matrix cores (v_mfma_f32_16x16x32_bf16, coalesced 1 KB cache streams).
  softcap/window select gemma2 semantics (MFMA or torch_ref path only)."""
  if _use_hip(q) and q.dtype == torch.bfloat16:
    if not isinstance(seq_len, torch.Tensor):
      seq_len = torch.full((q.shape[0],), int(seq_len), dtype=torch.int32, device=q.device)
    # a packed-only cache (k_cache None): kv heads and capacity from kp [B, KVH, T32/16, ..]
    kvh, cap = (k_cache.shape[1], k_cache.shape[2]) if k_cache is not None else (kp.shape[1], kp.shape[2] * 16)
    rep = q.shape[2] // kvh
    if kp is not None and rep <= 16 and mfma_attn_enabled():
      return _hip.attn_decode_mfma(q, kp, vp, seq_len, cap,
                                   scale or 0.0, softcap, window, k_scale, v_scale)
    _need_plain_cache("attn_decode", k_cache,
                      "only the MFMA decode kernel (XOT_MFMA_ATTN=1, at most 16 query heads per kv head) "
                      "reads the packed copies")
    if not softcap and not window and scale is None:
      return _hip.attn_decode(q, k_cache, v_cache, seq_len)
  _need_plain_cache("attn_decode", k_cache, "the torch path reads the plain cache")
  return torch_ref.attn_decode(q, k_cache, v_cache, seq_len, scale, softcap, window)


def swiglu(gate, up):
  if _use_hip(gate, up) and gate.dtype == torch.bfloat16:
    return _hip.swiglu(gate, up)
  return torch_ref.swiglu(gate, up)


def swiglu_packed(gu):
  """silu(gate)*up on the packed [.., 2I] fused gate_up GEMM output."""
  if _use_hip(gu) and gu.dtype == torch.bfloat16:
    return _hip.swiglu_packed(gu)
  return torch_ref.swiglu_packed(gu)


def geglu_packed(gu):
  """gelu_tanh(gate)*up on the packed [.., 2I] fused gate_up output (gemma2)."""
  if _use_hip(gu) and gu.dtype == torch.bfloat16:
    return _hip.geglu_packed(gu)
  return torch_ref.geglu_packed(gu)


# ---- GPU-only bindings: the decode GEMMs on prepacked weights (x [.., K]
# bf16, 32..256 rows in multiples of 32; wp from pack_decode_weight[_fp8]) and
# the MoE and MLA decode launches. No torch twin: models/linear.py, models/moe.py
# and models/deepseek_v3.py decide when they run, and a missing extension is an error.

def _gpu():
  if _load_hip() is None:
    raise RuntimeError(f"xotorch_amd HIP extension is not built (load error: {_hip_load_error})")
  return _hip


def _binding(name: str):
  return lambda *args: getattr(_gpu(), name)(*args)


skinny_gemm_packed = _binding("skinny_gemm_packed")                # (x, wp, N, bias) -> [.., N]
skinny_gemm_packed_xreg = _binding("skinny_gemm_packed_xreg")      # the same, x held in registers
# (x, wp from pack_decode_weight_glu, N = 2I) -> silu(gate) * up [.., I]: SwiGLU in the store, never split-K
skinny_gemm_packed_glu = _binding("skinny_gemm_packed_glu")
skinny_plan_nsplit = _binding("skinny_plan_nsplit")  # (N, K) -> K splits of the packed kernel's ordinary plan
skinny_gemm_packed_swiglu = _binding("skinny_gemm_packed_swiglu")  # (gu [.., 2I], wp, N, bias): swiglu + GEMM
skinny_gemm_grouped = _binding("skinny_gemm_grouped")  # (x [E, C, K], stacked wp, E, N) -> [E, C, N]
quant_fp8_rows = _binding("quant_fp8_rows")            # (x [M, K]) -> (e4m3 bytes [M, K], fp32 row scales [M])
skinny_gemm_fp8 = _binding("skinny_gemm_fp8")          # (x8, sx, wp8, sw, E, N[, bias]): W8A8, grouped when E > 1
# (x, wq, ws, E, N[, bias]): W4A16 on the MXFP4 images of pack_decode_weight_mxfp4, grouped when E > 1
skinny_gemm_mxfp4 = _binding("skinny_gemm_mxfp4")
# (fp32 logits [T, E], bias | None, k, mode[, n_group, topk_group, routed_scale, norm_topk]) -> (ids [T, k]
# int32, weights [T, k] fp32); mode 0 softmax-topk-renorm, mode 1 sigmoid + group-limited top-k
moe_route = _binding("moe_route")
moe_build = _binding("moe_build")      # (ids int32 [T, k], E, C): counting sort -> (gather_tok [E*C], inv_pos [T, k])
moe_combine = _binding("moe_combine")  # (y [E*C, D], inv_pos, weights fp32) -> [T, D] bf16, deterministic
# MLA (models/deepseek_v3.py) on the latent cache's packed copies (kp, vp; e4m3 with k_scale in fp8-KV mode)
# (ckv, latent norm w, cos, sin, int32 positions, lat_c, rot_c, kp, vp, eps, interleave, k_scale | None): norm + rope + append
mla_prep_append = _binding("mla_prep_append")
# (q [B,S,H,qk], q_lat, cos, sin, int32 positions, nope, interleave, fp8) -> (q [B,H,576][, per-head scales when fp8])
mla_q_prep = _binding("mla_q_prep")
attn_decode_mla = _binding("attn_decode_mla")  # (q, kp, vp, seq_lens, scale, q_scale | None, k_scale | None) -> [B, H, lat]


def _packed_epilogue(fn, x, wp, N, bias, epilogue):
  """Packed decode GEMM `fn` with its row epilogue (residual, norm_weight |
  None, eps) -> (h' = y + residual, rmsnorm(h') | None)."""
  res, w, eps = epilogue
  out = fn(x, wp, N, bias, res.contiguous(), w, eps, 0.0)
  return out[0], (out[1] if w is not None else None)


def skinny_gemm_packed_epilogue(x, wp, N: int, bias, epilogue):
  return _packed_epilogue(_gpu().skinny_gemm_packed_epilogue, x, wp, N, bias, epilogue)


def skinny_gemm_packed_swiglu_epilogue(gu, wp, N: int, bias, epilogue):
  return _packed_epilogue(_gpu().skinny_gemm_packed_swiglu_epilogue, gu, wp, N, bias, epilogue)


def skinny_gemm_mxfp4_epilogue(x, wq, ws, N: int, bias, epilogue):
  fn = lambda x, wq, *rest: _gpu().skinny_gemm_mxfp4_epilogue(x, wq, ws, *rest)
  return _packed_epilogue(fn, x, wq, N, bias, epilogue)


def pack_decode_weight(w: torch.Tensor) -> torch.Tensor:
  """Pre-shuffle a [N, K] bf16 weight into MFMA A-fragment order for the
  packed skinny decode GEMM: [N/32, K/16, 64 lanes, 8 bf16] with lane =
  (k-half)*32 + n-row. One-time at weight load; coalesced 1 KB wave streams
  at decode."""
  N, K = w.shape
  assert N % 32 == 0 and K % 64 == 0, (N, K)
  return w.view(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()


def glu_store_enabled() -> bool:
  """XOT_GLU_STORE (default 1, read at pack time): dense llama gate_up
  projections get the GLU-interleaved pack and run SwiGLU in the GEMM's store;
  0 keeps the plain pack and the separate swiglu_packed launch."""
  return os.getenv("XOT_GLU_STORE", "1") != "0"


def glu_interleave_perm(I: int) -> torch.Tensor:
  """Row order of the GLU-interleaved pack of a fused [gate; up] weight
  [2I, K] (gate rows 0..I-1, up rows I..2I-1): perm[r] = the weight row that
  packed row r holds. With n32 = r // 32, p = (r % 32) // 16, w = r % 16 and
  c = 16 * n32 + 8 * p + w % 8, row r is gate row c when w < 8, else up row c
  (= row I + c). In the 32x32 MFMA D layout a lane owns rows w and w + 8 of
  each 16-row half of a tile, so it holds both halves of its SwiGLU pairs."""
  assert I % 64 == 0, I  # 2I % 128 == 0, the packed kernel's rule
  r = torch.arange(2 * I)
  w = r % 16
  c = 16 * (r // 32) + 8 * ((r % 32) // 16) + w % 8
  return torch.where(w < 8, c, I + c)


def pack_decode_weight_glu(w: torch.Tensor) -> torch.Tensor:
  """pack_decode_weight(w[glu_interleave_perm(I)]) of a fused [gate; up]
  weight [2I, K], for skinny_gemm_packed_glu. One strided copy, without the
  row-gathered temporary: the permutation is a transpose of the row index
  read as [half, n32, p, w % 8] into [n32, p, half, w % 8]."""
  N, K = w.shape
  I = N // 2
  assert N % 128 == 0 and K % 64 == 0, (N, K)
  v = w.view(2, I // 16, 2, 8, K // 16, 2, 8)  # [half, n32, p, w8, k16, k-half, 8]
  return v.permute(1, 4, 5, 2, 0, 3, 6).reshape(N // 32, K // 16, 2, 32, 8).contiguous()


def pack_decode_weight_fp8(w: torch.Tensor):
  """Quantize a [N, K] weight to OCP e4m3 with per-output-channel scales and
  pre-shuffle into the MFMA fragment order (bytes): returns (packed_uint8,
  s_w fp32 [N]). Half the stream bytes of the bf16 prepack — the W8A8 decode
  GEMM path (XOT_FP8_GEMM=1)."""
  N, K = w.shape
  assert N % 32 == 0 and K % 64 == 0, (N, K)
  s_w = (w.float().abs().amax(dim=1).clamp(min=1e-12) / 448.0)
  w8 = (w.float() / s_w[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
  packed = w8.view(torch.uint8).view(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()
  return packed, s_w.contiguous()


def fp8_gemm_enabled() -> bool:
  return os.getenv("XOT_FP8_GEMM", "0") == "1"


# ---- MXFP4 (OCP microscaling): e2m1 elements, one e8m0 scale per 32 along K.
# A code is one nibble: bit 3 the sign, bits 2:0 the index into MXFP4_GRID.
MXFP4_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MXFP4_BLOCK = 32


def w4_gemm_enabled() -> bool:
  """XOT_W4_GEMM (default 0): MXFP4 weight-only (W4A16) decode GEMMs."""
  return os.getenv("XOT_W4_GEMM", "0") == "1"


def decode_weight_format() -> str:
  """The packed decode weight format the environment asks for: "bf16", "fp8"
  (XOT_FP8_GEMM=1) or "mxfp4" (XOT_W4_GEMM=1); both knobs together are an error."""
  if fp8_gemm_enabled() and w4_gemm_enabled():
    raise RuntimeError("XOT_FP8_GEMM=1 and XOT_W4_GEMM=1 are exclusive: choose one decode weight format")
  return "fp8" if fp8_gemm_enabled() else "mxfp4" if w4_gemm_enabled() else "bf16"


def quant_mxfp4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
  """[N, K] -> (codes uint8 [N, K], one per byte, e8 uint8 [N, K/32]). Per
  32-block the OCP rule: e = floor(log2(amax)) - 2 clamped to [-125, 125]
  (every dequantized value a normal bf16, the scale a normal fp32), stored as
  e + 127; elements are w / 2^e rounded to the nearest grid value, ties to
  the even code, saturating at +-6. An all-zero block stores 127."""
  N, K = w.shape
  assert N % 32 == 0 and K % 64 == 0, (N, K)
  wb = w.detach().float().view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
  amax = wb.abs().amax(dim=-1)
  _, ex = torch.frexp(amax)  # amax = m * 2^ex with m in [0.5, 1): floor(log2) = ex - 1
  e = torch.where(amax > 0, ex - 3, torch.zeros_like(ex)).clamp(-125, 125)
  a = torch.ldexp(wb.abs(), -e.unsqueeze(-1))  # exact: a power-of-two scale
  # one threshold per midpoint; a tie goes up only where the upper code is even
  idx = ((a > 0.25).to(torch.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75)
         + (a > 2.5) + (a >= 3.5) + (a > 5.0))
  codes = idx | (torch.signbit(wb).to(torch.uint8) << 3)
  return codes.view(N, K).contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequant_mxfp4(codes: torch.Tensor, e8: torch.Tensor) -> torch.Tensor:
  """The definition: fp32 [N, K] = (-1)^bit3 * MXFP4_GRID[bits 2:0] * 2^(e8 - 127)."""
  N, K = codes.shape
  grid = torch.tensor(MXFP4_GRID, dtype=torch.float32, device=codes.device)
  mag = grid[(codes & 7).long()]
  val = torch.where((codes & 8) != 0, -mag, mag).view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
  return torch.ldexp(val, (e8.to(torch.int32) - 127).unsqueeze(-1)).view(N, K)


def pack_decode_weight_mxfp4(w: torch.Tensor):
  """Quantize a [N, K] weight to MXFP4 and shuffle it into the two images the
  W4A16 decode GEMM streams (stated once beside skinny_gemm_packed_kernel):
  wq uint8 [N/32, K/64, 64 lanes, 16 B] (lane = (k-half)*32 + n-row; dword u
  = the lane's 8 codes of k16-chunk u, lower k in the lower nibble) and ws
  uint8 [N/32, K/64, 32 rows, 2] (the two e8m0 scales of that 64-k step).
  Returns (wq, ws, w_dq): w_dq = the dequantized weight in bf16, exact.
  17/32 byte per weight against 2 for the bf16 prepack (XOT_W4_GEMM=1)."""
  N, K = w.shape
  rows = 4096  # both images are row-tile major: bound the fp32 temporaries of a large weight
  if N > rows:
    parts = [pack_decode_weight_mxfp4(w[r:r + rows]) for r in range(0, N, rows)]
    return tuple(torch.cat(p) for p in zip(*parts))
  codes, e8 = quant_mxfp4(w)
  w_dq = dequant_mxfp4(codes, e8).to(torch.bfloat16)
  nib = (codes[:, 0::2] | (codes[:, 1::2] << 4)).view(N // 32, 32, K // 64, 4, 2, 4)  # [.., u, k-half, byte]
  wq = nib.permute(0, 2, 4, 1, 3, 5).reshape(N // 32, K // 64, 64, 16).contiguous()
  ws = e8.view(N // 32, 32, K // 64, 2).permute(0, 2, 1, 3).contiguous()
  return wq, ws, w_dq


def unpack_decode_weight_mxfp4(wq: torch.Tensor, ws: torch.Tensor, N: int, K: int):
  """Inverse of the pack: (wq, ws) -> (codes [N, K], e8 [N, K/32])."""
  nib = wq.view(N // 32, K // 64, 2, 32, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(N, K // 2)
  codes = torch.stack([nib & 15, nib >> 4], dim=-1).view(N, K)
  e8 = ws.view(N // 32, K // 64, 32, 2).permute(0, 2, 1, 3).reshape(N, K // 32)
  return codes.contiguous(), e8.contiguous()


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
  """y = x @ weight^T (+bias) on hipBLASLt/aten.

  The decode hot path uses XotLinear.pack_decode() + skinny_gemm_packed (the
  hand-written CDNA4 weight-streaming MFMA kernel) instead; this is the
  library-GEMM path for prefill/training/CPU and unpacked weights.
  """
  return torch.nn.functional.linear(x, weight, bias)


def softmax_sample(logits, temperature: float = 0.0, top_k: int = 0, generator=None,
                   top_p: float = 0.0):
  # torch ops here are graph-capturable (argmax / exponential+argmax)
  return torch_ref.softmax_sample(logits, temperature, top_k, generator, top_p)
