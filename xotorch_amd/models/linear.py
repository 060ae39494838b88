"""Decode GEMM routing: which kernel a decode-shaped projection runs.

`decode_rows` says whether an activation is decode-shaped; `auto_pick` races
the hand-written kernels (reached through `xotorch_amd.ops`) against their
baseline on first use and caches the winner; `XotLinear` walks its arms in
order. `llama.MLP` takes its fused-SwiGLU route through the same two helpers.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from xotorch_amd import ops

# key -> the route that won when timed in-situ (first eligible call, before
# hipGraph capture); seed it to force a route. (N, K, M) -> "packed" | "xreg" |
# "blaslt" for a GEMM, ("w4", N, K, M) -> "mxfp4" | "blaslt" for one in MXFP4
# mode, ("fuse_swiglu", N, I, M) -> "fused" | "split" for the MLP. For a gate_up
# with the GLU-interleaved pack, llama.MLP races under the GEMM's (N, K, M):
# "packed" is the GEMM with SwiGLU in its store, "blaslt" the library + swiglu.
DECODE_PICKS: dict = {}


def decode_rows(x: torch.Tensor, K: int) -> int:
  """Row count M of x [.., K] when it is a decode shape for the hand-written
  GEMMs (GPU bf16 inference, contiguous, 32..256 rows in multiples of 32,
  extension loaded), else 0."""
  if not (x.is_cuda and x.dtype == torch.bfloat16 and not torch.is_grad_enabled()
          and x.is_contiguous()):
    return 0
  M = x.numel() // K
  return M if 32 <= M <= 256 and M % 32 == 0 and ops.hip_available() else 0


def _time_us(fn, reps=4, rounds=3) -> float:
  """Min-of-rounds timing (DVFS / first-call noise makes a single round flip
  borderline auto-picks between runs)."""
  fn()  # warm
  best = float("inf")
  for _ in range(rounds):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
      fn()
    end.record()
    end.synchronize()
    best = min(best, start.elapsed_time(end) * 1000.0 / reps)
  return best


def auto_pick(key, what: str, dims: str, margin: float, contenders) -> str:
  """The cached route for `key`, raced on first use. contenders() gives
  [(name, fn), ...]: the baseline, then the challengers in trial order. The
  baseline's time counts times `margin` (a challenger must win clearly: real
  wins measure 20%+ and borderline shapes would flip run-to-run with DVFS),
  and a challenger wins only when strictly faster than the best so far. No
  timing under stream capture: the first challenger runs, uncached, so a
  normal warmup decides first."""
  use = DECODE_PICKS.get(key)
  if use is not None:
    return use
  base, *challengers = contenders()
  names = [name for name, _ in challengers]
  if torch.cuda.is_current_stream_capturing():
    return names[0]
  *times, t_base = [_time_us(fn) for _, fn in challengers + [base]]
  use, t_best = base[0], t_base * margin
  for name, t in zip(names, times):
    if t < t_best:
      use, t_best = name, t
  DECODE_PICKS[key] = use
  if os.getenv("XOT_DEBUG", "0") != "0":
    shape = " ".join(f"{d}={v}" for d, v in zip(dims, key[-len(dims):]))
    print(f"[xot] {what} auto-pick {shape}: " + " / ".join(f"{n} {t:.1f} us" for n, t in zip(names, times))
          + f" vs {base[0]} {t_base:.1f} us -> {use}", flush=True)
  return use


class XotLinear(nn.Linear):
  """nn.Linear with an optional decode-path prepack: `pack_decode()` stores a
  second copy of the weight in MFMA A-fragment order ([N/32,K/16,64,8], see
  ops.pack_decode_weight); decode-shaped (rows 32..256) bf16 GEMMs then run
  the hand-written CDNA4 weight-streaming kernel where it measures faster
  than hipBLASLt (auto-picked per (N,K,M) at first call: e.g. 70B down_proj
  110 -> 84.6 us, lm_head 5.3 -> 6.2 TB/s; hipBLASLt keeps the shapes it
  wins). Prefill/training/CPU stay on hipBLASLt/aten. Storage/state-dict
  identical to nn.Linear."""

  def __init__(self, *a, **kw):
    super().__init__(*a, **kw)
    self.weight_packed = None
    self.weight_packed_fp8 = None
    self.weight_scale = None
    self.weight_packed_w4 = None  # MXFP4 code image (ops.pack_decode_weight_mxfp4)
    self.weight_scale_w4 = None   # its e8m0 scale image
    self.keep_bf16 = False  # W4 mode leaves this module's weight and pack in bf16 (lm_head)
    # glu_store: set by the model's pack policy on a dense gate_up projection
    # (llama.pack_decode_weights); _pack() then stores the GLU-interleaved image.
    # glu_packed: weight_packed IS that image, which only
    # ops.skinny_gemm_packed_glu reads (llama.MLP.forward), never _gemm
    self.glu_store = False
    self.glu_packed = False
    self._w8 = None  # lazily cached fp8 prefill copy (_fp8_prefill)
    self._w8_scale = None

  def packable(self) -> bool:
    N, K = self.weight.shape
    return N % 128 == 0 and K % 64 == 0

  def pack_decode(self):
    if self.packable() and self.weight.is_cuda and self.weight.dtype == torch.bfloat16:
      self._pack()

  def _pack(self):
    """The pack of the format the environment selects. MXFP4 also writes the
    dequantized weight back into `weight`: prefill, the hipBLASLt arm and the
    W4 kernel then serve the same quantized model."""
    fmt = ops.decode_weight_format()
    if fmt == "fp8":
      if self.weight_packed_fp8 is None:
        self.weight_packed_fp8, self.weight_scale = ops.pack_decode_weight_fp8(self.weight.detach())
    elif fmt == "mxfp4" and not self.keep_bf16:
      if self.weight_packed_w4 is None:
        self.weight_packed_w4, self.weight_scale_w4, w_dq = ops.pack_decode_weight_mxfp4(self.weight.detach())
        with torch.no_grad():
          self.weight.copy_(w_dq)
    elif self.weight_packed is None:
      if self.glu_store:
        self.weight_packed = ops.pack_decode_weight_glu(self.weight.detach())
        self.glu_packed = True
      else:
        self.weight_packed = ops.pack_decode_weight(self.weight.detach())

  def unpack_decode(self):
    self.weight_packed = None
    self.glu_packed = False
    self.weight_packed_fp8 = None
    self.weight_packed_w4 = None
    self.weight_scale_w4 = None

  def _fp8_prefill(self, x):
    """Opt-in (XOT_FP8_PREFILL=1) e4m3 prefill GEMM via hipBLASLt scaled_mm:
    measured 2.58 vs 1.58 PF on the 70B gate_up prefill shape (rel err
    ~3.5%). Per-token activation scales, per-channel weight scales; the
    fp8 weight copy is cached lazily."""
    N, K = self.weight.shape
    M = x.numel() // K
    w8, sw = self._w8, self._w8_scale
    if w8 is None:
      w = self.weight.detach()
      sw = (w.float().abs().amax(dim=1, keepdim=True).clamp(min=1e-12) / 448.0)
      w8 = (w / sw.to(w.dtype)).clamp(-448, 448).to(torch.float8_e4m3fn)
      free, _ = torch.cuda.mem_get_info()
      if free > (12 << 30):  # persist the fp8 copy only with HBM headroom
        self._w8, self._w8_scale = w8, sw
    # activation quantization stays in bf16 (a fp32 image of a 65k x 8k
    # prefill activation would be 2 GB per layer)
    x2 = x.reshape(M, K)
    sx = (x2.abs().amax(dim=1, keepdim=True).float().clamp(min=1e-12) / 448.0)
    x8 = (x2 / sx.to(x2.dtype)).clamp(-448, 448).to(torch.float8_e4m3fn)
    y = torch._scaled_mm(x8, w8.t(), scale_a=sx, scale_b=sw.t(),
                         out_dtype=torch.bfloat16)
    if self.bias is not None:
      y = y + self.bias
    return y.view(list(x.shape[:-1]) + [N])

  def forward(self, x, epilogue=None):
    """epilogue = (residual, norm_weight | None, eps) turns the result into
    (h' = y + residual, rmsnorm(h') | None): inside the packed kernel's
    split-K combine where that path is picked, else one add_rmsnorm launch."""
    y = self._gemm(x, epilogue)
    if epilogue is None or isinstance(y, tuple):
      return y
    res, w, eps = epilogue
    return ops.add_rmsnorm(y, res.view(y.shape), w, eps)

  def _gemm(self, x, epilogue=None):
    if (x.is_cuda and x.dtype == torch.bfloat16 and not torch.is_grad_enabled()
        and os.getenv("XOT_FP8_PREFILL", "0") == "1"):
      N, K = self.weight.shape
      M = x.numel() // K
      if M > 256 and N % 16 == 0 and K % 16 == 0 and x.is_contiguous():
        try:
          return self._fp8_prefill(x)
        except torch.cuda.OutOfMemoryError:
          torch.cuda.empty_cache()  # fall back to the bf16 path
    wp, wp8, wq = self.weight_packed, self.weight_packed_fp8, self.weight_packed_w4
    if wp is not None or wp8 is not None or wq is not None:
      N, K = self.weight.shape
      M = decode_rows(x, K)
      if M and wp8 is not None:
        x8, sx = ops.quant_fp8_rows(x.view(M, K))
        y = ops.skinny_gemm_fp8(x8, sx, wp8, self.weight_scale, 1, N, self.bias)
        return y.view(list(x.shape[:-1]) + [N])
      if M and wq is not None:
        # `weight` holds the dequantized values (pack_decode), so the library
        # arm computes the same model; it keeps the shapes where 4-bit loses
        b, ws = self.bias, self.weight_scale_w4
        use = auto_pick(("w4", N, K, M), "w4-gemm", "NKM", 0.95, lambda: [
          ("blaslt", lambda: torch.nn.functional.linear(x, self.weight, b)),
          ("mxfp4", lambda: ops.skinny_gemm_mxfp4(x, wq, ws, 1, N, b))])
        if use == "mxfp4":
          if epilogue is not None:
            return ops.skinny_gemm_mxfp4_epilogue(x, wq, ws, N, b, epilogue)
          return ops.skinny_gemm_mxfp4(x, wq, ws, 1, N, b)
      if M and wp is not None and not self.glu_packed:  # a GLU-interleaved pack goes to the library here
        b = self.bias
        use = auto_pick((N, K, M), "gemm", "NKM", 0.95, lambda: [
          ("blaslt", lambda: torch.nn.functional.linear(x, self.weight, b)),
          ("packed", lambda: ops.skinny_gemm_packed(x, wp, N, b)),
          ("xreg", lambda: ops.skinny_gemm_packed_xreg(x, wp, N, b))])
        if use == "xreg":
          return ops.skinny_gemm_packed_xreg(x, wp, N, b)
        if use == "packed":
          if epilogue is not None:
            return ops.skinny_gemm_packed_epilogue(x, wp, N, b, epilogue)
          return ops.skinny_gemm_packed(x, wp, N, b)
    return ops.linear(x, self.weight, self.bias)
