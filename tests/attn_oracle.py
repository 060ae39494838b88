"""fp64 oracle for the decode-attention kernels (plain helper module, not a
conftest): reference packers of the fragment layouts, seeded input families
built to make wrong kernels visible, fp64 references with switchable
mutations, a derived error bound, and a CPU emulator of the fp8 P quantization.

Everything here runs on the CPU. The GPU tests move `device_inputs(case)` to
the card, launch one kernel and hand its output to `ratio(case, ref, out)`.

Error model (the bound, per output element; w = softmax weights, v = the V
values the kernel consumes, ref = sum_t w_t v_t, absw = sum_t w_t |v_t|):

  |out - ref| <= (pterm + eps_rel * absw) * (1 + 2^-8) + 2^-8 * |ref|

  Rounding to nearest into a format with s stored mantissa bits is off by at
  most half an ulp, 2^-(s+1) of the value's binade: 2^-8 for bf16 (s = 7),
  2^-4 for e4m3 (s = 3). (1 + 2^-8 lies midway between the bf16 neighbours 1
  and 1 + 2^-7, so no kernel that returns bf16 can promise 2^-9.)

  2^-8 * |ref|   final round-to-nearest of the fp32 result to bf16; the factor
                 (1 + 2^-8) carries the same rounding of the other terms.
  pterm, bf16    P is rounded to bf16 before the PV MFMA while the softmax
                 denominator keeps the fp32 p: each term of the numerator is
                 off by at most 2^-8 relative, so pterm = 2^-8 * absw. The
                 VALU kernel keeps p in fp32: pterm = 0 there.
  pterm, fp8     P' = p * s_v[t] / s_pv is rounded to e4m3, s_pv = the largest
                 V scale among the tile's positions below seq_len, so P' <= 1.
                 Half an ulp of e4m3 is 2^-4 relative for
                 normals (P' >= 2^-6); below that the spacing is 2^-9, half of
                 it 2^-10 absolute, in tile units. A position's term of the
                 output is P' * s_pv * code_t * exp(m_run - M) / L with
                 m_run <= M (running max against final max) and L the final
                 denominator, so a 2^-10 error of P' moves the output by at
                 most 2^-10 * (s_pv / s_v[t]) * |v_t| / L; and rounding never
                 moves a term by more than the term itself (flush to zero).
                   pterm = sum_t |v_t| * min(w_t, max(2^-4 w_t, 2^-10 rho_t / L)),
                   rho_t = s_pv(tile of t) / s_v[t].
  eps_rel        fp32 arithmetic on the scores and the accumulators:
                 a score is an fp32 sum of Dk exact products (bf16 x bf16 and
                 e4m3 x e4m3 fit fp32), then up to 8 fp32 multiplies/subtracts
                 (scale, s_q, s_k, softcap in and out, minus the max, times
                 log2 e inside __expf): |ds| <= 2^-24 * (Dk + 8) * sabs with
                 sabs = max_t scale * sum_d |q_d| |k_d| >= |s|. The hardware
                 exp2 adds 1 ulp = 2^-23 relative (taken as 2^-22 with the
                 final multiply), tanhf 2 ulp of a value <= 1, times softcap.
                 A relative error e_s on every p moves a weight by at most
                 2 e_s (numerator and denominator), hence the factor 2. The PV
                 sum and the denominator are fp32 sums of at most T terms,
                 rescaled once per tile and once per split by factors that are
                 the same rounded number on both: 2^-24 * (2 T + 16).
                   eps_rel = 2 * (2^-24 (Dk + 8) sabs + 2^-22 + 2^-22 softcap)
                             + 2^-24 (2 T + 16)
No constant above is fitted to kernel output.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

E4M3_MAX = 448.0
A_EDGE = 8.0    # V amplitude of the edges family's marker blocks
A_SCORE = 16.0  # V amplitude of the scores family's two marker blocks
A_TILE = 64.0   # V amplitude of the tiles family's half-tile blocks
BW = 16         # dims per marker block (edges, scores)
G_EDGE = 10.0   # score of an anchored position above the bulk (edges)
GAP = math.log(9.0)  # score gap of the two markers (scores)
MLA_LAT, MLA_ROPE = 512, 64


# ---------------------------------------------------------------------------
# Reference packers for the two fragment layouts at a general head dim, stated
# independently of the kernels:
#   K: d = c*32 + qt*8 + j, pos = tile*16 + p16, lane = qt*16 + p16
#      -> [B, KVH, t32/16, D/32, 64, 8]
#   V: pos = tp*32 + qt*8 + j, d = g*16 + c16, lane = qt*16 + c16
#      -> [B, KVH, D/16, t32/32, 64, 8]
# The MLA images are the same two layouts with one kv head: K over the 576
# [latent | rope] dims, V over the 512 latent dims.
# ---------------------------------------------------------------------------

def pad_t(x, t32):
  B, KVH, T, hd = x.shape
  out = torch.zeros(B, KVH, t32, hd, dtype=x.dtype, device=x.device)
  out[:, :, :T] = x
  return out


def pack_k(k, t32):
  B, KVH, _, hd = k.shape
  v = pad_t(k, t32).view(B, KVH, t32 // 16, 16, hd // 32, 4, 8)
  return v.permute(0, 1, 2, 4, 5, 3, 6).contiguous().view(B, KVH, t32 // 16, hd // 32, 64, 8)


def pack_v(v, t32):
  B, KVH, _, hd = v.shape
  w = pad_t(v, t32).view(B, KVH, t32 // 32, 4, 8, hd // 16, 16)
  return w.permute(0, 1, 5, 2, 3, 6, 4).contiguous().view(B, KVH, hd // 16, t32 // 32, 64, 8)


def unpack_k(kp, t32):
  B, KVH, _, chunks = kp.shape[:4]
  return kp.view(B, KVH, t32 // 16, chunks, 4, 16, 8).permute(0, 1, 2, 5, 3, 4, 6).reshape(B, KVH, t32, chunks * 32)


def unpack_v(vp, t32):
  B, KVH, groups = vp.shape[:3]
  return vp.view(B, KVH, groups, t32 // 32, 4, 16, 8).permute(0, 1, 3, 4, 6, 2, 5).reshape(B, KVH, t32, groups * 16)


def mla_pack(lat, rot, t32):
  """lat [B, T, 512], rot [B, T, 64] -> kp [B, t32/16, 18, 64, 8], vp [B, 32, t32/32, 64, 8]."""
  full = torch.cat([lat, rot], dim=-1)
  return pack_k(full[:, None], t32)[:, 0], pack_v(lat[:, None], t32)[:, 0]


# ---------------------------------------------------------------------------
# Launch geometry of the three bindings (split count and positions per split),
# restated here so that the tests can name the split they cut out of the
# reference and report which epilogue a case takes.
# ---------------------------------------------------------------------------

def split_geometry(kernel, B, H, KVH, T):
  t32 = (T + 31) // 32 * 32
  if kernel == "valu":
    nsplit = min(max(1, 512 // max(1, B * KVH)), max(1, (T + 127) // 128))
    return nsplit, (T + nsplit - 1) // nsplit
  groups, floor, cap = (B * KVH, 32, 32) if kernel == "mfma" else (B * ((H + 15) // 16), 16, 64)
  nsplit = 1
  while groups * nsplit * 2 < 4096 and t32 // (nsplit * 2) >= floor and nsplit < cap:
    nsplit *= 2
  return nsplit, ((t32 // nsplit + 31) >> 5) << 5


# ---------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class Spec:
  name: str
  kernel: str            # "mfma" | "valu" | "mla"
  hd: int                # q / k width (576 for mla)
  fp8: bool
  H: int
  KVH: int
  T: int
  lens: tuple
  softcap: float = 0.0
  window: int = 0
  anchor: str = "lat"    # mla, edges family: anchor inside the latent dims or the rope tail
  families: tuple = ("edges", "tiles", "scores", "plain")

  @property
  def dv(self):
    return MLA_LAT if self.kernel == "mla" else self.hd

  @property
  def scale(self):
    return self.hd ** -0.5


@dataclass
class Case:
  spec: Spec
  fam: list              # family of each batch row
  seq_lens: torch.Tensor  # [B] int64
  lo: torch.Tensor       # [B] first visible position
  q: torch.Tensor        # [B, H, Dk] fp32, bf16-exact: what a bf16 / GQA kernel is given
  qd: torch.Tensor       # [B, H, Dk] fp64: what the reference consumes (q8 * sq under fp8)
  k: torch.Tensor        # [B, G, T, Dk] fp64, as the kernel reads it (bf16-exact or dequantized)
  v: torch.Tensor        # [B, G, T, Dv] fp64
  q8: torch.Tensor = None   # fp8: e4m3 codes (uint8) and scales
  sq: torch.Tensor = None
  k8: torch.Tensor = None
  v8: torch.Tensor = None
  ksc: torch.Tensor = None  # [B, G, T] fp32, 1.0 beyond the filled positions
  vsc: torch.Tensor = None

  def rows(self, fam):
    return torch.tensor([f == fam for f in self.fam])


def _bf16(x):
  return x.to(torch.bfloat16).to(torch.float32)


def _gen_row(sp, fam, sl, g):
  """One batch row of family `fam`: q [H, Dk], k [G, T, Dk], v [G, T, Dv]
  (fp32, bf16-exact) and the number of filled positions."""
  H, G, T, Dk, Dv = sp.H, sp.KVH, sp.T, sp.hd, sp.dv
  mla = sp.kernel == "mla"
  lo = max(0, sl - sp.window) if sp.window else 0
  rn = lambda *s: torch.randn(*s, generator=g)
  k = rn(G, T, Dk)
  if mla:
    k[..., :MLA_LAT] *= 0.5
  v = k[..., :Dv] if mla else 0.5 * rn(G, T, Dv)  # mla: V (std 0.5) is the latent part of K, a view
  # anchor direction: +-1 on its support. MLA keeps it off the marker blocks'
  # dims (0..63), which V shares with K; the scores family and the "tail"
  # variant of edges put it inside the rope dims 512..575.
  if not mla:
    sup = torch.arange(Dk)
  elif fam in ("scores", "capped") or sp.anchor == "tail":
    sup = torch.arange(MLA_LAT, MLA_LAT + MLA_ROPE)
  else:
    sup = torch.arange(4 * BW, MLA_LAT)
  u = torch.zeros(Dk)
  u[sup] = torch.where(rn(len(sup)) < 0, -1.0, 1.0)
  n = len(sup)
  fill = sl
  nblk = 0
  if fam in ("tiles", "plain"):
    # moderately peaked random scores (std about 1) over V of std 0.5: that is
    # all of "plain"; in "tiles" every 16-position half-tile adds A_TILE to its
    # own block of (at most 8) V dims
    q = (1.5 if mla else 1.0) * rn(H, Dk)
    if fam == "tiles":
      nblk = T // 16
      stride = Dv // nblk
      bwid = min(stride, 8)
      pos = torch.arange(T)
      add = torch.zeros(T, Dv)
      # a half-tile's share of the weight falls as 1 / T: the amplitude grows with T past 1024
      add[pos[:, None], (pos // 16)[:, None] * stride + torch.arange(bwid)] = A_TILE * max(1, T // 1024)
      v += add
  elif fam == "ramp":
    # State carried from tile to tile inside one split: the odd 32-position
    # tiles score about 3 higher than the even ones (alpha = exp(-3) when a
    # split steps from an even tile to the odd one after it) and hold V 8 times
    # larger (the fp8 running scale steps by rfac = 1/8). Even tiles fill only
    # the lower half of the V dims and odd tiles the upper half, so the lower
    # half reads back exactly what was accumulated before the rescale.
    # MLA: q's latent part is 0, the scores come from the rope dims alone.
    sup = torch.arange(MLA_LAT, Dk) if mla else sup
    u = torch.zeros(Dk)
    u[sup] = torch.where(rn(len(sup)) < 0, -1.0, 1.0)
    a = math.sqrt(3.0 / (sp.scale * len(sup)))
    q = rn(H, Dk) + a * u
    if mla:
      q[:, :MLA_LAT] = 0
    odd = (torch.arange(T) // 32) % 2 == 1
    k[:, odd] += a * u
    vr = rn(G, T, Dv).abs()   # one sign: nothing cancels in the sum over positions
    half = Dv // 2
    v[:] = 0
    v[:, ~odd, :half] = 0.5 * vr[:, ~odd, :half]
    v[:, odd, half:] = 4.0 * vr[:, odd, half:]
  elif fam == "edges":
    # lo-1, lo, sl-1, sl carry K along the anchor (score about G_EDGE above the
    # bulk if visible) and V = A_EDGE in their own block; lo-1 and sl are poison
    a = math.sqrt(G_EDGE / (sp.scale * n))
    q = 0.5 * rn(H, Dk) + a * u
    anchored = set()
    for i, p in enumerate((lo - 1, lo, sl - 1, sl)):
      if 0 <= p < T:
        if p not in anchored:
          k[:, p] += a * u
          anchored.add(p)
        v[:, p, i * BW:(i + 1) * BW] += A_EDGE
    fill = min(sl + 1, T)  # the poison at sl is stale data past the length
    nblk, bwid = 4, BW
  else:
    # two visible markers whose K differ only along the anchor: their score gap
    # is scale * (c1 - c2) * a^2 * n = GAP for every head (q's random part is
    # orthogonal to the anchor), read back as the ratio of their V blocks.
    # Marker scores: 12, or under softcap 8 ("scores": the cap barely bends
    # them, so a wrong scale shows) and 24 ("capped": the cap halves the gap).
    gs = 24.0 if fam == "capped" else (8.0 if sp.softcap else 12.0)
    a = math.sqrt(gs / (sp.scale * n))
    qr = 0.5 * rn(H, Dk)
    qr -= (qr @ u / n)[:, None] * u
    q = qr + a * u
    p1, p2 = sl - 1, lo + (sl - 1 - lo) // 2
    if sl - lo >= 2:
      common = 0.5 * rn(G, Dk)
      k[:, p1] = common + a * u
      k[:, p2] = common + (1.0 - GAP / gs) * a * u
      v[:, p1, 0:BW] += A_SCORE
      v[:, p2, BW:2 * BW] += A_SCORE
      if p2 + 1 < p1:
        k[:, p2 + 1] *= 2.0   # p2's neighbour: an fp8 K scale unlike p2's own
    elif sl - lo == 1:
      k[:, p1] += a * u
      v[:, p1, 0:BW] += A_SCORE
    nblk, bwid = 2, BW
  if mla and nblk:
    # V blocks live in K's dims: keep q's sum over each block zero so that a
    # block of amplitude A adds nothing to the scores
    stride = Dv // nblk if fam == "tiles" else bwid
    qb = q[:, :nblk * stride].view(H, nblk, stride)[:, :, :bwid]
    qb -= qb.mean(-1, keepdim=True)
  k[:, fill:] = 0
  if not mla:
    v[:, fill:] = 0
  q, k = _bf16(q), _bf16(k)
  v = k[..., :Dv].clone() if mla else _bf16(v)
  return q, k, v, fill


def _quant_rows(x, amax):
  """e4m3 codes of x at scale amax / 448 (fp32 math, round to nearest even, saturating)."""
  sc = (amax.float().clamp_min(1e-12) / E4M3_MAX)
  codes = (x.float() * (1.0 / sc)[..., None]).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
  return codes, sc


def build_case(sp: Spec, seed: int = 0) -> Case:
  g = torch.Generator().manual_seed(1000 + seed)
  fam, lens, qs, ks, vs, fills = [], [], [], [], [], []
  for f in sp.families:
    for sl in sp.lens:
      q, k, v, fill = _gen_row(sp, f, sl, g)
      fam.append(f); lens.append(sl); qs.append(q); ks.append(k); vs.append(v); fills.append(fill)
  q, k, v = torch.stack(qs), torch.stack(ks), torch.stack(vs)
  sl_t = torch.tensor(lens)
  lo = (sl_t - sp.window).clamp_min(0) if sp.window else torch.zeros_like(sl_t)
  c = Case(sp, fam, sl_t, lo, q, q.double(), k.double(), v.double())
  if sp.fp8:
    # a fresh cache: codes 0 and scales 1.0 beyond the filled positions
    filled = torch.arange(sp.T)[None, None, :] < torch.tensor(fills)[:, None, None]
    k8, ksc = _quant_rows(k, k.abs().amax(-1))
    ksc = torch.where(filled, ksc, torch.ones_like(ksc))
    if sp.kernel == "mla":
      v8, vsc = k8[..., :MLA_LAT], ksc   # one scale per token over all 576 dims
    else:
      v8, vsc = _quant_rows(v, v.abs().amax(-1))
      vsc = torch.where(filled, vsc, torch.ones_like(vsc))
    # q: per-head amax / 448, fp32 multiply by the reciprocal (what the GQA
    # kernel does in registers and what the MLA caller passes in)
    q8, sq = _quant_rows(q, q.abs().amax(-1))
    c.q8, c.sq = q8.view(torch.uint8), sq
    c.k8, c.v8, c.ksc, c.vsc = k8.view(torch.uint8), v8.contiguous().view(torch.uint8), ksc, vsc
    c.qd = q8.float().double() * sq.double()[..., None]
    c.k = k8.float().double() * ksc.double()[..., None]
    c.v = v8.float().double() * vsc.double()[..., None]
  return c


def case_from_fp8_cache(kernel, q, k8, v8, ksc, vsc, seq_lens, softcap=0.0, window=0, sq=None) -> Case:
  """A case over an fp8 cache that the append kernels wrote: k8 / v8 are the
  unpacked e4m3 codes [B, G, T, D] (uint8), ksc / vsc their scales [B, G, T].
  q is the bf16 query [B, H, Dk] of the GQA kernel, quantized here as the
  kernel does it, or (sq given) the MLA caller's e4m3 codes with scales sq."""
  q, k8, v8, ksc, vsc = (x.detach().cpu() for x in (q, k8, v8, ksc, vsc))
  B, H, Dk = q.shape
  sp = Spec("cache", kernel, Dk, True, H, k8.shape[1], k8.shape[2], tuple(int(s) for s in seq_lens),
            softcap, window, families=("plain",))
  if sq is None:
    q = q.float()
    q8, sq = _quant_rows(q, q.abs().amax(-1))
    q8 = q8.view(torch.uint8)
  else:
    q8, sq = q, sq.detach().cpu().float()
  sl_t = torch.tensor(sp.lens)
  lo = (sl_t - window).clamp_min(0) if window else torch.zeros_like(sl_t)
  f = lambda x: x.view(torch.float8_e4m3fn).float().double()
  return Case(sp, ["plain"] * B, sl_t, lo, q, f(q8) * sq.double()[..., None], f(k8) * ksc.double()[..., None],
              f(v8) * vsc.double()[..., None], q8, sq, k8, v8, ksc.float(), vsc.float())


def fp8_cache_worst_ratio(out, q, kp8, vp8, ksc, vsc, seq_lens, softcap=0.0, window=0, sq=None) -> float:
  """Worst |out - ref| / bound of one fp8 decode over packed caches: the GQA
  kernel's (q bf16 [B, 1, H, hd], kp8 / vp8 6-d) or, with sq, the MLA kernel's
  (q e4m3 codes [B, H, 576], kp8 / vp8 5-d, ksc [B, T], vsc unused)."""
  T = ksc.shape[-1]
  if sq is None:
    c = case_from_fp8_cache("mfma", q[:, 0], unpack_k(kp8, T), unpack_v(vp8, T), ksc, vsc, seq_lens, softcap, window)
  else:
    k8 = unpack_k(kp8[:, None], T)
    c = case_from_fp8_cache("mla", q, k8, k8[..., :MLA_LAT], ksc[:, None], ksc[:, None], seq_lens, sq=sq)
  worst = ratio(c, reference(c), out).amax().item()
  print(f"fp8 decode vs fp64 oracle on the dequantized cache: worst err/bound {worst:.3f}")
  return worst


def device_inputs(c: Case, device="cuda"):
  """The tensors of one launch, packed as the binding of c.spec.kernel takes them."""
  sp = c.spec
  d = dict(seq_lens=c.seq_lens.to(torch.int32).to(device))
  bf = lambda x: x.to(torch.bfloat16).to(device)
  if sp.kernel == "valu":
    d.update(q=bf(c.q)[:, None], kc=bf(c.k), vc=bf(c.v))
  elif sp.kernel == "mfma":
    d["q"] = bf(c.q)[:, None]
    if sp.fp8:
      d.update(kp=pack_k(c.k8, sp.T).to(device), vp=pack_v(c.v8, sp.T).to(device),
               k_scale=c.ksc.to(device), v_scale=c.vsc.to(device))
    else:
      d.update(kp=pack_k(bf(c.k), sp.T), vp=pack_v(bf(c.v), sp.T))
  else:
    if sp.fp8:
      kp, vp = mla_pack(c.k8[:, 0, :, :MLA_LAT], c.k8[:, 0, :, MLA_LAT:], sp.T)
      d.update(q=c.q8.to(device), kp=kp.to(device), vp=vp.to(device),
               q_scale=c.sq.contiguous().to(device), k_scale=c.ksc[:, 0].contiguous().to(device))
    else:
      kb = bf(c.k)
      kp, vp = mla_pack(kb[:, 0, :, :MLA_LAT], kb[:, 0, :, MLA_LAT:], sp.T)
      d.update(q=bf(c.q), kp=kp, vp=vp)
  return d


# ---------------------------------------------------------------------------
# fp64 reference, with the mutations a wrong kernel would amount to
# ---------------------------------------------------------------------------

@dataclass
class Ref:
  out: torch.Tensor    # [B, H, Dv]
  absw: torch.Tensor   # [B, H, Dv]  sum_t w_t |v_t|
  w: torch.Tensor      # [B, H, T]
  L: torch.Tensor      # [B, H]      sum_t exp(s_t - max s)
  sabs: torch.Tensor   # [B, H]      max_t scale * sum_d |q_d| |k_d|
  s: torch.Tensor      # [B, H, T]   scores after scale and softcap, unmasked


def reference(c: Case, *, sl_shift=0, lo_shift=0, drop=None, scale_mul=1.0, no_softcap=False,
              no_tail=False, k_scale_shift=False) -> Ref:
  """GQA decode (per-row seq_lens, scale, softcap, window) or MLA decode
  (scores over [lat | rot], PV over lat) in fp64. Mutations: sl_shift /
  lo_shift move an end of the visible range, drop = (p0, p1) per-row tensors
  hides [p0, p1), scale_mul scales the scores, no_softcap skips the tanh,
  no_tail ignores the 64 rope dims (MLA), k_scale_shift dequantizes K with the
  scale of the next position (fp8)."""
  sp = c.spec
  B, H, Dk = c.qd.shape
  G, T = c.k.shape[1], c.k.shape[2]
  q, k = c.qd, c.k
  if k_scale_shift:
    nxt = torch.arange(T).add(1).clamp_max(T - 1)
    k = c.k8.view(torch.float8_e4m3fn).float().double() * c.ksc.double()[:, :, nxt, None]
  if no_tail:
    q, k = q[..., :MLA_LAT], k[..., :MLA_LAT]
  qg = q.reshape(B, G, H // G, -1)
  s = torch.einsum("bgrd,bgtd->bgrt", qg, k).reshape(B, H, T) * (sp.scale * scale_mul)
  sabs = torch.einsum("bgrd,bgtd->bgrt", qg.abs(), k.abs()).reshape(B, H, T) * sp.scale
  if sp.softcap and not no_softcap:
    s = sp.softcap * torch.tanh(s / sp.softcap)
  sl = (c.seq_lens + sl_shift).clamp(0, T)
  lo = (c.seq_lens - sp.window + lo_shift).clamp_min(0) if sp.window else torch.zeros_like(sl)
  pos = torch.arange(T)[None, :]
  vis = (pos >= lo[:, None]) & (pos < sl[:, None])
  if drop is not None:
    vis &= ~((pos >= drop[0][:, None]) & (pos < drop[1][:, None]))
  vis = vis[:, None, :]
  sm = s.masked_fill(~vis, -math.inf)
  M = sm.amax(-1, keepdim=True)
  M = torch.where(torch.isfinite(M), M, torch.zeros_like(M))  # rows with nothing visible
  e = torch.exp(sm - M)
  L = e.sum(-1)
  w = e / L.clamp_min(1e-300)[..., None]
  wg = w.reshape(B, G, H // G, T)
  out = torch.einsum("bgrt,bgtd->bgrd", wg, c.v).reshape(B, H, -1)
  absw = torch.einsum("bgrt,bgtd->bgrd", wg, c.v.abs()).reshape(B, H, -1)
  return Ref(out, absw, w, L, sabs.masked_fill(~vis, 0.0).amax(-1), s)


def bound(c: Case, ref: Ref) -> torch.Tensor:
  """Per-element error bound of a correct kernel (derivation: module docstring)."""
  sp = c.spec
  B, H, T = ref.w.shape
  G = c.k.shape[1]
  if sp.fp8:
    vs = c.vsc.double()
    below = torch.arange(T)[None, None, :] < c.seq_lens[:, None, None]
    spv = torch.where(below, vs, torch.zeros_like(vs)).view(B, G, T // 32, 32).amax(-1).clamp_min(1e-12)
    rho = spv.repeat_interleave(32, dim=-1) / vs                      # [B, G, T]
    rho = rho[:, :, None, :].expand(B, G, H // G, T).reshape(B, H, T)
    sub = 2.0 ** -10 * rho / ref.L.clamp_min(1.0)[..., None]
    e = torch.minimum(ref.w, torch.maximum(2.0 ** -4 * ref.w, sub))
    pterm = torch.einsum("bgrt,bgtd->bgrd", e.reshape(B, G, H // G, T), c.v.abs()).reshape(B, H, -1)
  elif sp.kernel == "valu":
    pterm = 0.0   # p stays in fp32
  else:
    pterm = 2.0 ** -8 * ref.absw
  e_s = 2.0 ** -24 * (c.qd.shape[-1] + 8) * ref.sabs + 2.0 ** -22 + 2.0 ** -22 * sp.softcap
  eps_rel = (2.0 * e_s + 2.0 ** -24 * (2 * T + 16))[..., None]
  return (pterm + eps_rel * ref.absw) * (1.0 + 2.0 ** -8) + 2.0 ** -8 * ref.out.abs()


def ratio(c: Case, ref: Ref, out) -> torch.Tensor:
  """|out - ref| / bound per element; 0 where both vanish, inf where only the bound does."""
  err = (out.double().cpu().reshape(ref.out.shape) - ref.out).abs()
  b = bound(c, ref)
  return torch.where(err == 0, torch.zeros_like(err), err / b)


def report(c: Case, r: torch.Tensor) -> str:
  worst = {f: r[c.rows(f)].max().item() for f in c.spec.families}
  nsplit, chunk = split_geometry(c.spec.kernel, len(c.fam), c.spec.H, c.spec.KVH, c.spec.T)
  return f"{c.spec.name}: nsplit {nsplit} chunk {chunk} worst err/bound " + \
         " ".join(f"{f} {x:.3f}" for f, x in worst.items())


# ---------------------------------------------------------------------------
# Mutations and the rows each applies to
# ---------------------------------------------------------------------------

def mutations(c: Case):
  """(name, reference kwargs, [B] mask of the rows it must move) for every
  mutation that applies to the case."""
  sp = c.spec
  B, T = len(c.fam), sp.T
  sl, lo = c.seq_lens, c.lo
  nvis = sl - lo
  edges, tiles, scores, capped = c.rows("edges"), c.rows("tiles"), c.rows("scores"), c.rows("capped")
  nsplit, chunk = split_geometry(sp.kernel, B, sp.H, sp.KVH, T)
  muts = [("sl+1", dict(sl_shift=1), edges & (sl < T)),
          ("sl-1", dict(sl_shift=-1), edges & (sl >= 1))]
  if sp.window:
    muts += [("lo+1", dict(lo_shift=1), edges & (sl - sp.window + 1 > 0)),
             ("lo-1", dict(lo_shift=-1), edges & (lo >= 1))]
  # the first and the last half-tile that lie wholly inside the visible range
  first = (lo + 15) // 16 * 16
  last = sl // 16 * 16 - 16
  has_full = tiles & (last >= first)
  muts += [("half-tile (first)", dict(drop=(first, first + 16)), has_full),
           ("half-tile (last)", dict(drop=(last, last + 16)), has_full)]
  c0 = last.clamp_min(0) // chunk * chunk
  muts.append(("split", dict(drop=(c0, c0 + chunk)), has_full))
  muts.append(("scale*sqrt2", dict(scale_mul=math.sqrt(2.0)), scores & (nvis >= 2)))
  if sp.softcap:
    muts.append(("no softcap", dict(no_softcap=True), capped & (nvis >= 2)))
  if sp.kernel == "mla":
    muts.append(("no rope tail", dict(no_tail=True), scores & (nvis >= 2)))
  if sp.fp8:
    muts.append(("k_scale of neighbour", dict(k_scale_shift=True), scores & (nvis >= 2)))
  return muts


# ---------------------------------------------------------------------------
# CPU emulator of the kernels' tile loop, one split at a time as the launch
# geometry cuts them: 32-position tiles, running max m and sum l, the rescale
# alpha of what was accumulated before, and under fp8 the tile's s_pv, P'
# rounded to e4m3 and the accumulator kept in units of 1/R with R = the last
# s_pv (rfac = R / s_pv moves it from tile to tile). Everything else is fp64.
#   whole_tile  s_pv over all 32 positions of a tile, visible or not, instead
#               of only those below the split's visible end
#   quantize    round P' to e4m3 (fp8 cases)
#   drop_alpha / drop_rfac   leave that factor out of the accumulator rescale:
#               what a kernel wrong in the tile-to-tile carry would compute
# ---------------------------------------------------------------------------

def emulate_tiles(c: Case, ref: Ref, whole_tile=False, quantize=False, drop_alpha=False, drop_rfac=False,
                  rows=None) -> torch.Tensor:
  sp = c.spec
  B, H, T = ref.w.shape
  G, rep = sp.KVH, sp.H // sp.KVH
  nsplit, chunk = split_geometry(sp.kernel, B, H, G, T)
  if sp.fp8:
    vals, vsc = c.v8.view(torch.float8_e4m3fn).float().double(), c.vsc.double()
  else:
    vals, vsc = c.v, torch.ones(B, G, T, dtype=torch.float64)
  e4m3 = lambda x: x.float().to(torch.float8_e4m3fn).float().double()
  out = torch.zeros(B, H, sp.dv, dtype=torch.float64)
  for b in (range(B) if rows is None else rows):
    sl, lo = int(c.seq_lens[b]), int(c.lo[b])
    for g in range(G):
      hs = slice(g * rep, (g + 1) * rep)
      ms, ls, accs = [], [], []
      for split in range(nsplit):
        c0 = max(split * chunk, lo // 32 * 32)
        c1 = min(split * chunk + chunk, sl)
        m = torch.full((rep,), -math.inf, dtype=torch.float64)
        l = torch.zeros(rep, dtype=torch.float64)
        acc = torch.zeros(rep, sp.dv, dtype=torch.float64)   # in units of 1 / R
        R = torch.tensor(1.0, dtype=torch.float64)
        for t in range(c0, c1, 32):
          pos = torch.arange(t, t + 32)
          ok = (pos < c1) & (pos >= lo)
          s = ref.s[b, hs, t:t + 32].masked_fill(~ok, -math.inf)
          mn = torch.maximum(m, s.amax(-1))
          alpha = torch.where(l > 0, torch.exp(m - mn), torch.zeros_like(l))
          p = torch.exp(s - mn[:, None])
          l = l * alpha + p.sum(-1)
          vs = vsc[b, g, t:t + 32]
          s_pv = (vs if whole_tile else vs[pos < c1]).max().clamp_min(1e-12)
          rfac, R = R / s_pv, s_pv
          pq = p * vs / s_pv
          if quantize:
            pq = e4m3(pq)
          acc = acc * (torch.ones_like(alpha) if drop_alpha else alpha)[:, None] * (1.0 if drop_rfac else rfac) \
              + pq @ vals[b, g, t:t + 32]
          m = mn
        ms.append(m); ls.append(l); accs.append(acc * R)
      ms, ls, accs = torch.stack(ms), torch.stack(ls), torch.stack(accs)
      M = ms.amax(0)
      al = torch.where(ls > 0, torch.exp(ms - M), torch.zeros_like(ls))
      Lt = (al * ls).sum(0)
      O = (al[..., None] * accs).sum(0)
      out[b, hs] = torch.where(Lt[:, None] > 0, O / Lt.clamp_min(1e-300)[:, None], torch.zeros_like(O))
  return out


def emulate_fp8(c: Case, ref: Ref, whole_tile: bool) -> torch.Tensor:
  return emulate_tiles(c, ref, whole_tile=whole_tile, quantize=True)


# ---------------------------------------------------------------------------
# The cases of the GPU file (tests/test_attn_decode_oracle_gpu.py); the CPU
# file checks every one of them for emulator and mutation margins.
# ---------------------------------------------------------------------------

LENS_128 = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 100, 127, 128)
LENS_256 = (1, 31, 33, 63, 64, 65, 96, 127, 128, 129, 160, 191, 192, 193, 255, 256)
LENS_1024 = (1, 40, 65, 520, 1000, 1024)
LENS_WINDOW = (41, 72, 73, 103, 104, 105, 128)
LENS_2048 = (33, 100, 1000, 1990, 2048)
LENS_128_MORE = LENS_128 + (2, 8, 20, 40, 48, 50, 66, 70, 80, 90, 99, 101, 110, 112, 120, 126)
WITH_RAMP = ("edges", "tiles", "scores", "plain", "ramp")


def _specs():
  out = []
  for hd in (128, 256):
    for fp8 in (False, True):
      tag = f"mfma{hd}-{'fp8' if fp8 else 'bf16'}"
      kw = dict(kernel="mfma", hd=hd, fp8=fp8, H=8, KVH=2)
      out += [Spec(f"{tag}-T128", T=128, lens=LENS_128, **kw),
              Spec(f"{tag}-T256", T=256, lens=LENS_256, **kw),
              Spec(f"{tag}-T1024", T=1024, lens=LENS_1024, **kw),
              Spec(f"{tag}-T128-window40-softcap30", T=128, lens=LENS_WINDOW, softcap=30.0, window=40,
                   families=("edges", "tiles", "scores", "capped", "plain"), **kw)]
      # two 32-position tiles per split, so that alpha, rfac and the K prefetch act on
      # accumulated state: T=2048 gives nsplit 32 (the cap), chunk 64, workspace merge
      out.append(Spec(f"{tag}-T2048", T=2048, lens=LENS_2048, families=WITH_RAMP, **kw))
  # 128 rows x 8 kv heads at T=128: nsplit 2, chunk 64, merged in the workgroup
  for fp8 in (False, True):
    out.append(Spec(f"mfma128-{'fp8' if fp8 else 'bf16'}-T128-B128", kernel="mfma", hd=128, fp8=fp8, H=16, KVH=8,
                    T=128, lens=LENS_128_MORE, families=("edges", "tiles", "scores", "ramp")))
  # 7 query heads per kv head: q rows 7..15 of the MFMA tile are clamped copies
  out.append(Spec("mfma128-fp8-T128-H14", kernel="mfma", hd=128, fp8=True, H=14, KVH=2, T=128, lens=LENS_128))
  for hd in (64, 128):
    out.append(Spec(f"valu{hd}-bf16-T128", kernel="valu", hd=hd, fp8=False, H=8, KVH=2, T=128, lens=LENS_128))
  for fp8 in (False, True):
    for H in (16, 20):
      tag = f"mla-{'fp8' if fp8 else 'bf16'}-H{H}"
      kw = dict(kernel="mla", hd=MLA_LAT + MLA_ROPE, fp8=fp8, H=H, KVH=1)
      out += [Spec(f"{tag}-T128", T=128, lens=LENS_128, anchor="tail", **kw),
              Spec(f"{tag}-T1024", T=1024, lens=(40, 65, 1000), anchor="lat", **kw)]
    # nsplit 64 (the cap), chunk 64: two tiles per split
    out.append(Spec(f"mla-{'fp8' if fp8 else 'bf16'}-H16-T4096", kernel="mla", hd=MLA_LAT + MLA_ROPE, fp8=fp8, H=16,
                    KVH=1, T=4096, lens=(100, 2100, 4090), anchor="lat", families=WITH_RAMP))
  return out


SPECS = _specs()

# one zero-length row between two live ones, per kernel
ZERO_SPECS = [Spec(f"zero-{s.name}", s.kernel, s.hd, s.fp8, s.H, s.KVH, 128, (40, 0, 97), families=("edges",))
              for s in SPECS if s.name.endswith("-T128") and s.H in (8, 16)]
