"""Integer oracle for the decode GEMMs (plain helper module, not a conftest):
seeded input families, CPU references with one-defect mutations, and the
launch plan restated so that a test can name the split and the K-step it cuts
out. Everything here runs on the CPU; the GPU tests move `launch_args(case)`
to the card, launch one binding and compare on the CPU.

Exact family. The kernels multiply bf16 (e4m3, e2m1) operands, accumulate in
fp32, add fp32 split-K partials and round to bf16 once. With w in {-1, +1},
x in {0, -1, +1, -A, +A} (at most 512 non-zeros per row), every product is an
integer, every partial sum in any order stays below 2 * A + 512 < 2^24, and
the final sums are asserted to be at most 256 in magnitude. Every such value
is exact in fp32 and the result is exact in bf16, so a correct kernel returns
the bits of `matmul -> bf16` whatever its tile, BK, split count or order. The
reference multiplies in fp64, which is exact for these integers. The +-A
entries come in cancelling pairs on two equal weight columns that lie in
different 16-k chunks and, when K is split, in different splits: they add zero
to the result and make the intermediate sums 13 (fp8: 9) bits wide, so an
accumulator or partial narrower than fp32 loses the +-1 terms.

Variants. fp8: integer e4m3 codes and power-of-two scales, still exact.
MXFP4: the +-1 weight dequantizes to itself. SwiGLU staging: gate in {0, 32}
and up = j / 32; exp(-32) < 2^-24, so 1 + exp(-32) rounds to 1, rcp(1) = 1
and silu(32) * j / 32 = j exactly; silu(0) * up = 0. Row epilogue: an integer
residual with |y + res| <= 256. GLU store: integer sums G and U, reference
silu(G) * U in fp64, see glu_bound.

Real family (x ~ N(0, 0.5), w ~ N(0, 0.02), bias ~ N(0, 0.5), all bf16;
reference in fp64). Per output, with T = sum_k |x_k| |w_k| + |bias|:

  |got - ref| <= 2^-8 |ref'| + (K + nsplit + 2) 2^-24 T,
  ref' = |ref| + (K + nsplit + 2) 2^-24 T.

  Products of two bf16 (8-bit significands) are exact in fp32. The sum of K of
  them takes at most K - 1 fp32 additions however they are grouped into MFMA
  chunks, steps and splits, the nsplit partials nsplit - 1 more, the bias one:
  under K + nsplit additions, each off by at most 2^-24 of a partial sum that
  is itself at most T (1 + 2^-24)^K in magnitude. K + nsplit + 2 leaves two
  roundings to spare (fp8: the two scale multiplies). What is rounded to bf16
  is then within the second term of ref, so its magnitude is at most ref', and
  round-to-nearest moves it by at most half an ulp, 2^-8 relative. Truncation
  would move it by up to 2^-7: the exact family cannot see that, this one can.

GLU store (glu_bound). The kernel rounds both sums to bf16 (Gb, Ub), then
s = Gb * rcp(1 + __expf(-Gb)) and out = bf16(s * Ub), all fp32. With
dG = |Gb - G|, dU = |Ub - U| (zero for the exact family's integers) and
|silu'| <= 1.1:
  |out - ref| <= 2^-8 r' + eps |ref| + 1.1 dG (|U| + dU) + |silu(G)| dU
                 + 2^-126 (1 + |U|)
  eps = 2^-24 (|G| + 7): __expf is exp2(x * log2 e); the product's rounding
  moves the result by |G| 2^-24 relative, V_EXP_F32 and V_RCP_F32 are 1 ulp
  (2^-23) each as the CDNA ISA reference states them, and 1 + e, G * rcp and
  s * U are one rounding (2^-24) each. r' = |ref| plus the other terms. The
  last term is the flush of results below the fp32 normal range: silu(-100) is
  2^-139 and comes out as zero.
No constant above is fitted to kernel output.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import torch

from xotorch_amd import ops

PACKED_OPS = ("packed", "grouped", "epilogue", "swiglu", "swiglu_epilogue", "glu", "mxfp4")
BIG = 1 << 20  # XOT_SKINNY_TARGET that splits K as far as the plan's other rules allow


# ---------------------------------------------------------------------------
# The launch plan (skinny_plan, skinny_wide_tile and the BK rule of skinny_run)
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class Plan:
  nsplit: int
  kc: int
  bk: int
  nw: int

  def split_range(self, s, K):
    return s * self.kc, min((s + 1) * self.kc, K)


def plan(op, M, K, N, E=1, target=384, bk64=False, bn=None) -> Plan:
  k_align = 16 if op == "plain" else 64
  packed = op in PACKED_OPS
  ntiles = N // 128
  tgt = 0 if op == "glu" else target
  nsplit = 1
  while ntiles * nsplit * E < tgt and K // (nsplit * 2) >= 1024 and nsplit < 16:
    nsplit *= 2
  kc = (K // nsplit + k_align - 1) // k_align * k_align
  while kc * (nsplit - 1) >= K:
    nsplit -= 1
  bk = 128 if packed and K % 128 == 0 and kc % 128 == 0 and kc >= 2048 and not bk64 else 64
  wide = False
  if packed and M >= 128 and N % 256 == 0:
    if bn is not None:
      wide = bn == 256
    elif M < 256:
      wide = kc >= 2048
    else:
      wide = (ntiles // 2) * nsplit * E >= 128
  if wide and M // 32 >= 7:
    bk = 64
  return Plan(nsplit, kc, bk, 8 if wide else 4)


# ---------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------

@dataclass(frozen=True)
class Spec:
  op: str            # packed | plain | xreg | grouped | epilogue | swiglu | swiglu_epilogue | glu | fp8 | mxfp4
  M: int             # rows per expert
  K: int
  N: int = 256
  E: int = 1
  bias: bool = False
  target: int = 0    # XOT_SKINNY_TARGET: 0 unsplit, BIG split as far as K allows
  bk64: bool = False  # XOT_SKINNY_BK64
  bn: int = None     # XOT_SKINNY_BN
  family: str = "exact"

  @property
  def name(self):
    s = f"{self.op}-{self.family}-M{self.M}-K{self.K}-N{self.N}"
    s += f"-E{self.E}" if self.E > 1 else ""
    s += f"-t{'big' if self.target == BIG else self.target}" + ("-bk64" if self.bk64 else "")
    return s + (f"-bn{self.bn}" if self.bn else "") + ("-bias" if self.bias else "")

  @property
  def plan(self) -> Plan:
    return plan(self.op, self.M, self.K, self.N, self.E, self.target, self.bk64, self.bn)

  @property
  def seed(self):
    return zlib.crc32(self.name.encode())


@dataclass
class Case:
  spec: Spec
  x: torch.Tensor          # [E*M, K] fp64: what the MFMA consumes (fp8: the codes' values)
  w: torch.Tensor          # [E, N, K] fp64 (fp8: the codes' values)
  bias: torch.Tensor = None  # [N] fp64
  res: torch.Tensor = None   # [E*M, N] fp64 (row epilogue)
  sx: torch.Tensor = None    # fp8: [E*M] and [E, N] fp64
  sw: torch.Tensor = None
  gu: torch.Tensor = None    # SwiGLU staging: the fused [M, 2K] gate | up input
  S: torch.Tensor = None     # [E*M, N] fp64 sums before scales, bias, activation and residual
  T: torch.Tensor = None     # real family: sum |x||w| (+ |bias|) in output units
  ref: torch.Tensor = None   # the output, fp64
  extra: dict = field(default_factory=dict)


def _bf16(t):
  return t.to(torch.bfloat16).double()


def _pm1(g, *shape):
  return torch.randint(0, 2, shape, generator=g).double() * 2 - 1


def sums(c: Case, x=None, w=None, ks=None):
  """x @ w[e]^T per expert over the k range ks (a slice), fp64."""
  sp = c.spec
  x = c.x if x is None else x
  w = c.w if w is None else w
  ks = slice(None) if ks is None else ks
  return torch.cat([x[e * sp.M:(e + 1) * sp.M, ks] @ w[e][:, ks].T for e in range(sp.E)])


def finish(c: Case, S, with_bias=True):
  """Scales, bias, activation and residual on the sums S, as the kernel's store applies them."""
  sp = c.spec
  y = S
  if sp.op == "fp8":
    y = y * c.sx[:, None] * c.sw.repeat_interleave(sp.M, dim=0)
  if c.bias is not None and with_bias:
    y = y + c.bias
  if sp.op == "glu":
    G, U = y[:, :sp.N // 2], y[:, sp.N // 2:]
    y = G * torch.sigmoid(G) * U
  if c.res is not None:
    y = y + c.res
  return y


def build_case(sp: Spec) -> Case:
  assert sp.M % 32 == 0 and 32 <= sp.M <= 256 and sp.N % 128 == 0 and sp.K % (16 if sp.op == "plain" else 64) == 0
  c = _build_exact(sp) if sp.family == "exact" else _build_real(sp)
  c.S = sums(c)
  c.ref = finish(c, c.S)
  if sp.family == "exact" and sp.op != "glu":
    # the builder's condition, on the reference alone
    assert c.ref.abs().max() <= 256, (sp.name, c.ref.abs().max().item())
    assert torch.equal(c.ref, _bf16(c.ref)), sp.name
    assert c.S.abs().max() <= 256
  if sp.family == "exact":
    assert torch.equal(c.S, c.S.round()) and int((c.x != 0).sum(1).max()) <= 512
  return c


def _build_exact(sp: Spec) -> Case:
  g = torch.Generator().manual_seed(sp.seed)
  pl = sp.plan
  M, K, N, E = sp.M, sp.K, sp.N, sp.E
  rows, C = E * M, K // 16
  fp8 = sp.op == "fp8"
  A = 256.0 if fp8 else 4096.0
  w = _pm1(g, E, N, K)
  # fill: about nnz non-zeros per row, then one per (16-k chunk, 32-row m-tile) cell
  nnz = min(128 if fp8 else 384, K // 2)
  x = (torch.rand(rows, K, generator=g) < nnz / K).double() * _pm1(g, rows, K)
  r = torch.arange(rows // 32)[:, None] * 32 + torch.randint(0, 32, (rows // 32, C), generator=g)
  k = torch.arange(C)[None, :] * 16 + torch.randint(0, 16, (rows // 32, C), generator=g)
  x[r, k] = _pm1(g, rows // 32, C)
  # cancelling pairs from a pool of P column pairs, all 2P columns in different chunks
  P = min(8, C // 2)
  used, k1s, k2s = set(), [], []
  def pick(lo, hi):
    while True:
      kk = int(torch.randint(lo, hi, (1,), generator=g))
      if kk // 16 not in used:
        used.add(kk // 16)
        return kk
  for i in range(P):
    if pl.nsplit > 1:
      s1 = i % pl.nsplit
      s2 = (s1 + 1 + (i // pl.nsplit) % (pl.nsplit - 1)) % pl.nsplit
      assert s1 != s2
      k1s.append(pick(*pl.split_range(s1, K)))
      k2s.append(pick(*pl.split_range(s2, K)))
    else:
      k1s.append(pick(0, K))
      k2s.append(pick(0, K))
  k1s, k2s = torch.tensor(k1s), torch.tensor(k2s)
  w[:, :, k2s] = w[:, :, k1s]
  for j in range(min(2, P)):
    idx = torch.randint(0, P, (rows,), generator=g)
    sgn = _pm1(g, rows)
    x[torch.arange(rows), k1s[idx]] = A * sgn
    x[torch.arange(rows), k2s[idx]] = -A * sgn
  c = Case(sp, x, w, extra=dict(pairs=(k1s, k2s)))
  if sp.bias:
    c.bias = torch.randint(1, 65, (N,), generator=g).double() * _pm1(g, N)
  if fp8:
    c.sx = 2.0 ** torch.randint(0, 2, (rows,), generator=g).double()
    c.sw = 2.0 ** -torch.randint(0, 2, (E, N), generator=g).double()
  if sp.op in ("epilogue", "swiglu_epilogue"):
    c.res = torch.randint(-64, 65, (rows, N), generator=g).double()
  if sp.op in ("swiglu", "swiglu_epilogue"):
    # x = silu(gate) * up: gate 32 and up = x / 32 where x != 0; a zero is either
    # gate 0 under a random up or gate 32 over up 0
    gate0 = (x == 0) & (torch.rand(rows, K, generator=g) < 0.5)
    gate = torch.where(gate0, 0.0, 32.0).double()
    up = torch.where(gate0, torch.randint(-128, 129, (rows, K), generator=g).double() / 32, x / 32)
    c.gu = torch.cat([gate, up], dim=1)
    assert torch.equal(c.gu, _bf16(c.gu))
  if sp.op == "mxfp4":
    codes, e8 = ops.quant_mxfp4(w.view(E * N, K).float())
    assert torch.equal(ops.dequant_mxfp4(codes, e8).double(), w.view(E * N, K))  # +-1 dequantizes to itself
  return c


def _e4m3(t):
  return t.float().to(torch.float8_e4m3fn).double()


def _build_real(sp: Spec) -> Case:
  g = torch.Generator().manual_seed(sp.seed)
  M, K, N, E = sp.M, sp.K, sp.N, sp.E
  x = 0.5 * torch.randn(E * M, K, generator=g)
  w = 0.02 * torch.randn(E, N, K, generator=g)
  if sp.op == "glu":
    w *= 4.0  # sums of a few tenths to a few units: silu on both sides of zero
  c = Case(sp, _bf16(x), _bf16(w))
  if sp.bias:
    c.bias = _bf16(0.5 * torch.randn(N, generator=g))
  if sp.op == "fp8":
    c.sx = (c.x.abs().amax(1).float() / 448.0).double()
    c.sw = (c.w.abs().amax(2).float() / 448.0).double()
    c.x = _e4m3((c.x / c.sx[:, None]).clamp(-448, 448))
    c.w = _e4m3((c.w / c.sw[:, :, None]).clamp(-448, 448))
  T = sums(c, c.x.abs(), c.w.abs())
  if sp.op == "fp8":
    T = T * c.sx[:, None] * c.sw.repeat_interleave(M, dim=0)
  c.T = T + (c.bias.abs() if c.bias is not None else 0.0)
  return c


def glu_bound(c: Case):
  sp = c.spec
  I = sp.N // 2
  G, U = c.S[:, :I], c.S[:, I:]
  dG, dU = (_bf16(G) - G).abs(), (_bf16(U) - U).abs()
  if sp.family == "real":
    e = (sp.K + 3) * 2.0 ** -24 * c.T
    dG, dU = dG + e[:, :I] * (1 + 2.0 ** -8), dU + e[:, I:] * (1 + 2.0 ** -8)
  silu = (G * torch.sigmoid(G)).abs()
  ref = c.ref.abs()
  rest = 2.0 ** -24 * (G.abs() + 7) * ref + 1.1 * dG * (U.abs() + dU) + silu * dU + 2.0 ** -126 * (1 + U.abs())
  return 2.0 ** -8 * (ref + rest) + rest


def bound(c: Case):
  """Per-output error bound of a correct kernel: zero for the exact family."""
  sp = c.spec
  if sp.op == "glu":
    return glu_bound(c)
  if sp.family == "exact":
    return torch.zeros_like(c.ref)
  second = (sp.K + sp.plan.nsplit + 2) * 2.0 ** -24 * c.T
  return 2.0 ** -8 * (c.ref.abs() + second) + second


def worst_ratio(c: Case, got) -> float:
  """max |got - ref| / bound (0 where both vanish)."""
  err = (got.double().cpu().reshape(c.ref.shape) - c.ref).abs()
  b = bound(c)
  return float(torch.where(err == 0, torch.zeros_like(err), err / b).max())


def check(c: Case, got):
  """The assertion of the GPU tests: bit equality for exact cases, the bound otherwise."""
  got = got.cpu().reshape(c.ref.shape)
  if c.spec.family == "exact" and c.spec.op != "glu":
    want = c.ref.to(torch.bfloat16)
    if not torch.equal(got, want):
      bad = (got != want).nonzero()
      m, n = (int(v) for v in bad[0])
      raise AssertionError(f"{c.spec.name}: {len(bad)} of {want.numel()} outputs differ, rows {sorted(set(bad[:, 0].tolist()))[:8]} "
                           f"cols {sorted(set(bad[:, 1].tolist()))[:8]}; first ({m}, {n}) got {float(got[m, n])} want {float(want[m, n])}")
    return 0.0
  r = worst_ratio(c, got)
  print(f"{c.spec.name}: nsplit {c.spec.plan.nsplit} worst err/bound {r:.3f}")
  assert r <= 1.0, (c.spec.name, r)
  return r


def launch_args(c: Case):
  """CPU tensors of one launch, in the order the binding of c.spec.op takes them
  (after which come N, bias and the epilogue, see the GPU tests)."""
  sp = c.spec
  bf = lambda t: t.to(torch.bfloat16)
  pack = lambda f, w: torch.stack([f(bf(w[e])) for e in range(sp.E)]) if sp.op == "grouped" else f(bf(w[0]))
  if sp.op == "plain":
    return bf(c.x), bf(c.w[0]).contiguous()
  if sp.op == "glu":
    return bf(c.x), ops.pack_decode_weight_glu(bf(c.w[0]))
  if sp.op in ("swiglu", "swiglu_epilogue"):
    return bf(c.gu), ops.pack_decode_weight(bf(c.w[0]))
  if sp.op == "fp8":
    codes = lambda t: t.float().to(torch.float8_e4m3fn).view(torch.uint8)
    w8 = codes(c.w)
    wp8 = w8.view(sp.E, sp.N // 32, 32, sp.K // 16, 2, 8).permute(0, 1, 3, 4, 2, 5).contiguous()
    return codes(c.x), c.sx.float(), wp8, c.sw.float().reshape(-1).contiguous()
  if sp.op == "mxfp4":
    wq, ws, w_dq = ops.pack_decode_weight_mxfp4(bf(c.w.view(sp.E * sp.N, sp.K)))
    assert torch.equal(w_dq.double(), c.w.view(sp.E * sp.N, sp.K))
    x = bf(c.x)
    return (x.view(sp.E, sp.M, sp.K) if sp.E > 1 else x), wq, ws
  x = bf(c.x)
  return (x.view(sp.E, sp.M, sp.K) if sp.op == "grouped" else x), pack(ops.pack_decode_weight, c.w)


# ---------------------------------------------------------------------------
# Mutations: the reference with one defect each
# ---------------------------------------------------------------------------

def mutations(c: Case):
  """(name, mutated output [rows, out cols], [rows/32, out col tiles] bool mask
  of the output tiles the defect must show in). An output tile is 32 rows by the
  columns of one 32-row weight tile: 32 columns, or 16 under the GLU store,
  whose weight tile j holds gate and up rows of output columns 16j .. 16j+15."""
  sp, pl = c.spec, c.spec.plan
  g = torch.Generator().manual_seed(sp.seed + 1)
  M, K, N, E = sp.M, sp.K, sp.N, sp.E
  rows, I = E * M, N // 2
  glu = sp.op == "glu"
  nwt = N // 32
  ri = lambda n: int(torch.randint(0, n, (1,), generator=g))
  def wcols(j):  # columns of S that weight tile j produces
    if glu:
      return torch.cat([torch.arange(16 * j, 16 * j + 16), I + torch.arange(16 * j, 16 * j + 16)])
    return torch.arange(32 * j, 32 * j + 32)
  def mask(e=None, j=None):
    m = torch.zeros(rows // 32, nwt, dtype=torch.bool)
    m[(slice(None) if e is None else slice(e * M // 32, (e + 1) * M // 32)), (slice(None) if j is None else j)] = True
    return m
  def part(e, cols, ks):
    return c.x[e * M:(e + 1) * M, ks] @ c.w[e][cols][:, ks].T
  out = []
  for tag, ch in (("random", ri(K // 16)), ("last", K // 16 - 1)):
    e, j = ri(E), ri(nwt)
    ks, er = slice(ch * 16, ch * 16 + 16), slice(e * M, (e + 1) * M)
    for name, sign in ((f"chunk dropped ({tag})", -1.0), (f"chunk twice ({tag})", 1.0)):
      S = c.S.clone()
      S[er, wcols(j)] += sign * part(e, wcols(j), ks)
      out.append((name, finish(c, S), mask(e, j)))
  if pl.nsplit > 1:
    s = ri(pl.nsplit)
    out.append(("split dropped", finish(c, c.S - sums(c, ks=slice(*pl.split_range(s, K)))), mask()))
  k0, k1 = pl.split_range(pl.nsplit - 1, K)
  last = k0 + (k1 - k0 - 1) // pl.bk * pl.bk
  out.append(("last K-step dropped", finish(c, c.S - sums(c, ks=slice(last, k1))), mask()))
  e, j = ri(E), ri(nwt)
  S = c.S.clone()
  er = slice(e * M, (e + 1) * M)
  if glu:  # packed rows w and w + 8 of a tile are the gate and up row of one column
    n = 16 * j + ri(16)
    a, b = n, I + n
  else:
    a = 32 * j + 16 * ri(2) + ri(8)
    b = a + 8
  S[er, a], S[er, b] = c.S[er, b], c.S[er, a]
  out.append(("weight rows 8 apart swapped", finish(c, S), mask(e, j)))
  if c.bias is not None:
    out.append(("bias dropped", finish(c, c.S, with_bias=False), mask()))
  # the accumulator rounded to bf16 after each K-step, the partials added in fp32
  # It applies to the m-tiles with a row whose +-A entries do not cancel inside
  # one K-step (always so when K is split; a one-step case has no such row).
  S = torch.zeros_like(c.S)
  big = c.x * (c.x.abs() >= 256)
  open_rows = torch.zeros(rows, dtype=torch.bool)
  for s in range(pl.nsplit):
    k0, k1 = pl.split_range(s, K)
    acc = torch.zeros_like(c.S)
    for k in range(k0, k1, pl.bk):
      ks = slice(k, min(k + pl.bk, k1))
      acc = _bf16(acc + sums(c, ks=ks))
      open_rows |= (big[:, ks].sum(1) != 0) & (k1 - k0 > pl.bk)
    S += acc
  m = mask() & open_rows.view(rows // 32, 32).any(1)[:, None]
  if m.any() or sp.family == "real":
    out.append(("bf16 accumulator", finish(c, S), m))
  return out


# mutations the real family is not meant to see: at K <= 2048 a bf16 accumulator
# moves a sum by a few 2^-8 of its size, which is the size of the bound itself
REAL_BLIND = ("bf16 accumulator",)


def visible(c: Case, mut):
  """[rows, cols] bool: outputs a defect moves by at least one bf16 ulp (exact
  family) or by at least 4x the bound (real family, GLU store)."""
  if c.spec.family == "exact" and c.spec.op != "glu":
    return mut.to(torch.bfloat16) != c.ref.to(torch.bfloat16)
  return (mut - c.ref).abs() >= 4 * bound(c)


def tile_fraction(c: Case, vis):
  """[rows/32, out col tiles]: share of each output tile's outputs that are visible."""
  ct = 16 if c.spec.op == "glu" else 32
  r, n = vis.shape
  return vis.view(r // 32, 32, n // ct, ct).double().mean(dim=(1, 3))


# ---------------------------------------------------------------------------
# The cases of the GPU file (tests/test_gemm_oracle_gpu.py); the CPU file checks
# every one of them for the builder's conditions and the mutation margins.
# ---------------------------------------------------------------------------

def _packed_specs():
  out = []
  for mt in range(1, 9):
    M = 32 * mt
    for bn in ((128, 256) if M >= 128 else (None,)):
      b = mt % 2 == 1  # bias on odd MT here, on even MT in the second block
      kw = dict(op="packed", M=M, bn=bn)
      out += [Spec(K=64, bias=b, **kw), Spec(K=128, bias=not b, **kw),
              # 16 steps at BK=128 (BK=64 on the wide tile at MT >= 7), 32 at BK=64
              Spec(K=2048, bias=not b, **kw), Spec(K=2048, bk64=True, bias=b, **kw),
              # nsplit 2 at BK=128 (16 and 17 steps per split); nsplit 4 at BK=64 (16 and 17)
              Spec(K=4096, target=3, bias=b, **kw), Spec(K=4352, target=3, bias=not b, **kw),
              Spec(K=4096, target=BIG, bias=not b, **kw), Spec(K=4352, target=BIG, bias=b, **kw),
              Spec(K=2112, target=BIG, bias=not b, **kw)]  # nsplit 2, kc 1088 + a ragged 1024
      # an odd step count, unsplit: the last step is the one after the two-step loop and its
      # MFMAs run straight into the store, whose read order depends on the bias. 3 steps at
      # BK=64, 17 at BK=128, 34 and 33 at BK=64
      for bias in (False, True):
        out += [Spec(K=192, bias=bias, **kw), Spec(K=2176, bias=bias, **kw),
                Spec(K=2176, bk64=True, bias=bias, **kw), Spec(K=2112, bk64=True, bias=bias, **kw)]
  for M in (32, 128, 256):  # N that stays on the narrow tile
    for N in (128, 384):
      out += [Spec("packed", M, 2176, N, bias=True), Spec("packed", M, 4352, N, target=BIG),
              Spec("packed", M, 192, N)]
  out.append(Spec("packed", 32, 16384, 128, target=BIG, bias=True))  # nsplit 16
  return out


def _reduced_specs():
  out = []
  for M in (32, 128, 256):
    # unpacked kernel: 64-wide steps and 16-wide tail steps; kc is 16-aligned
    out += [Spec("plain", M, 2048, bias=True), Spec("plain", M, 2096), Spec("plain", M, 2096, bias=True), Spec("plain", M, 4096, target=BIG),
            Spec("plain", M, 4416, target=BIG, bias=True), Spec("plain", M, 48)]  # kc 1104 = 17 * 64 + 16
    out += [Spec("xreg", M, 2048), Spec("xreg", M, 2112, bias=True), Spec("xreg", M, 2112), Spec("xreg", M, 64),
            Spec("xreg", M, 4096, target=BIG, bias=True), Spec("xreg", M, 4352, target=BIG)]
    bn = 256 if M >= 128 else None
    out += [Spec("grouped", M, 2048, E=3, bn=bn), Spec("grouped", M, 2176, E=3, bn=bn),
            Spec("grouped", M, 4096, E=3, target=BIG, bn=bn), Spec("grouped", M, 4352, E=3, target=BIG, bn=bn),
            Spec("grouped", M, 192, 128, E=3)]
    for op in ("epilogue", "swiglu_epilogue"):
      out += [Spec(op, M, 2176, bias=True, bn=bn), Spec(op, M, 2176, bn=bn), Spec(op, M, 4352, target=BIG, bias=True, bn=bn),
              Spec(op, M, 4096, target=3, bn=bn)]
    out += [Spec("swiglu", M, 192, bn=bn), Spec("swiglu", M, 2176, bias=True, bn=bn), Spec("swiglu", M, 2176, bn=bn),
            Spec("swiglu", M, 2176, bk64=True, bn=bn), Spec("swiglu", M, 4352, target=BIG, bn=bn),
            Spec("swiglu", M, 4352, target=3, bias=True, bn=bn)]
    for bn in ((128, 256) if M >= 128 else (None,)):
      for K in (2048, 2176, 4224):
        out += [Spec("glu", M, K, bn=bn), Spec("glu", M, K, bn=bn, bk64=True)]
      out.append(Spec("glu", M, 192, bn=bn))
    out += [Spec("fp8", M, 2048, bias=True), Spec("fp8", M, 2112), Spec("fp8", M, 2112, bias=True), Spec("fp8", M, 64),
            Spec("fp8", M, 4096, target=BIG), Spec("fp8", M, 4352, target=BIG, bias=True),
            Spec("fp8", M, 2112, 128, E=3), Spec("fp8", M, 4352, 128, E=3, target=BIG)]
  out += [Spec("mxfp4", 32, 2176, bias=True), Spec("mxfp4", 32, 2176), Spec("mxfp4", 128, 2112, bias=True), Spec("mxfp4", 128, 4352, target=BIG, bn=256),
          Spec("mxfp4", 256, 2304, 128, E=3, bk64=True),  # 36 steps at BK=64: the ring of 4 leaves none over
          Spec("mxfp4", 64, 2112, 128, E=3)]              # 33 steps: one left over
  return out


def _real_specs():
  out = []
  for M in (32, 128, 256):
    bn = 256 if M >= 128 else None
    # K <= 256 cannot split (the plan keeps 1024 per split): the split cases run
    # the smallest K that splits, under the same bound
    out += [Spec("packed", M, 256, bias=True, bn=bn, family="real"),
            Spec("packed", M, 192, bn=bn, family="real"),
            Spec("packed", M, 2048, target=BIG, bias=True, bn=bn, family="real"),
            Spec("fp8", M, 256, bias=True, family="real"),
            Spec("fp8", M, 2048, target=BIG, family="real"),
            Spec("glu", M, 256, bn=bn, family="real"), Spec("glu", M, 192, bn=bn, family="real")]
  return out


SPECS = _packed_specs() + _reduced_specs() + _real_specs()
assert len({s.name for s in SPECS}) == len(SPECS)
