// xotorch_amd CDNA4 (gfx950 / MI355X) kernels for the transformer hot path.
//
// These replace the ops the reference delegates to torchtune
// (SURVEY.md §2.2 op table; reference call sites cited per kernel below):
//   - fused residual-add + RMSNorm      (llm_utils.py:465-476)
//   - fused RoPE rotate + KV-cache append, dual layout (general_mha.py:78-106)
//   - GQA attention, prefill AND decode, on matrix cores
//     (general_mha.py:211-226): flash-forward / flash-decoding with online
//     softmax, v_mfma_f32_16x16x32_bf16 for scores and PV, streaming an
//     MFMA-fragment-packed KV cache with coalesced 1 KB wave loads
//   - decode projections (qkv/o/gate_up/down/lm_head, general_mha.py:83-102,
//     llm_utils.py:491-500): weight-streaming split-K GEMMs on
//     v_mfma_f32_32x32x16_bf16 over prepacked weight fragments (non-temporal
//     loads; a grouped variant runs every MoE expert in one launch, and a
//     W8A8 e4m3 variant halves the stream) — auto-picked per shape against
//     TunableOp-tuned hipBLASLt at runtime
//   - SwiGLU activation                  (llm_utils.py:491-500)
//
// Design notes (per /opt/skills/guides/cdna_hip_programming.md):
//   * wave = 64 lanes; all block sizes are multiples of 64
//   * bf16 is loaded vectorized (ushort8 = 16 B per lane); the big streamed
//     operands (weights, KV) are pre-shuffled ONCE into MFMA fragment order
//     so every hot-loop load is a coalesced wave-wide 1 KB stream
//     (fragment-shaped 16 B gathers measured TA-bound at ~2 TB/s vs 5.5)
//   * everything is launch-shape-static so the whole decode step can be
//     captured in a hipGraph (lengths come from device tensors)
//
// Prefill projections (compute-bound) stay on hipBLASLt through torch —
// plain library GEMMs per the MI355X build rules; measured ~1.6 PF there.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include <cstring>
#include <vector>

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float floatx16;
typedef __attribute__((ext_vector_type(4))) float floatx4;
typedef __attribute__((ext_vector_type(4))) unsigned int uintx4;

typedef __attribute__((ext_vector_type(8))) unsigned short ushort8;
typedef __attribute__((ext_vector_type(4))) unsigned short ushort4_t;

#define DEVINL __device__ __forceinline__

DEVINL float b2f(unsigned short u) {
  union { float f; unsigned int i; } v;
  v.i = ((unsigned int)u) << 16;
  return v.f;
}

DEVINL unsigned short f2b(float f) {
  __hip_bfloat16 h = __float2bfloat16(f);  // round-to-nearest-even
  return *reinterpret_cast<unsigned short*>(&h);
}

// ---------------------------------------------------------------------------
// Device helpers shared by the norm, KV-append and attention kernels
// ---------------------------------------------------------------------------

// 64-lane xor-butterfly reductions; every lane ends with the wave's value
DEVINL float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

DEVINL float wave_max(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}

// MFMA-fragment-packed KV cache — the ONE definition of the two layouts
// (the tests' _pack_k / _pack_v / _mla_pack_ref state them independently).
// A fragment is 64 lanes x 8 elements (bf16, or e4m3 bytes in fp8 mode) and is
// what one v_mfma_f32_16x16x32 B operand reads: the attention kernels stream
// it lane-linearly (lane * 8), one coalesced wave load per fragment.
//   K image of a head: [pos>>4][d>>5][lane][d&7],  lane = ((d&31)>>3)*16 + (pos&15)
//     a 16-position tile holds dims/32 fragments: hd/32 for GQA (4 at hd=128,
//     8 at hd=256), 18 for MLA
//   V image of a head: [d>>4][pos>>5][lane][pos&7], lane = ((pos&31)>>3)*16 + (d&15)
//     one fragment per (16-dim group, 32-position tile): hd/16 groups GQA
//     (8 at hd=128, 16 at hd=256), 32 MLA
// The GQA kernels take the packed layouts at hd in {128, 256} (GQA_PACKED_HD).
constexpr int FRAG = 512;  // elements per fragment
constexpr bool GQA_PACKED_HD(int hd) { return hd == 128 || hd == 256; }
constexpr int GQA_KTILE(int hd) { return (hd >> 5) * FRAG; }  // one 16-position K tile
constexpr int GQA_VGROUPS(int hd) { return hd >> 4; }         // 16-dim V groups

// offset of (dim d, position pos) inside its 16-position K tile
DEVINL size_t kfrag_off(int d, int pos) {
  return (size_t)(d >> 5) * FRAG + (((d & 31) >> 3) * 16 + (pos & 15)) * 8 + (d & 7);
}

// offset of (dim d, position pos) inside a head's V image of tiles32 32-position tiles
DEVINL size_t vfrag_off(int d, int pos, int tiles32) {
  return ((size_t)(d >> 4) * tiles32 + (pos >> 5)) * FRAG + (((pos & 31) >> 3) * 16 + (d & 15)) * 8 + (pos & 7);
}

// OCP e4m3 quantization: scale = amax / 448 (floored so 1/scale is finite)
DEVINL float e4m3_scale(float amax) { return fmaxf(amax, 1e-12f) / 448.f; }

DEVINL unsigned short to_e4m3x2(float a, float b) {
  return (unsigned short)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
}

DEVINL unsigned char to_e4m3(float v) { return (unsigned char)(to_e4m3x2(v, 0.f) & 0xff); }

// 8 bf16 (one MFMA fragment, or 16 B of a row) times inv -> 8 e4m3 bytes
DEVINL long to_e4m3x8(bf16x8 v, float inv) {
  unsigned char o[8];
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const unsigned short pk = to_e4m3x2((float)v[j] * inv, (float)v[j + 1] * inv);
    o[j] = (unsigned char)(pk & 0xff);
    o[j + 1] = (unsigned char)(pk >> 8);
  }
  return *reinterpret_cast<const long*>(o);
}

// positions: [S] (shared across batch) or [B*S] (per-row — continuous
// batching where every slot decodes at its own position); bs = b * S + s
DEVINL int row_position(const int* __restrict__ positions, int npos, int B, int S, int bs) {
  return positions[(npos == B * S && npos != S) ? bs : bs % S];
}

// HF rotate-half on one (x1, x2) pair -> (r1, r2) = (x1 c - x2 s, x2 c + x1 s)
DEVINL void rope_pair(float x1, float x2, float c, float sn, float& r1, float& r2) {
  r1 = x1 * c - x2 * sn;
  r2 = x2 * c + x1 * sn;
}

// ---------------------------------------------------------------------------
// RMSNorm (optionally fused with residual add)
// one workgroup per row; 256 threads; row cached in registers between the
// two passes (up to 8 chunks of 8 bf16 per thread -> D <= 16384)
// ---------------------------------------------------------------------------

template <bool RESIDUAL>
__global__ __launch_bounds__(256) void rmsnorm_kernel(
    const unsigned short* __restrict__ x, const unsigned short* __restrict__ res,
    const unsigned short* __restrict__ w, unsigned short* __restrict__ out,
    unsigned short* __restrict__ res_out, int D, float eps, float w_bias) {
  const int row = blockIdx.x;
  const size_t off = (size_t)row * D;
  float vals[64];
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int i = threadIdx.x * 8 + c * 256 * 8;
    if (i < D) {
      ushort8 v = *(const ushort8*)(x + off + i);
      if (RESIDUAL) {
        ushort8 r = *(const ushort8*)(res + off + i);
        ushort8 s;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = b2f(v[j]) + b2f(r[j]);
          vals[c * 8 + j] = f;
          s[j] = f2b(f);
          acc += f * f;
        }
        *(ushort8*)(res_out + off + i) = s;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = b2f(v[j]);
          vals[c * 8 + j] = f;
          acc += f * f;
        }
      }
    }
  }
  // wave reduce then cross-wave through LDS
  acc = wave_sum(acc);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  const float total = red[0] + red[1] + red[2] + red[3];
  const float inv = rsqrtf(total / (float)D + eps);
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int i = threadIdx.x * 8 + c * 256 * 8;
    if (i < D) {
      ushort8 wv = *(const ushort8*)(w + i);
      ushort8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2b(vals[c * 8 + j] * inv * (b2f(wv[j]) + w_bias));
      *(ushort8*)(out + off + i) = o;
    }
  }
}

// ---------------------------------------------------------------------------
// Fused RoPE (HF rotate-half) + KV-cache append, on the PACKED qkv tensor
// (one fused QKV GEMM writes [B, S, (H+2*KVH)*hd]; this kernel rotates the
// q heads in place, rotates k heads into the cache, copies v heads into the
// cache — no separate q/k/v tensors ever materialize).
// one wave per (b, s, head-slot); cache layout [B, KVH, T, hd];
// cos/sin tables fp32 [maxT, hd/2].
// ---------------------------------------------------------------------------

// When the MFMA-packed cache copies exist (kpc/vpc non-null, hd 128 or 256)
// the same kernel also appends into them (decode attention then streams the
// cache as coalesced v_mfma_f32_16x16x32_bf16 B-fragments), per (b, kv-head)
// in the kfrag_off / vfrag_off layouts:
//   K_packed [B,KVH][T32/16 tile][hd/32 hd-chunk][64 lane][8]
//   V_packed [B,KVH][hd/16 hd-group][T32/32 tile][64 lane][8]
// A wave owns hd/2 rotate pairs: PAIRS = 1 per lane up to hd = 128, 2 at
// hd <= 256 (pair e of a lane is dims p, p + hd/2 with p = lane + 64 e; the V
// copy moves dims 128 e + 2 lane, + 1).
// Optional qwen3 per-head q/k RMSNorm (qn/kn weights [hd], fused before the
// rotation): the slot's wave reduces sum-of-squares over the head row, then
// scales while rotating.
// fp8 packed mode (kp8 non-null): the packed copies are OCP e4m3 bytes with
// per-row scales sk/sv [B*KVH*T32] — half the decode stream and ~60% of the
// dual-cache residency (plain cache stays bf16 for prefill). XOT_FP8_KV=1.

// this lane's rotated pairs (pair e: dims p, p + hd/2, p = lane + 64 e) of one
// q or k head row, after the optional per-head RMSNorm (w non-null) over the
// whole row; pairs with p >= hd/2 get 0
template <int PAIRS>
DEVINL void rope_head_pair(const unsigned short* row, const unsigned short* __restrict__ w,
                           const float* __restrict__ cosb, const float* __restrict__ sinb,
                           int pos, int hd, int lane, float eps, float (&f1)[PAIRS], float (&f2)[PAIRS]) {
  const int hd2 = hd >> 1;
  float x1[PAIRS], x2[PAIRS];
#pragma unroll
  for (int e = 0; e < PAIRS; ++e) {
    const int p = lane + e * 64;
    x1[e] = x2[e] = 0.f;
    if (p < hd2) {
      x1[e] = b2f(row[p]);
      x2[e] = b2f(row[p + hd2]);
    }
  }
  if (w) {
    float ss = x1[0] * x1[0] + x2[0] * x2[0];
#pragma unroll
    for (int e = 1; e < PAIRS; ++e) ss += x1[e] * x1[e] + x2[e] * x2[e];
    const float inv = rsqrtf(wave_sum(ss) / (float)hd + eps);
#pragma unroll
    for (int e = 0; e < PAIRS; ++e) {
      const int p = lane + e * 64;
      if (p < hd2) {
        x1[e] *= inv * b2f(w[p]);
        x2[e] *= inv * b2f(w[p + hd2]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < PAIRS; ++e) {
    const int p = lane + e * 64;
    const bool on = p < hd2;
    rope_pair(x1[e], x2[e], on ? cosb[(size_t)pos * hd2 + p] : 0.f,
              on ? sinb[(size_t)pos * hd2 + p] : 0.f, f1[e], f2[e]);
  }
}

template <int PAIRS>
__global__ __launch_bounds__(256) void rope_qkv_append_kernel(
    unsigned short* __restrict__ qkv, const float* __restrict__ cosb,
    const float* __restrict__ sinb, const int* __restrict__ positions,
    unsigned short* __restrict__ kc, unsigned short* __restrict__ vc,
    int B, int S, int H, int KVH, int hd, int T,
    unsigned short* __restrict__ kpc, unsigned short* __restrict__ vpc, int T32,
    const unsigned short* __restrict__ qn, const unsigned short* __restrict__ kn,
    float norm_eps, int npos,
    unsigned char* __restrict__ kp8, unsigned char* __restrict__ vp8,
    float* __restrict__ sk, float* __restrict__ sv) {
  const int wid = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int slots = H + 2 * KVH;
  if (wid >= B * S * slots) return;
  const int slot = wid % slots;
  const int bs = wid / slots;
  const int b = bs / S;
  const int pos = row_position(positions, npos, B, S, bs);
  const int hd2 = hd >> 1;
  unsigned short* row = qkv + ((size_t)bs * slots + slot) * hd;
  if (slot < H) {
    float f1[PAIRS], f2[PAIRS];
    rope_head_pair(row, qn, cosb, sinb, pos, hd, lane, norm_eps, f1, f2);
#pragma unroll
    for (int e = 0; e < PAIRS; ++e) {
      const int p = lane + e * 64;
      if (p < hd2) {
        row[p] = f2b(f1[e]);
        row[p + hd2] = f2b(f2[e]);
      }
    }
  } else if (slot < H + KVH) {
    const size_t head = (size_t)(b * KVH + (slot - H));
    float f1[PAIRS], f2[PAIRS];
    rope_head_pair(row, kn, cosb, sinb, pos, hd, lane, norm_eps, f1, f2);
    const size_t ktile = (head * (T32 >> 4) + (pos >> 4)) * GQA_KTILE(hd);
    // kc / vc null: a packed-only cache, there is no plain copy to write
    unsigned short* dst = kc ? kc + (head * T + pos) * hd : nullptr;
    float mx = 0.f;
#pragma unroll
    for (int e = 0; e < PAIRS; ++e) {
      const int p = lane + e * 64;
      mx = fmaxf(mx, fmaxf(fabsf(f1[e]), fabsf(f2[e])));
      if (p < hd2) {
        if (dst) {
          dst[p] = f2b(f1[e]);
          dst[p + hd2] = f2b(f2[e]);
        }
        if (kpc) {
          kpc[ktile + kfrag_off(p, pos)] = f2b(f1[e]);
          kpc[ktile + kfrag_off(p + hd2, pos)] = f2b(f2[e]);
        }
      }
    }
    if (kp8) {
      const float scl = e4m3_scale(wave_max(mx));
      const float inv = 1.f / scl;
      if (lane == 0) sk[head * T32 + pos] = scl;
#pragma unroll
      for (int e = 0; e < PAIRS; ++e) {
        const int p = lane + e * 64;
        if (p < hd2) {
          kp8[ktile + kfrag_off(p, pos)] = to_e4m3(f1[e] * inv);
          kp8[ktile + kfrag_off(p + hd2, pos)] = to_e4m3(f2[e] * inv);
        }
      }
    }
  } else {
    const size_t head = (size_t)(b * KVH + (slot - H - KVH));
    unsigned short* dst = vc ? vc + (head * T + pos) * hd : nullptr;
    const size_t vhead = head * GQA_VGROUPS(hd) * (T32 >> 5) * FRAG;
    float mx = 0.f;
#pragma unroll
    for (int e = 0; e < PAIRS; ++e) {
      const int d = e * 128 + lane * 2;
      if (d < hd) {
        if (dst) *(unsigned int*)(dst + d) = *(const unsigned int*)(row + d);
        mx = fmaxf(mx, fmaxf(fabsf(b2f(row[d])), fabsf(b2f(row[d + 1]))));
        if (vpc) {
#pragma unroll
          for (int j = 0; j < 2; ++j) vpc[vhead + vfrag_off(d + j, pos, T32 >> 5)] = row[d + j];
        }
      }
    }
    if (vp8) {
      const float scl = e4m3_scale(wave_max(mx));
      const float inv = 1.f / scl;
      if (lane == 0) sv[head * T32 + pos] = scl;
#pragma unroll
      for (int e = 0; e < PAIRS; ++e) {
        const int d = e * 128 + lane * 2;
        if (d < hd) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
            vp8[vhead + vfrag_off(d + j, pos, T32 >> 5)] = to_e4m3(b2f(row[d + j]) * inv);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// GQA decode attention (flash-decoding): split-KV partials + merge.
//
// partial kernel: grid = B * KVH * NSPLIT workgroups, 256 threads = 4 waves
// = 16 groups of 16 lanes. Each group walks cache positions with stride 16;
// a group handles one position per step: 16 lanes x 16 B = one 256 B KV row
// (hd=128) coalesced. All NQ = H/KVH query heads of this kv-head are scored
// in the same pass (KV bytes read once per kv-head). Online softmax per
// (group, head); group partials merged through LDS; one (m, l, o[hd]) fp32
// partial per (b, qh, split) written to the workspace.
// ---------------------------------------------------------------------------

// merge of the split-KV partials (VALU, MFMA and MLA decode): one workgroup
// per (b, head), 128 threads (256 at HD 256 and 512), HD / threads dims per thread
template <int HD>
__global__ __launch_bounds__(HD > 128 ? 256 : 128) void attn_decode_merge(
    const float* __restrict__ ws_o, const float* __restrict__ ws_ml,
    unsigned short* __restrict__ out, int nsplit) {
  constexpr int NT = HD > 128 ? 256 : 128;
  const int bh = blockIdx.x;  // b * H + qh
  if (HD <= NT && threadIdx.x >= HD) return;
  float M = -INFINITY;
  for (int i = 0; i < nsplit; ++i) M = fmaxf(M, ws_ml[((size_t)bh * nsplit + i) * 2 + 0]);
#pragma unroll
  for (int e = 0; e < (HD + NT - 1) / NT; ++e) {
    const int d = threadIdx.x + e * NT;
    float L = 0.f, O = 0.f;
    for (int i = 0; i < nsplit; ++i) {
      const float lg = ws_ml[((size_t)bh * nsplit + i) * 2 + 1];
      const float alpha = (lg > 0.f) ? __expf(ws_ml[((size_t)bh * nsplit + i) * 2 + 0] - M) : 0.f;
      L += alpha * lg;
      O += alpha * ws_o[((size_t)bh * nsplit + i) * HD + d];
    }
    out[(size_t)bh * HD + d] = f2b(L > 0.f ? O / L : 0.f);
  }
}

template <int NQ, int HD>
__global__ __launch_bounds__(256) void attn_decode_partial(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ kc,
    const unsigned short* __restrict__ vc, const int* __restrict__ seq_lens,
    float* __restrict__ ws_o, float* __restrict__ ws_ml,
    int B, int H, int KVH, int T, int nsplit, int qh0, float scale, long long q_stride) {
  constexpr int EPL = HD / 16;  // bf16 elements per lane (8 @128, 4 @64)
  const int blk = blockIdx.x;
  const int split = blk % nsplit;
  const int t1 = blk / nsplit;
  const int kvh = t1 % KVH;
  const int b = t1 / KVH;
  const int sl = seq_lens[b];
  const int chunk = (T + nsplit - 1) / nsplit;  // capacity-static (graph-safe)
  const int c0 = split * chunk;
  const int c1 = min(c0 + chunk, sl);
  const int lane = threadIdx.x & 63;
  const int gl = lane & 15;
  const int group = (threadIdx.x >> 6) * 4 + (lane >> 4);  // 0..15

  const int qh_base = kvh * (H / KVH) + qh0;
  float qreg[NQ][EPL];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const unsigned short* qp = q + ((size_t)b * q_stride + (qh_base + n) * HD + gl * EPL);
#pragma unroll
    for (int e = 0; e < EPL; ++e) qreg[n][e] = b2f(qp[e]) * scale;
  }

  float m[NQ], l[NQ], oacc[NQ][EPL];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    m[n] = -INFINITY;
    l[n] = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) oacc[n][e] = 0.f;
  }

  const size_t cache_base = ((size_t)(b * KVH + kvh)) * T * HD;
  for (int t = c0 + group; t < c1; t += 16) {
    float kf[EPL], vf[EPL];
    {
      const unsigned short* kr = kc + cache_base + (size_t)t * HD + gl * EPL;
      const unsigned short* vr = vc + cache_base + (size_t)t * HD + gl * EPL;
      if constexpr (EPL == 8) {
        ushort8 kv8 = *(const ushort8*)kr;
        ushort8 vv8 = *(const ushort8*)vr;
#pragma unroll
        for (int e = 0; e < 8; ++e) { kf[e] = b2f(kv8[e]); vf[e] = b2f(vv8[e]); }
      } else {
        ushort4_t kv4 = *(const ushort4_t*)kr;
        ushort4_t vv4 = *(const ushort4_t*)vr;
#pragma unroll
        for (int e = 0; e < 4; ++e) { kf[e] = b2f(kv4[e]); vf[e] = b2f(vv4[e]); }
      }
    }
    float dot[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) d += qreg[n][e] * kf[e];
      dot[n] = d;
    }
    // reduce the dot across the 16-lane group (xor masks < 16 stay in-group)
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
#pragma unroll
      for (int mm = 8; mm > 0; mm >>= 1) dot[n] += __shfl_xor(dot[n], mm);
    }
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      const float s = dot[n];
      const float mn = fmaxf(m[n], s);
      const float alpha = (l[n] > 0.f) ? __expf(m[n] - mn) : 0.f;
      const float p = __expf(s - mn);
      l[n] = l[n] * alpha + p;
#pragma unroll
      for (int e = 0; e < EPL; ++e) oacc[n][e] = oacc[n][e] * alpha + p * vf[e];
      m[n] = mn;
    }
  }

  // merge the 16 group-partials through LDS -> one partial per (head, split)
  __shared__ float lds_o[16 * NQ * HD];
  __shared__ float lds_ml[16 * NQ * 2];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) lds_o[(group * NQ + n) * HD + gl * EPL + e] = oacc[n][e];
    if (gl == 0) {
      lds_ml[(group * NQ + n) * 2 + 0] = m[n];
      lds_ml[(group * NQ + n) * 2 + 1] = l[n];
    }
  }
  __syncthreads();
  // 256 threads; HD (<=128) of them combine the 16 groups per head
  for (int n = 0; n < NQ; ++n) {
    const int d = threadIdx.x;
    if (d < HD) {
      float M = -INFINITY;
#pragma unroll
      for (int g = 0; g < 16; ++g) M = fmaxf(M, lds_ml[(g * NQ + n) * 2 + 0]);
      float L = 0.f, O = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const float lg = lds_ml[(g * NQ + n) * 2 + 1];
        const float alpha = (lg > 0.f) ? __expf(lds_ml[(g * NQ + n) * 2 + 0] - M) : 0.f;
        L += alpha * lg;
        O += alpha * lds_o[(g * NQ + n) * HD + d];
      }
      const int qh = qh_base + n;
      const size_t pidx = ((size_t)(b * H + qh) * nsplit + split);
      ws_o[pidx * HD + d] = O;
      if (d == 0) {
        ws_ml[pidx * 2 + 0] = M;
        ws_ml[pidx * 2 + 1] = L;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// MFMA flash-decoding attention (HD = 128 or 256): scores and PV on matrix cores.
//
// One WAVE per (b, kv-head, kv-split); the wave's all NQ (<=16) query heads
// are scored together: per 32-position tile,
//   scores[16q][32p] = 2 x (HD/32 x v_mfma_f32_16x16x32_bf16)  (Q fragments resident,
//                      K streamed from the packed cache as coalesced 1 KB loads)
//   online softmax row stats via 4 shfl_xor over the 16-lane column groups
//   P -> bf16 A-fragments through a 96 B-stride LDS image (conflict-free)
//   out[16q][HD] += HD/16 x v_mfma_f32_16x16x32_bf16 (V streamed packed)
// No cross-wave barriers in the position loop (per-wave LDS slice), so ragged
// per-batch lengths cannot deadlock. With nsplit <= 4 the workgroup merges its
// own splits after one barrier that every wave reaches (attn_merge_in_workgroup);
// otherwise partials go to the same (m, l, o) workspace as the VALU kernel and
// are merged by attn_decode_merge<HD> (256 threads x 1 dim at HD = 256).
// Replaces the torchtune cached-decode step (reference general_mha.py:211-215);
// the VALU split-KV kernel above stays as the hd=64 / unpacked-cache path.
// ---------------------------------------------------------------------------

// MFMA operand fragment of the packed cache, keyed on the fp8 mode: register
// type, element type of the stream it is loaded from, and the 16x16x32 MFMA
template <bool FP8>
struct Frag {
  using T = bf16x8;
  using E = unsigned short;
  static DEVINL floatx4 mfma(T a, T b, floatx4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};

template <>
struct Frag<true> {
  using T = long;
  using E = unsigned char;
  static DEVINL floatx4 mfma(T a, T b, floatx4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0);
  }
};

template <bool FP8>
DEVINL typename Frag<FP8>::T frag_load(const typename Frag<FP8>::E* p) {
  return *reinterpret_cast<const typename Frag<FP8>::T*>(p);
}

template <bool FP8>
DEVINL typename Frag<FP8>::T frag_load_nt(const typename Frag<FP8>::E* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const typename Frag<FP8>::T*>(p));
}

// The online-softmax step over one 32-position tile of the GQA decode kernel.
// In: sc0, sc1 = the two masked, scaled 16-column half-tiles of scores (this
// lane's 4 rows r, its column lane & 15). Out: p in sc0 / sc1, updated running
// max m and sum lsum, and alpha = the rescale of everything accumulated before
// this tile. Every decode tile has a visible position, so no row is all -inf.
// The prefill and MLA kernels keep their own copy of these lines (prefill
// with its all-masked-row guard): called through this helper, LLVM promotes
// the by-reference arrays as vectors and schedules their main loops
// differently, which measured 1-2% slower there.
DEVINL void attn_softmax_tile(floatx4& sc0, floatx4& sc1, float (&m)[4], float (&lsum)[4], float (&alpha)[4]) {
  float rmax[4], rsum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) rmax[r] = fmaxf(sc0[r], sc1[r]);
#pragma unroll
  for (int mm = 1; mm < 16; mm <<= 1)
#pragma unroll
    for (int r = 0; r < 4; ++r) rmax[r] = fmaxf(rmax[r], __shfl_xor(rmax[r], mm));
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float mn = fmaxf(m[r], rmax[r]);
    alpha[r] = (lsum[r] > 0.f) ? __expf(m[r] - mn) : 0.f;
    m[r] = mn;
    const float p0 = __expf(sc0[r] - mn);
    const float p1 = __expf(sc1[r] - mn);
    sc0[r] = p0;
    sc1[r] = p1;
    rsum[r] = p0 + p1;
  }
#pragma unroll
  for (int mm = 1; mm < 16; mm <<= 1)
#pragma unroll
    for (int r = 0; r < 4; ++r) rsum[r] += __shfl_xor(rsum[r], mm);
#pragma unroll
  for (int r = 0; r < 4; ++r) lsum[r] = lsum[r] * alpha[r] + rsum[r];
}

// acco (NG 16-dim output groups) *= alpha[row] * f
template <int NG>
DEVINL void attn_rescale(floatx4 (&acco)[NG], const float (&alpha)[4], float f) {
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) acco[g][r] *= alpha[r] * f;
}

// fp8 PV running scale: s_pv = the V-scale ceiling of the tile's positions
// below vend, the tile's visible end; acco is kept in units of 1/R so the
// quantized P' = p * s_v[pos] / s_pv enters at full e4m3 range. Positions from
// vend on carry p = 0 and stay out of the maximum: past the sequence length a
// fresh cache holds scale 1.0, about 250 times a real scale, which would push
// every P' of the last tile below e4m3's smallest normal. vs = this head's
// per-position V scales. Returns s_pv, sets rfac (the factor that moves acco
// from the old R to the new) and R.
DEVINL float attn_fp8_pv_scale(const float* __restrict__ vs, int t, int vend, int lane, float& R, float& rfac) {
  const int pos = t + (lane & 31);
  const float s_pv = fmaxf(wave_max(pos < vend ? vs[pos] : 0.f), 1e-12f);
  rfac = R / s_pv;
  R = s_pv;
  return s_pv;
}

// P -> LDS image (16 rows x 32 positions, 48-element row stride: 96 B for
// bf16, conflict-free b128 reads) and back as the PV MFMA's A fragment
// [row = lane & 15][k = (lane >> 4) * 8 + j]. FP8 stores p * s_v[pos] / s_pv
// as e4m3 bytes (vs / s_pv / vend as in attn_fp8_pv_scale; unused otherwise);
// from vend on it stores 0 without reading the scale, whatever lies there.
// GQA decode kernel only: the prefill and MLA kernels store through their own
// LDS pointer — passed through a parameter, LLVM resolves the LDS address
// space later and their loops came out 1-26% slower.
template <bool FP8>
DEVINL typename Frag<FP8>::T attn_p_fragment(unsigned short* plds, const floatx4 (&sc)[2], int lane,
                                             const float* __restrict__ vs, int t, int vend, float s_pv) {
  typename Frag<FP8>::E* pl = reinterpret_cast<typename Frag<FP8>::E*>(plds);
  const int col = lane & 15;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    float svv = 1.f;
    if constexpr (FP8) svv = (t + h * 16 + col < vend) ? vs[t + h * 16 + col] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ((lane >> 4) * 4 + r) * 48 + h * 16 + col;
      if constexpr (FP8) pl[i] = to_e4m3(sc[h][r] * svv / s_pv);
      else pl[i] = f2b(sc[h][r]);
    }
  }
  return frag_load<FP8>(pl + col * 48 + (lane >> 4) * 8);
}

// split-KV epilogue: the wave's 16 query rows (nq of them real, heads
// bh0 .. bh0 + nq - 1 with bh = b * H + head) each store one fp32
// (m, l, o[NG * 16]) partial for this split; oscale undoes the fp8 R units.
template <int NG>
DEVINL void attn_store_partial(float* __restrict__ ws_o, float* __restrict__ ws_ml,
                               const floatx4 (&acco)[NG], const float (&m)[4], const float (&lsum)[4],
                               int lane, int nq, int bh0, int nsplit, int split, float oscale) {
  const int col = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = (lane >> 4) * 4 + r;
    if (qrow < nq) {
      const size_t pidx = ((size_t)(bh0 + qrow) * nsplit + split);
#pragma unroll
      for (int g = 0; g < NG; ++g) ws_o[pidx * (NG * 16) + g * 16 + col] = acco[g][r] * oscale;
      if (col == 0) {
        ws_ml[pidx * 2 + 0] = m[r];
        ws_ml[pidx * 2 + 1] = lsum[r];
      }
    }
  }
}

// In-workgroup split-KV merge (nsplit in {1, 2, 4}): the 4 / nsplit
// (b, kv-head) groups of a workgroup hold every split of their rows, so the
// waves exchange their partials through LDS and write final bf16 rows — no
// workspace round trip, no merge launch. A wave's slab is 16 query rows of
// ATTN_MROW(hd) = hd + 4 floats: o[hd], then m and l in the pad; 4 * 132 and
// 4 * 260 = 16 (mod 32) keep the four row groups of a store on distinct
// banks. The slab starts at the wave's own P image, which is dead once its
// position loop has ended, so the one barrier below is the only
// synchronisation needed.
// The arithmetic and the split order are attn_decode_merge's, term for term:
// the result is bit-identical to the workspace path.
constexpr int ATTN_MROW(int hd) { return hd + 4; }
constexpr int ATTN_MSLAB(int hd) { return 16 * ATTN_MROW(hd); }

template <int NG>
DEVINL void attn_merge_in_workgroup(float* __restrict__ lds, unsigned short* __restrict__ out,
                                    const floatx4 (&acco)[NG], const float (&m)[4], const float (&lsum)[4],
                                    int wv, int lane, int nq, int bh0, int nsplit, float oscale, bool live) {
  constexpr int HD = NG * 16, MROW = ATTN_MROW(HD), MSLAB = ATTN_MSLAB(HD);
  static_assert(GQA_PACKED_HD(HD), "merge slab rows hold 128 or 256 dims");
  const int col = lane & 15;
  float* mine = lds + wv * MSLAB;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = (lane >> 4) * 4 + r;
    if (live && qrow < nq) {
#pragma unroll
      for (int g = 0; g < NG; ++g) mine[qrow * MROW + g * 16 + col] = acco[g][r] * oscale;
      if (col == 0) {
        mine[qrow * MROW + HD] = m[r];
        mine[qrow * MROW + HD + 1] = lsum[r];
      }
    }
  }
  __syncthreads();
  if (!live) return;
  // the group's nsplit waves share its nq rows; a lane owns dims 2*lane,
  // 2*lane+1 of every 128-dim half
  const int split = wv % nsplit;
  const float* grp = lds + (wv - split) * MSLAB;
  for (int row = split; row < nq; row += nsplit) {
    const float* rp = grp + row * MROW;
    float M = -INFINITY;
    for (int i = 0; i < nsplit; ++i) M = fmaxf(M, rp[i * MSLAB + HD]);
    float L = 0.f, O0[HD / 128] = {}, O1[HD / 128] = {};
    for (int i = 0; i < nsplit; ++i) {
      const float lg = rp[i * MSLAB + HD + 1];
      const float alpha = (lg > 0.f) ? __expf(rp[i * MSLAB + HD] - M) : 0.f;
      L += alpha * lg;
#pragma unroll
      for (int e = 0; e < HD / 128; ++e) {
        O0[e] += alpha * rp[i * MSLAB + e * 128 + lane * 2];
        O1[e] += alpha * rp[i * MSLAB + e * 128 + lane * 2 + 1];
      }
    }
#pragma unroll
    for (int e = 0; e < HD / 128; ++e) {
      const unsigned int lo = f2b(L > 0.f ? O0[e] / L : 0.f), hi = f2b(L > 0.f ? O1[e] / L : 0.f);
      *reinterpret_cast<unsigned int*>(out + (size_t)(bh0 + row) * HD + e * 128 + lane * 2) = lo | (hi << 16);
    }
  }
}

// softcap > 0 applies gemma2's attention-logit soft-capping
// (s = cap * tanh(s / cap), after scale, before masking); window > 0 is the
// sliding-window mask (query at sl-1 sees positions [sl - window, sl)).
// Both are wave-uniform runtime flags: the llama path (0, 0) takes no tanh.
// FP8: the packed cache copies are OCP e4m3 bytes with per-row scales
// sk/sv (appended by rope_qkv_append's fp8 mode) — half the stream bytes.
// q is quantized per head in-kernel; scores rescale by s_q[row]*s_k[col];
// PV keeps a per-tile running scale R (s_v folded into the quantized P).
// 3 waves/SIMD is what the position loop reaches on its own (136 VGPR + 32
// AGPR with PREFETCH); stated, because with the merge slabs in LDS the
// register allocator otherwise spends a wave of occupancy (168 + 32).
// HD = 256 doubles acco (64 registers) and kbuf (64 with PREFETCH): the bf16
// PREFETCH variant takes all 256 VGPRs of 2 waves/SIMD without scratch, and
// only two 65 KB workgroups fit a CU's 160 KB LDS, so 2 is stated there.
template <bool PREFETCH = false, bool FP8 = false, int HD = 128>
__global__ __launch_bounds__(256, HD > 128 ? 2 : 3) void attn_decode_mfma_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ kp,
    const unsigned short* __restrict__ vp, const int* __restrict__ seq_lens,
    float* __restrict__ ws_o, float* __restrict__ ws_ml,
    int B, int H, int KVH, int T32, int nsplit, float scale, long long q_stride,
    float softcap, int window,
    const float* __restrict__ sk = nullptr, const float* __restrict__ sv = nullptr,
    unsigned short* __restrict__ out = nullptr) {
  static_assert(GQA_PACKED_HD(HD), "packed GQA cache: head_dim 128 or 256");
  constexpr int NC = HD / 32, NG = GQA_VGROUPS(HD), KTILE = GQA_KTILE(HD);  // qk chunks, pv groups
  const int wv = threadIdx.x >> 6;
  const int wid = blockIdx.x * 4 + wv;
  // The kernel's one LDS object: each wave's merge slab, whose head doubles as
  // its P image (16 rows, 96 B row stride: bank-conflict-free b128 reads).
  // Declared in the P image's element type: declared as float and cast for
  // the loop, the same kernel measured 60 us instead of 48 at B=128, sl=540.
  __shared__ __attribute__((aligned(16))) unsigned short plds_all[4][ATTN_MSLAB(HD) * 2];
  // out != null selects the in-workgroup merge: waves past the end (whole
  // groups, as nsplit divides 4) then stay for its barrier with an empty
  // position range and touch no global memory.
  const bool live = wid < B * KVH * nsplit;
  if (!live && out == nullptr) return;
  const int widc = live ? wid : 0;
  const int split = widc % nsplit;
  const int kvh = (widc / nsplit) % KVH;
  const int b = widc / (nsplit * KVH);
  const int lane = threadIdx.x & 63;
  const int NQ = H / KVH;
  const int sl = live ? seq_lens[b] : 0;
  const int chunk = ((T32 / nsplit + 31) >> 5) << 5;
  const int win_lo = (window > 0) ? max(0, sl - window) : 0;  // first visible pos
  const int c0 = max(split * chunk, (win_lo >> 5) << 5);
  const int c1 = min(split * chunk + chunk, sl);
  unsigned short* plds = plds_all[wv];

  using F = Frag<FP8>;
  using FT = typename F::T;
  using FE = typename F::E;

  // Q fragments: A[i = lane&15 (query head, clamped), k = (lane>>4)*8 + j]
  const int qh_base = kvh * NQ;
  const int qi = min(lane & 15, NQ - 1);
  FT qf[NC];
  float srow[4];
  {
    const unsigned short* qrow = q + (size_t)b * q_stride + (size_t)(qh_base + qi) * HD + (lane >> 4) * 8;
    bf16x8 qb[NC] = {};
    if (live) {
#pragma unroll
      for (int c = 0; c < NC; ++c) qb[c] = frag_load<false>(qrow + c * 32);
    }
    if constexpr (FP8) {
      // quantize per head: amax over the 4 lanes x HD / 4 elements of the row
      float mx = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf((float)qb[c][j]));
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float sq = e4m3_scale(mx);
      const float inv = 1.f / sq;
#pragma unroll
      for (int c = 0; c < NC; ++c) qf[c] = to_e4m3x8(qb[c], inv);
#pragma unroll
      for (int r = 0; r < 4; ++r) srow[r] = __shfl(sq, (lane >> 4) * 4 + r);
    } else {
#pragma unroll
      for (int c = 0; c < NC; ++c) qf[c] = qb[c];
    }
  }

  float m[4], lsum[4], Rscale = 1.f;
  floatx4 acco[NG];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; lsum[r] = 0.f; }
#pragma unroll
  for (int g = 0; g < NG; ++g) acco[g] = (floatx4)(0.f);

  // this (b, kv-head)'s K / V images at this lane's slice of every fragment,
  // and (fp8) its per-position scale rows
  const size_t head = (size_t)(b * KVH + kvh);
  const FE* khead = reinterpret_cast<const FE*>(kp) + head * (T32 >> 4) * KTILE + lane * 8;
  const FE* vhead = reinterpret_cast<const FE*>(vp) + head * NG * (T32 >> 5) * FRAG + lane * 8;
  const float* ks_row = FP8 ? sk + head * T32 : nullptr;
  const float* vs_row = FP8 ? sv + head * T32 : nullptr;
  const int col = lane & 15;

  // the 2 * NC K fragments (2 half-tiles x NC hd-chunks) of the 32-position tile at t.
  // PREFETCH: the next tile's are loaded during the previous tile's PV phase
  // (kbuf stays live, +32 VGPR at hd 128, +64 at 256) so the score MFMAs never wait on HBM;
  // measured A/B via XOT_ATTN_PREFETCH.
  FT kbuf[2 * NC];
  auto load_k_tile = [&](int t) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int c = 0; c < NC; ++c)
        kbuf[h * NC + c] = frag_load_nt<FP8>(khead + (size_t)((t >> 4) + h) * KTILE + c * FRAG);
  };
  if (PREFETCH && c0 < c1) load_k_tile(c0);

  for (int t = c0; t < c1; t += 32) {
    // ---- scores: two 16-position half-tiles ----
    if (!PREFETCH) load_k_tile(t);
    floatx4 sc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      sc[h] = (floatx4)(0.f);
#pragma unroll
      for (int c = 0; c < NC; ++c) sc[h] = F::mfma(qf[c], kbuf[h * NC + c], sc[h]);
    }
    // ---- scale, softcap, mask (rows r are this lane's 4 query heads) ----
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int pos = t + h * 16 + col;
      const bool ok = pos < c1 && pos >= win_lo;
      const float skc = FP8 ? ks_row[min(pos, T32 - 1)] : 1.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s = sc[h][r] * scale;
        if (FP8) s *= srow[r] * skc;
        if (softcap > 0.f) s = softcap * tanhf(s * (1.f / softcap));
        sc[h][r] = ok ? s : -INFINITY;
      }
    }
    float alpha[4], s_pv = 1.f, rfac = 1.f;
    attn_softmax_tile(sc[0], sc[1], m, lsum, alpha);
    if (FP8) s_pv = attn_fp8_pv_scale(vs_row, t, c1, lane, Rscale, rfac);
    attn_rescale(acco, alpha, rfac);
    const FT pf = attn_p_fragment<FP8>(plds, sc, lane, vs_row, t, c1, s_pv);
    // issue next tile's K stream now; it completes under the PV MFMAs
    if (PREFETCH && t + 32 < c1) load_k_tile(t + 32);
    // ---- PV: out[16q][g*16..] += P x V ----
    const FE* vt = vhead + (size_t)(t >> 5) * FRAG;
#pragma unroll
    for (int g = 0; g < NG; ++g)
      acco[g] = F::mfma(pf, frag_load_nt<FP8>(vt + (size_t)g * (T32 >> 5) * FRAG), acco[g]);
  }

  // ---- epilogue: final rows merged in the workgroup, or one (m, l, o[HD])
  // partial per (b, qh, split) for attn_decode_merge ----
  if (out != nullptr)
    attn_merge_in_workgroup(reinterpret_cast<float*>(&plds_all[0][0]), out, acco, m, lsum, wv, lane, NQ, b * H + qh_base, nsplit,
                            FP8 ? Rscale : 1.f, live);
  else
    attn_store_partial(ws_o, ws_ml, acco, m, lsum, lane, NQ, b * H + qh_base, nsplit, split,
                       FP8 ? Rscale : 1.f);
}

// ---------------------------------------------------------------------------
// MFMA flash-forward prefill attention (HD = 128 or 256, causal, GQA).
//
// Replaces torch sdpa for the prefill step (reference: torchtune
// MultiHeadAttention prefill, general_mha.py:218-226; sdpa measures ~1.8 ms
// per 70B layer at B=64xS=512 — VALU/flash at ~300 TF).  Grid: one 4-wave
// workgroup per (b, q-head, 128-row q block); the block's waves share K/V
// tiles staged in LDS from the MFMA-packed cache (fragment layout is
// lane-linear, so staging is 1 KB coalesced loads and conflict-free b128
// reads).  Each wave owns 32 q rows (2 MFMA sub-tiles; 16 rows and 64-row q
// blocks at HD = 256, ATTN_PREFILL_NT), walks kv position
// tiles of 32 with online softmax, masks the causal boundary, writes final
// bf16 rows (no split-K workspace).
// ---------------------------------------------------------------------------

// 16-row MFMA sub-tiles per wave (NT): 2 at HD = 128 (128-row q blocks). At
// HD = 256 two sub-tiles still compile without scratch (256 VGPR + 156 AGPR)
// but leave 1 wave/SIMD; one sub-tile (64-row q blocks) runs 2 waves/SIMD and
// measured 0.56 ms against 1.43 ms for a B=64 x S=512, H=16 layer.
constexpr int ATTN_PREFILL_NT(int hd) { return hd > 128 ? 1 : 2; }

template <int HD, int NT>
__global__ __launch_bounds__(256) void attn_prefill_mfma_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ kp,
    const unsigned short* __restrict__ vp, unsigned short* __restrict__ out,
    int B, int S, int H, int KVH, int T32, int start_pos,
    long long q_bstride, long long q_sstride, float scale,
    float softcap, int window) {
  static_assert(GQA_PACKED_HD(HD), "packed GQA cache: head_dim 128 or 256");
  constexpr int NC = HD / 32, NG = GQA_VGROUPS(HD), KTILE = GQA_KTILE(HD);  // qk chunks, pv groups
  static_assert(NT == 1 || NT == 2, "a wave owns one or two 16-row sub-tiles");
  constexpr int QSHIFT = NT == 2 ? 7 : 6, QROWS = 1 << QSHIFT;  // q rows per block: 4 waves x NT x 16
  // block -> (b, h, q-block)
  const int qblocks = (S + QROWS - 1) >> QSHIFT;
  const int h = blockIdx.x % H;
  const int t1 = blockIdx.x / H;
  const int qb = t1 % qblocks;
  const int b = t1 / qblocks;
  const int wv = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int kvh = h / (H / KVH);

  // this wave's 16 * NT q rows: [r0, r0 + 16 * NT)
  const int r0 = qb * QROWS + wv * (16 * NT);
  const int col = lane & 15;

  constexpr int KV_K = 2 * KTILE, KV_V = NG * FRAG;
  __shared__ unsigned short kv_lds[2][KV_K + KV_V];  // dbuf

  // Q fragments for NT sub-tiles x NC hd-chunks; rows clamped to S-1 (writes
  // are predicated, extra rows only waste compute)
  bf16x8 qf[NT][NC];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int row = min(r0 + t * 16 + col, S - 1);
    const unsigned short* qrow = q + (size_t)b * q_bstride + (size_t)row * q_sstride + (size_t)h * HD;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      qf[t][c] = frag_load<false>(qrow + c * 32 + (lane >> 4) * 8);
  }

  float m[NT][4], lsum[NT][4];
  floatx4 acco[NT][NG];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) { m[t][r] = -INFINITY; lsum[t][r] = 0.f; }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < NG; ++g) acco[t][g] = (floatx4)(0.f);

  const size_t kbase = (size_t)(b * KVH + kvh) * (T32 >> 4) * KTILE;
  const size_t vbase = (size_t)(b * KVH + kvh) * NG * (T32 >> 5) * FRAG;
  // causal end for the BLOCK (max row): positions [0, start_pos + block_hi]
  const int block_hi = min(qb * QROWS + QROWS - 1, S - 1);
  const int kv_end = start_pos + block_hi + 1;  // exclusive

  __shared__ unsigned short plds_all[4][16 * 48 * NT];

  // cooperative stage of kv tile `tp` (32 positions) into kv_lds[buf]
  auto stage = [&](int tp, int buf) {
    // K: two 16-pos tiles x NC chunks x 512 elems; V: NG groups x 512 elems
    const unsigned short* ksrc = kp + kbase + (size_t)(tp * 2) * KTILE;
    const unsigned short* vsrc = vp + vbase + (size_t)tp * FRAG;
    unsigned short* dk = kv_lds[buf];
    unsigned short* dv = kv_lds[buf] + KV_K;
    const int tid = threadIdx.x;
    // K: KV_K elems (8 KB at hd 128, 16 KB at 256): 256 threads x KV_K / 2048 x 16 B
#pragma unroll
    for (int i = 0; i < KV_K / 2048; ++i) {
      const int e = (tid + i * 256) * 8;
      *(ushort8*)(dk + e) = *(const ushort8*)(ksrc + e);
    }
    // V: NG groups x 512 elems, group stride (T32>>5)*512 in global
#pragma unroll
    for (int i = 0; i < NG / 4; ++i) {
      const int e = tid + i * 256;           // 0..NG*64-1 -> (group, piece)
      const int g = e >> 6, piece = e & 63;  // 64 pieces of 8 elems per group
      *(ushort8*)(dv + g * FRAG + piece * 8) =
          *(const ushort8*)(vsrc + (size_t)g * (T32 >> 5) * FRAG + piece * 8);
    }
  };

  const int ntiles = (kv_end + 31) >> 5;
  // sliding window: the block's lowest q row sees nothing before
  // start_pos + qb*QROWS - window + 1 — skip whole kv tiles below it
  const int tp0 = (window > 0) ? max(0, (start_pos + qb * QROWS - window + 1) >> 5) : 0;
  stage(tp0, tp0 & 1);
  __syncthreads();

  for (int tp = tp0; tp < ntiles; ++tp) {
    const int buf = tp & 1;
    if (tp + 1 < ntiles) stage(tp + 1, buf ^ 1);  // plain loads overlap compute
    const unsigned short* dk = kv_lds[buf];
    const unsigned short* dv = kv_lds[buf] + KV_K;
    unsigned short* plds = plds_all[wv];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      // scores for two 16-pos halves of this kv tile
      floatx4 sc[2];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        sc[hh] = (floatx4)(0.f);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const bf16x8 kb = *reinterpret_cast<const bf16x8*>(dk + (hh * NC + c) * FRAG + lane * 8);
          sc[hh] = Frag<false>::mfma(qf[t][c], kb, sc[hh]);
        }
      }
      // causal mask: kv pos must be < start_pos + row + 1
      float rmax[4];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int pos = tp * 32 + hh * 16 + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = r0 + t * 16 + (lane >> 4) * 4 + r;
          bool ok = (pos <= start_pos + row) && (pos < kv_end);
          if (window > 0) ok = ok && (pos > start_pos + row - window);
          float s = sc[hh][r] * scale;
          if (softcap > 0.f) s = softcap * tanhf(s * (1.f / softcap));
          sc[hh][r] = ok ? s : -INFINITY;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) rmax[r] = fmaxf(sc[0][r], sc[1][r]);
#pragma unroll
      for (int mm = 1; mm < 16; mm <<= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) rmax[r] = fmaxf(rmax[r], __shfl_xor(rmax[r], mm));
      float alpha[4], rsum[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mn = fmaxf(m[t][r], rmax[r]);
        if (mn == -INFINITY) { alpha[r] = 1.f; rsum[r] = 0.f; sc[0][r] = 0.f; sc[1][r] = 0.f; continue; }
        alpha[r] = (lsum[t][r] > 0.f) ? __expf(m[t][r] - mn) : 0.f;
        m[t][r] = mn;
        const float p0 = __expf(sc[0][r] - mn);
        const float p1 = __expf(sc[1][r] - mn);
        sc[0][r] = p0;
        sc[1][r] = p1;
        rsum[r] = p0 + p1;
      }
#pragma unroll
      for (int mm = 1; mm < 16; mm <<= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r) rsum[r] += __shfl_xor(rsum[r], mm);
#pragma unroll
      for (int r = 0; r < 4; ++r) lsum[t][r] = lsum[t][r] * alpha[r] + rsum[r];
      attn_rescale(acco[t], alpha, 1.f);
      unsigned short* pl = plds + t * 16 * 48;  // one P image per sub-tile
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          pl[((lane >> 4) * 4 + r) * 48 + hh * 16 + col] = f2b(sc[hh][r]);
      const bf16x8 pf = *reinterpret_cast<const bf16x8*>(pl + (lane & 15) * 48 + (lane >> 4) * 8);
#pragma unroll
      for (int g = 0; g < NG; ++g) {
        const bf16x8 vb = *reinterpret_cast<const bf16x8*>(dv + g * FRAG + lane * 8);
        acco[t][g] = Frag<false>::mfma(pf, vb, acco[t][g]);
      }
    }
    __syncthreads();  // all waves done with kv_lds[buf] before restaging
  }

  // epilogue: out[b, row, h, g*16 + col] = acc / lsum
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = r0 + t * 16 + (lane >> 4) * 4 + r;
      if (row < S) {
        const float inv = (lsum[t][r] > 0.f) ? 1.f / lsum[t][r] : 0.f;
        unsigned short* orow = out + (((size_t)b * S + row) * H + h) * HD;
#pragma unroll
        for (int g = 0; g < NG; ++g) orow[g * 16 + col] = f2b(acco[t][g][r] * inv);
      }
    }
  }
}

// layout probe for tests: one v_mfma_f32_16x16x32_bf16, row-major inputs
__global__ void mfma16_probe_kernel(const unsigned short* __restrict__ A,
                                    const unsigned short* __restrict__ Bm,
                                    float* __restrict__ D) {
  const int lane = threadIdx.x;
  bf16x8 a = *reinterpret_cast<const bf16x8*>(A + (lane & 15) * 32 + (lane >> 4) * 8);
  bf16x8 b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b[j] = *reinterpret_cast<const __bf16*>(Bm + ((lane >> 4) * 8 + j) * 16 + (lane & 15));
  floatx4 d = (floatx4)(0.f);
  d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, d, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) D[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = d[r];
}

// ---------------------------------------------------------------------------
// MoE decode-routing glue: the static-capacity routed path needs
// (token-expert pairs -> per-expert-sorted gather list) and the weighted
// combine. In torch this is ~8 launches per MoE layer per step (argsort,
// repeat_interleave, cumsum, eq+sum, clamp, where, index_add) — measured as
// the TOP decode cost on DeepSeek-V2-Lite (profiles/r02_new_decoders_...).
// Here: ONE single-workgroup counting-sort kernel (A = T*k pairs <= 2048,
// E <= 256 fits LDS) + ONE deterministic gather-combine kernel (no atomics:
// out[t] = sum_j w[t,j] * y[pos(t,j)]).
// ---------------------------------------------------------------------------

// Fused MoE router: one wave per token row over the gate logits [T, E].
// mode 0: softmax -> top-k -> renormalize (Mixtral / qwen3-moe).
// mode 1: sigmoid + e-score bias -> group-limited top-k (top-2-sum group
//         scores, keep topk_group groups) -> gather sigmoid weights ->
//         optional renorm -> routed scaling (DeepSeek V2/V3).
// Replaces ~4-10 torch launches per MoE layer per step. E <= 256, k <= 8.
__global__ __launch_bounds__(256) void moe_route_kernel(
    const float* __restrict__ logits, const float* __restrict__ bias,
    int* __restrict__ idx, float* __restrict__ w,
    int T, int E, int k, int mode, int n_group, int topk_group,
    float routed_scale, int norm_topk) {
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= T) return;
  const int lane = threadIdx.x & 63;
  // per-lane 4 contiguous elements (E <= 256)
  float v[4], s[4], c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = lane * 4 + j;
    v[j] = (e < E) ? logits[(size_t)row * E + e] : -INFINITY;
  }
  if (mode == 0) {
    // softmax over the row
    float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = (v[j] == -INFINITY) ? 0.f : __expf(v[j] - mx);
      sum += s[j];
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] /= sum;
      c[j] = (v[j] == -INFINITY) ? -INFINITY : s[j];
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      s[j] = 1.f / (1.f + __expf(-v[j]));
      const int e = lane * 4 + j;
      c[j] = (e < E) ? s[j] + (bias ? bias[e] : 0.f) : -INFINITY;
    }
    if (n_group > 1) {
      // group score = sum of top-2 choice values in the group; keep the
      // topk_group best groups, mask the rest
      const int gsize = E / n_group;  // elements per group (>= 4 assumed)
      float gs[8];
      for (int g = 0; g < n_group; ++g) {
        float m1 = -INFINITY, m2 = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = lane * 4 + j;
          const float cv = (e >= g * gsize && e < (g + 1) * gsize) ? c[j] : -INFINITY;
          if (cv > m1) { m2 = m1; m1 = cv; }
          else if (cv > m2) { m2 = cv; }
        }
        // wave-combine per-lane top2
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
          const float o1 = __shfl_xor(m1, m);
          const float o2 = __shfl_xor(m2, m);
          if (o1 > m1) { m2 = fmaxf(m1, o2); m1 = o1; }
          else { m2 = fmaxf(m2, o1); }
        }
        gs[g] = m1 + (m2 == -INFINITY ? 0.f : m2);
      }
      // select topk_group groups (all lanes hold identical gs)
      unsigned int keep = 0;
      for (int t = 0; t < topk_group; ++t) {
        int best = -1;
        float bv = -INFINITY;
        for (int g = 0; g < n_group; ++g)
          if (!(keep >> g & 1) && gs[g] > bv) { bv = gs[g]; best = g; }
        if (best >= 0) keep |= 1u << best;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = lane * 4 + j;
        if (e < E && !(keep >> (e / gsize) & 1)) c[j] = -INFINITY;
      }
    }
  }
  // iterative wave-wide top-k on c; weights come from s
  float wsum = 0.f;
  float wk[8];
  int ik[8];
  for (int t = 0; t < k; ++t) {
    float mx = fmaxf(fmaxf(c[0], c[1]), fmaxf(c[2], c[3]));
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    // lowest index attaining the max (torch.topk tie convention)
    int my = INT_MAX;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c[j] == mx && lane * 4 + j < my) my = lane * 4 + j;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) my = min(my, __shfl_xor(my, m));
    const int owner = my >> 2, slot = my & 3;
    float sv;
    switch (slot) {
      case 0: sv = __shfl(s[0], owner); break;
      case 1: sv = __shfl(s[1], owner); break;
      case 2: sv = __shfl(s[2], owner); break;
      default: sv = __shfl(s[3], owner); break;
    }
    ik[t] = my;
    wk[t] = sv;
    wsum += sv;
    if (lane == owner) c[slot] = -INFINITY;
  }
  if (lane == 0) {
    const float inv = (mode == 0 || norm_topk) ? 1.f / (wsum + 1e-20f) : 1.f;
    for (int t = 0; t < k; ++t) {
      idx[(size_t)row * k + t] = ik[t];
      w[(size_t)row * k + t] = wk[t] * inv * routed_scale;
    }
  }
}

__global__ __launch_bounds__(256) void moe_build_kernel(
    const int* __restrict__ idx, int* __restrict__ gather_tok,
    int* __restrict__ inv_pos, int T, int k, int E, int C) {
  __shared__ int counts[256];
  __shared__ int offsets[256];
  const int tid = threadIdx.x;
  const int A = T * k;
  for (int e = tid; e < E; e += 256) counts[e] = 0;
  __syncthreads();
  for (int a = tid; a < A; a += 256) atomicAdd(&counts[idx[a]], 1);
  __syncthreads();
  if (tid == 0) {  // E <= 256: serial prefix is ~E adds, negligible here
    int run = 0;
    for (int e = 0; e < E; ++e) {
      offsets[e] = run;
      run += counts[e];
    }
  }
  __syncthreads();
  for (int e = tid; e < E; e += 256) counts[e] = 0;  // reuse as cursors
  // default: invalid capacity slots gather token 0 (scale is 0 via inv_pos)
  for (int p = tid; p < E * C; p += 256) gather_tok[p] = 0;
  __syncthreads();
  for (int a = tid; a < A; a += 256) {
    const int e = idx[a];
    const int r = atomicAdd(&counts[e], 1);           // rank within expert
    const int global_rank = offsets[e] + r;           // dense order
    // dense position -> padded [E, C] position
    const int pos = e * C + r;                        // r < C always (count_e <= T <= C)
    gather_tok[pos] = a / k;
    inv_pos[a] = pos;
    (void)global_rank;
  }
}

// out[t, :] = sum_j w[t, j] * y[inv_pos[t*k + j], :]   (fp32 accumulate)
__global__ __launch_bounds__(256) void moe_combine_kernel(
    const unsigned short* __restrict__ y, const int* __restrict__ inv_pos,
    const float* __restrict__ w, unsigned short* __restrict__ out,
    int T, int k, int D) {
  const long long n8 = (long long)T * (D >> 3);
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int d8 = D >> 3;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n8; i += stride) {
    const int t = (int)(i / d8);
    const int c8 = (int)(i % d8) * 8;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int j = 0; j < k; ++j) {
      const float wj = w[t * k + j];
      const ushort8 v = *(const ushort8*)(y + (size_t)inv_pos[t * k + j] * D + c8);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += wj * b2f(v[q]);
    }
    ushort8 o;
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] = f2b(acc[q]);
    *(ushort8*)(out + (size_t)t * D + c8) = o;
  }
}

// ---------------------------------------------------------------------------
// MLA (DeepSeek V2/V3) decode attention on matrix cores — ABSORBED form.
//
// The kv_b projection is folded into the query and output (DeepSeek's own
// inference trick): q_lat[h] = q_nope[h] @ W_k[h] lives in latent space, so
// decode attention is MQA over the cached per-token latent(512)+rope(64)
// stream — 1152 B/token TOTAL regardless of head count (the reference's
// torchtune engine cannot run MLA at all; a GQA cache for V3 would be
// n_heads*576 per token).  Per 32-position tile and 16-head group:
//   scores[16h][16p]: 18 x v_mfma_f32_16x16x32_bf16 per half-tile
//     (A = q fragments re-gathered from L1, B = 1 KB coalesced packed-cache
//      streams — same fragment geometry as the GQA kernel)
//   online softmax via 4 x shfl over 16-lane column groups (same lines as the
//     GQA kernel's attn_softmax_tile; the rescale and fp8 PV scale are shared)
//   out_lat[16h][512] += 32 x mfma (P from LDS image, V = packed latent)
// One wave per (b, head-group, split); fp32 (m, l, o[512]) partials merged
// by attn_decode_merge<512>.  Latent+rope cache copies are kept in the SAME
// fragment-packed layouts as the GQA kp/vp (kfrag_off / vfrag_off with
// 18 qk-chunks / 32 pv-groups), appended by mla_append_kernel.
// ---------------------------------------------------------------------------

#define MLA_LAT 512
#define MLA_ROPE 64
#define MLA_DQK 576   // latent + rope, the absorbed q/k width
#define MLA_CHQK 18   // 32-dim MFMA chunks across DQK
#define MLA_GPV 32    // 16-dim output groups across LAT
#define MLA_KTILE (MLA_CHQK * FRAG)  // one 16-position K tile of the latent+rope image

// rope of a 64-dim MLA tail x: lane l < 32 owns the input pair (2l, 2l+1)
// (interleaved convention) or (l, l+32) (half); the rotated pair is always
// output dims (l, l+32) — HALF layout, cat([x1c - x2s, x2c + x1s]) like _rope
DEVINL void mla_rope_pair(const unsigned short* x, const float* __restrict__ cosb,
                          const float* __restrict__ sinb, int pos, int lane, int interleave,
                          float& r1, float& r2) {
  const int i1 = interleave ? lane * 2 : lane;
  const int i2 = interleave ? lane * 2 + 1 : lane + 32;
  rope_pair(b2f(x[i1]), b2f(x[i2]), cosb[(size_t)pos * 32 + lane], sinb[(size_t)pos * 32 + lane], r1, r2);
}

// Fused MLA KV-side prep: raw kv_a output [B,S,576] -> RMSNorm the 512-dim
// latent (fp32 math, weight w), rope the 64-dim shared key at `positions`
// (interleaved or half convention), and write BOTH cache layouts (plain
// [B,1,T,512]/[B,1,T,64] for the eager prefill reader, fragment-packed
// kp/vp for the MFMA decode kernel). Replaces ~10 torch launches per layer
// (norm ops, rope ops, two .contiguous() copies, slice writes) with one.
// One wave per (b, s): 512 = 64 lanes x 8 for the rms reduce.
__global__ __launch_bounds__(256) void mla_prep_append_kernel(
    const unsigned short* __restrict__ ckv, const unsigned short* __restrict__ w,
    const float* __restrict__ cosb, const float* __restrict__ sinb,
    const int* __restrict__ positions,
    unsigned short* __restrict__ lat_c, unsigned short* __restrict__ rot_c,
    unsigned short* __restrict__ kp, unsigned short* __restrict__ vp,
    int B, int S, int T, int T32, float eps, int interleave, int npos,
    unsigned char* __restrict__ kp8, unsigned char* __restrict__ vp8,
    float* __restrict__ ks) {
  const int wid = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wid >= B * S) return;
  const int lane = threadIdx.x & 63;
  const int b = wid / S;
  const int pos = row_position(positions, npos, B, S, wid);
  const unsigned short* row = ckv + (size_t)wid * MLA_DQK;
  // ---- rms over the 512 latent dims ----
  float v[8];
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = b2f(row[lane * 8 + j]);
    acc += v[j] * v[j];
  }
  const float inv = rsqrtf(wave_sum(acc) / (float)MLA_LAT + eps);
  float lat[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) lat[j] = v[j] * inv * b2f(w[lane * 8 + j]);
  // ---- rope the 64-dim shared key (lanes 0..31 handle one pair each) ----
  float r1 = 0.f, r2 = 0.f;
  if (lane < 32) mla_rope_pair(row + MLA_LAT, cosb, sinb, pos, lane, interleave, r1, r2);
  // plain caches (bf16, prefill reader) + bf16 packed copies
  unsigned short* lrow = lat_c + ((size_t)b * T + pos) * MLA_LAT;
  unsigned short* rrow = rot_c + ((size_t)b * T + pos) * MLA_ROPE;
  const int tiles32 = T32 >> 5;
  const size_t ktile = ((size_t)b * (T32 >> 4) + (pos >> 4)) * MLA_KTILE;
  const size_t vhead = (size_t)b * MLA_GPV * tiles32 * FRAG;
  const int d1 = MLA_LAT + lane, d2 = MLA_LAT + lane + 32;  // the rope pair's k dims
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int d = lane * 8 + j;
    lrow[d] = f2b(lat[j]);
    if (kp) {
      kp[ktile + kfrag_off(d, pos)] = f2b(lat[j]);
      vp[vhead + vfrag_off(d, pos, tiles32)] = f2b(lat[j]);
    }
  }
  if (lane < 32) {
    rrow[lane] = f2b(r1);
    rrow[lane + 32] = f2b(r2);
    if (kp) {
      kp[ktile + kfrag_off(d1, pos)] = f2b(r1);
      kp[ktile + kfrag_off(d2, pos)] = f2b(r2);
    }
  }
  if (kp8) {
    // fp8 packed copies: one scale per token row over all 576 dims
    float mx = fmaxf(fabsf(r1), fabsf(r2));
#pragma unroll
    for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(lat[j]));
    const float scl = e4m3_scale(wave_max(mx));
    const float qinv = 1.f / scl;
    if (lane == 0) ks[(size_t)b * T32 + pos] = scl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = lane * 8 + j;
      const unsigned char q8 = to_e4m3(lat[j] * qinv);
      kp8[ktile + kfrag_off(d, pos)] = q8;
      vp8[vhead + vfrag_off(d, pos, tiles32)] = q8;
    }
    if (lane < 32) {
      kp8[ktile + kfrag_off(d1, pos)] = to_e4m3(r1 * qinv);
      kp8[ktile + kfrag_off(d2, pos)] = to_e4m3(r2 * qinv);
    }
  }
}

// q-side finisher: rope the 64-dim query tail and assemble the absorbed
// query [B, H, 576] = [q_lat(512) | rope(q_rot)(64)] in one launch
// (replaces ~6 torch ops per layer: rope mul/cat x2, cat, contiguous).
// One wave per (b, h): q strided [B, S=1, H, 192], q_lat [B, 1, H, 512].
__global__ __launch_bounds__(256) void mla_q_prep_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ q_lat,
    const float* __restrict__ cosb, const float* __restrict__ sinb,
    const int* __restrict__ positions, unsigned short* __restrict__ qfull,
    int B, int H, long long q_bstride, int nope, int interleave, int npos,
    unsigned char* __restrict__ q8, float* __restrict__ sq) {
  const int wid = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wid >= B * H) return;
  const int lane = threadIdx.x & 63;
  const int h = wid % H;
  const int b = wid / H;
  const unsigned short* lsrc = q_lat + ((size_t)b * H + h) * MLA_LAT;
  float lv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) lv[j] = b2f(lsrc[lane * 8 + j]);
  float r1 = 0.f, r2 = 0.f;
  if (lane < 32)
    mla_rope_pair(q + (size_t)b * q_bstride + (size_t)h * (nope + MLA_ROPE) + nope, cosb, sinb,
                  row_position(positions, npos, B, 1, b), lane, interleave, r1, r2);
  if (q8 == nullptr) {
    unsigned short* dst = qfull + ((size_t)b * H + h) * MLA_DQK;
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[lane * 8 + j] = f2b(lv[j]);
    if (lane < 32) {
      dst[MLA_LAT + lane] = f2b(r1);
      dst[MLA_LAT + lane + 32] = f2b(r2);
    }
    return;
  }
  // fp8 output: one e4m3 scale per (b, h) query row over all 576 dims
  float mx = fmaxf(fabsf(r1), fabsf(r2));
#pragma unroll
  for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(lv[j]));
  const float scl = e4m3_scale(wave_max(mx));
  const float inv = 1.f / scl;
  if (lane == 0) sq[(size_t)b * H + h] = scl;
  unsigned char* dst8 = q8 + ((size_t)b * H + h) * MLA_DQK;
#pragma unroll
  for (int j = 0; j < 8; ++j) dst8[lane * 8 + j] = to_e4m3(lv[j] * inv);
  if (lane < 32) {
    dst8[MLA_LAT + lane] = to_e4m3(r1 * inv);
    dst8[MLA_LAT + lane + 32] = to_e4m3(r2 * inv);
  }
}

__global__ __launch_bounds__(256) void mla_append_kernel(
    const unsigned short* __restrict__ lat, const unsigned short* __restrict__ rot,
    const int* __restrict__ positions, unsigned short* __restrict__ kp,
    unsigned short* __restrict__ vp, int B, int S, int T32, int npos) {
  // wave per (b, s); lane covers dims d = lane*9 .. lane*9+8 (576 = 64*9)
  const int wid = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wid >= B * S) return;
  const int lane = threadIdx.x & 63;
  const int b = wid / S;
  const int pos = row_position(positions, npos, B, S, wid);
  const unsigned short* lrow = lat + (size_t)wid * MLA_LAT;
  const unsigned short* rrow = rot + (size_t)wid * MLA_ROPE;
  const size_t ktile = ((size_t)b * (T32 >> 4) + (pos >> 4)) * MLA_KTILE;
  const size_t vhead = (size_t)b * MLA_GPV * (T32 >> 5) * FRAG;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const int d = lane * 9 + i;
    const unsigned short v = (d < MLA_LAT) ? lrow[d] : rrow[d - MLA_LAT];
    kp[ktile + kfrag_off(d, pos)] = v;
    if (d < MLA_LAT) vp[vhead + vfrag_off(d, pos, T32 >> 5)] = v;
  }
}

template <bool FP8 = false>
__global__ __launch_bounds__(256) void attn_decode_mla_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ kp,
    const unsigned short* __restrict__ vp, const int* __restrict__ seq_lens,
    float* __restrict__ ws_o, float* __restrict__ ws_ml,
    int B, int H, int T32, int nsplit, float scale,
    const float* __restrict__ sq = nullptr, const float* __restrict__ ks = nullptr) {
  const int wv = threadIdx.x >> 6;
  const int wid = blockIdx.x * 4 + wv;
  const int hgroups = (H + 15) >> 4;
  __shared__ unsigned short plds_all[4][16 * 48];
  if (wid >= B * hgroups * nsplit) return;
  const int split = wid % nsplit;
  const int hg = (wid / nsplit) % hgroups;
  const int b = wid / (nsplit * hgroups);
  const int lane = threadIdx.x & 63;
  const int sl = seq_lens[b];
  const int chunk = ((T32 / nsplit + 31) >> 5) << 5;
  const int c0 = split * chunk;
  const int c1 = min(c0 + chunk, sl);
  unsigned short* plds = plds_all[wv];

  const int nq = min(16, H - hg * 16);
  const int qi = min(lane & 15, nq - 1);
  const unsigned short* qrow = q + ((size_t)b * H + hg * 16 + qi) * MLA_DQK + (lane >> 4) * 8;
  const unsigned char* qrow8 = reinterpret_cast<const unsigned char*>(q)
      + ((size_t)b * H + hg * 16 + qi) * MLA_DQK + (lane >> 4) * 8;
  const unsigned char* kp8 = reinterpret_cast<const unsigned char*>(kp);
  const unsigned char* vp8 = reinterpret_cast<const unsigned char*>(vp);
  float srow[4], Rscale = 1.f;
  if (FP8) {
    const float sqv = sq[(size_t)b * H + hg * 16 + qi];
#pragma unroll
    for (int r = 0; r < 4; ++r) srow[r] = __shfl(sqv, (lane >> 4) * 4 + r);
  }

  float m[4], lsum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; lsum[r] = 0.f; }
  floatx4 acco[MLA_GPV];
#pragma unroll
  for (int g = 0; g < MLA_GPV; ++g) acco[g] = (floatx4)(0.f);

  const size_t kbase = (size_t)b * (T32 >> 4) * MLA_KTILE;
  const size_t vbase = (size_t)b * MLA_GPV * (T32 >> 5) * FRAG;
  const int col = lane & 15;

  for (int t = c0; t < c1; t += 32) {
    floatx4 sc[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) sc[h] = (floatx4)(0.f);
    // scores over the 18 qk chunks; q fragments re-gathered per chunk
    // (L1-resident after the first tile), k streamed packed
    for (int c = 0; c < MLA_CHQK; ++c) {
      if (FP8) {
        const long a = *reinterpret_cast<const long*>(qrow8 + c * 32);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const unsigned char* kt = kp8 + kbase
              + ((size_t)((t >> 4) + h) * MLA_CHQK + c) * 512 + (size_t)lane * 8;
          const long kb = __builtin_nontemporal_load(reinterpret_cast<const long*>(kt));
          sc[h] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, kb, sc[h], 0, 0, 0);
        }
      } else {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(qrow + c * 32);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const unsigned short* kt = kp + kbase
              + ((size_t)((t >> 4) + h) * MLA_CHQK + c) * 512 + (size_t)lane * 8;
          const bf16x8 kb = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(kt));
          sc[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, kb, sc[h], 0, 0, 0);
        }
      }
    }
    float rmax[4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int pos = t + h * 16 + col;
      const bool ok = pos < c1;
      const float skc = FP8 ? ks[(size_t)b * T32 + min(pos, T32 - 1)] : 1.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sv_ = sc[h][r] * scale;
        if (FP8) sv_ *= srow[r] * skc;
        sc[h][r] = ok ? sv_ : -INFINITY;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) rmax[r] = fmaxf(sc[0][r], sc[1][r]);
#pragma unroll
    for (int mm = 1; mm < 16; mm <<= 1)
#pragma unroll
      for (int r = 0; r < 4; ++r) rmax[r] = fmaxf(rmax[r], __shfl_xor(rmax[r], mm));
    float alpha[4], rsum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mn = fmaxf(m[r], rmax[r]);
      alpha[r] = (lsum[r] > 0.f) ? __expf(m[r] - mn) : 0.f;
      m[r] = mn;
      const float p0 = __expf(sc[0][r] - mn);
      const float p1 = __expf(sc[1][r] - mn);
      sc[0][r] = p0;
      sc[1][r] = p1;
      rsum[r] = p0 + p1;
    }
#pragma unroll
    for (int mm = 1; mm < 16; mm <<= 1)
#pragma unroll
      for (int r = 0; r < 4; ++r) rsum[r] += __shfl_xor(rsum[r], mm);
#pragma unroll
    for (int r = 0; r < 4; ++r) lsum[r] = lsum[r] * alpha[r] + rsum[r];
    float s_pv = 1.f, rfac = 1.f;
    if (FP8) s_pv = attn_fp8_pv_scale(ks + (size_t)b * T32, t, c1, lane, Rscale, rfac);
    attn_rescale(acco, alpha, rfac);
    long pf8 = 0;
    bf16x8 pf;
    if (FP8) {
      unsigned char* pl8 = reinterpret_cast<unsigned char*>(plds);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int pos = t + h * 16 + col;
        const float svv = pos < c1 ? ks[(size_t)b * T32 + pos] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned short pk = (unsigned short)__builtin_amdgcn_cvt_pk_fp8_f32(
              sc[h][r] * svv / s_pv, 0.f, 0, false);
          pl8[((lane >> 4) * 4 + r) * 48 + h * 16 + col] = (unsigned char)(pk & 0xff);
        }
      }
      pf8 = *reinterpret_cast<const long*>(pl8 + (lane & 15) * 48 + (lane >> 4) * 8);
      const unsigned char* vt8 = vp8 + vbase + (size_t)(t >> 5) * 512 + (size_t)lane * 8;
      for (int g = 0; g < MLA_GPV; ++g) {
        const long vb = __builtin_nontemporal_load(
            reinterpret_cast<const long*>(vt8 + (size_t)g * (T32 >> 5) * 512));
        acco[g] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(pf8, vb, acco[g], 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          plds[((lane >> 4) * 4 + r) * 48 + h * 16 + col] = f2b(sc[h][r]);
      pf = *reinterpret_cast<const bf16x8*>(plds + (lane & 15) * 48 + (lane >> 4) * 8);
      const unsigned short* vt = vp + vbase + (size_t)(t >> 5) * 512 + (size_t)lane * 8;
      for (int g = 0; g < MLA_GPV; ++g) {
        const bf16x8 vb = __builtin_nontemporal_load(
            reinterpret_cast<const bf16x8*>(vt + (size_t)g * (T32 >> 5) * 512));
        acco[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vb, acco[g], 0, 0, 0);
      }
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow_i = (lane >> 4) * 4 + r;
    if (qrow_i < nq) {
      const size_t pidx = ((size_t)(b * H + hg * 16 + qrow_i) * nsplit + split);
      for (int g = 0; g < MLA_GPV; ++g)
        ws_o[pidx * MLA_LAT + g * 16 + col] = acco[g][r] * (FP8 ? Rscale : 1.f);
      if (col == 0) {
        ws_ml[pidx * 2 + 0] = m[r];
        ws_ml[pidx * 2 + 1] = lsum[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// SwiGLU: silu(gate) * up, elementwise, vectorized
// ---------------------------------------------------------------------------

// The one SwiGLU expression: silu(gate) * up on bf16 bits, fp32 math, one
// rounding. Every kernel that applies the activation calls this, so the
// elementwise kernels, the down GEMM's X staging and the gate_up GEMM's fused
// store give the same bits.
DEVINL unsigned short swiglu_bf16(unsigned short g, unsigned short u) {
  const float gf = b2f(g);
  const float s = gf * __builtin_amdgcn_rcpf(1.f + __expf(-gf));
  return f2b(s * b2f(u));
}

__global__ __launch_bounds__(256) void swiglu_kernel(
    const unsigned short* __restrict__ g, const unsigned short* __restrict__ u,
    unsigned short* __restrict__ out, long long n8) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n8; i += stride) {
    ushort8 gv = *(const ushort8*)(g + i * 8);
    ushort8 uv = *(const ushort8*)(u + i * 8);
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = swiglu_bf16(gv[j], uv[j]);
    *(ushort8*)(out + i * 8) = o;
  }
}

// packed variant: gu = [rows, 2*I] from the fused gate_up GEMM ([gate | up])
__global__ __launch_bounds__(256) void swiglu_packed_kernel(
    const unsigned short* __restrict__ gu, unsigned short* __restrict__ out,
    long long rows, int I) {
  const long long n8 = rows * (I >> 3);
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int i8 = I >> 3;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n8; i += stride) {
    const long long row = i / i8;
    const long long col8 = i % i8;
    const unsigned short* base = gu + row * (2LL * I) + col8 * 8;
    ushort8 gv = *(const ushort8*)base;
    ushort8 uv = *(const ushort8*)(base + I);
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = swiglu_bf16(gv[j], uv[j]);
    *(ushort8*)(out + i * 8) = o;
  }
}

// packed GeGLU (gemma2): gelu_tanh(gate) * up on the fused [gate | up] GEMM
// output — same stream shape as swiglu_packed, tanh-approximate gelu in fp32.
__global__ __launch_bounds__(256) void geglu_packed_kernel(
    const unsigned short* __restrict__ gu, unsigned short* __restrict__ out,
    long long rows, int I) {
  const long long n8 = rows * (I >> 3);
  const long long stride = (long long)gridDim.x * blockDim.x;
  const int i8 = I >> 3;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n8; i += stride) {
    const long long row = i / i8;
    const long long col8 = i % i8;
    const unsigned short* base = gu + row * (2LL * I) + col8 * 8;
    ushort8 gv = *(const ushort8*)base;
    ushort8 uv = *(const ushort8*)(base + I);
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gf = b2f(gv[j]);
      const float g3 = 0.7978845608028654f * (gf + 0.044715f * gf * gf * gf);
      const float s = 0.5f * gf * (1.f + tanhf(g3));
      o[j] = f2b(s * b2f(uv[j]));
    }
    *(ushort8*)(out + i * 8) = o;
  }
}

// ---------------------------------------------------------------------------
// Skinny decode GEMM: Y[M,N] = X[M,K] @ W[N,K]^T, bf16, M <= 256 (decode
// batch).  This is the decode hot path's dominant cost (the reference runs
// every projection through torchtune's nn.Linear -> cuBLAS,
// llm_utils.py:491-500 / general_mha.py:83-102); at decode shapes the GEMM is
// pure weight streaming and hipBLASLt leaves bandwidth on the table at large
// K (down_proj [M,28672]x[28672,8192] measured 3.6 TB/s vs ~6.3 achievable).
//
// Design (MI355X / CDNA4):
//   * computed as D^T = W . X^T on v_mfma_f32_32x32x16_bf16: the A operand
//     (W, the streamed 0.1-2 GB operand) and the B operand (X, L2/L3
//     resident) are BOTH k-contiguous 16 B per lane in this orientation, so
//     no transpose and no LDS staging at all -- per the CDNA4 guide's
//     "GEMV / small-M decode weights: load straight to VGPRs, deep unroll,
//     late vmcnt" rule.  Each 128 B cache line of W is consumed by 8
//     fragment loads of the same wave (L1-absorbed).
//   * grid = (N/BN) * SPLITK workgroups of 4 waves; BN = 128 (one 32-row
//     n-tile per wave); SPLITK chosen so the grid oversubscribes the 256 CUs
//     (>= 2 blocks/CU) while K/SPLITK stays >= ~1024 (latency amortized).
//   * fp32 split-K partials + a tiny vectorized combine kernel (bias fused);
//     SPLITK == 1 writes bf16 directly.
// ---------------------------------------------------------------------------

DEVINL bf16x8 load_bf16x8(const unsigned short* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}

// Shared epilogue of every skinny GEMM kernel: store one wave's MT 32x32
// accumulators. D layout (32x32): m = lane&31 (col), n_local = (r&3) +
// 8*(r>>2) + 4*(lane>>5). m0 = the lane's row in m-tile 0 (expert offset
// included), nbase = the lane's first n. SPLIT writes fp32 partials into
// P [nsplit, rows_total, N] (bias is added by the combine), otherwise bf16
// + bias into Y. SCALED (fp8) dequantizes by sx[m] * sw[sw_base + n]
// (sw_base = the expert's offset into sw); the bf16 kernels pass no scales.
// GLU (unsplit bf16, no bias): the weight rows are in the GLU-interleaved order
// of ops.glu_interleave_perm, so in every 32-row tile n_local w and w + 8
// (w % 16 < 8) are the gate and up row of one SwiGLU column and a lane's
// accumulators 8p + j and 8p + 4 + j are such a pair. Both sums are rounded to
// bf16 as the plain store rounds them, then swiglu_bf16 gives what
// swiglu_packed gives on the plain output: Y is [rows, N / 2], the lane's 4
// results of half p go to columns 16 * n32 + 8 * p + 4 * (lane >> 5) + j.
template <int MT, bool SPLIT, bool SCALED = false, bool GLU = false>
DEVINL void skinny_store_acc(const floatx16 (&acc)[MT], unsigned short* Y, float* P,
                             const unsigned short* bias, int N, int split, int rows_total,
                             int m0, int nbase, const float* sx = nullptr,
                             const float* sw = nullptr, size_t sw_base = 0) {
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = m0 + t * 32;
    float sxm = 1.f;
    if (SCALED) sxm = sx[m];
    if constexpr (GLU) {
      static_assert(!SPLIT && !SCALED, "the GLU store takes final bf16 sums");
      const int I = N >> 1;
      unsigned short* yrow = Y + (size_t)m * I + ((nbase >> 5) << 4) + (nbase & 31);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        unsigned short o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          o[j] = swiglu_bf16(f2b(acc[t][8 * p + j]), f2b(acc[t][8 * p + 4 + j]));
        *reinterpret_cast<unsigned long long*>(yrow + 8 * p) =
            *reinterpret_cast<unsigned long long*>(o);
      }
    } else if (SPLIT) {
      float* prow = P + ((size_t)split * rows_total + m) * N;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        floatx4 v4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v4[j] = acc[t][g * 4 + j];
          if (SCALED) v4[j] = v4[j] * sxm * sw[sw_base + nbase + g * 8 + j];
        }
        *reinterpret_cast<floatx4*>(prow + nbase + g * 8) = v4;
      }
    } else {
      unsigned short* yrow = Y + (size_t)m * N;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        unsigned short o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = acc[t][g * 4 + j];
          if (SCALED) v = v * sxm * sw[sw_base + nbase + g * 8 + j];
          if (bias) v += b2f(bias[nbase + g * 8 + j]);
          o[j] = f2b(v);
        }
        *reinterpret_cast<unsigned long long*>(yrow + nbase + g * 8) =
            *reinterpret_cast<unsigned long long*>(o);
      }
    }
  }
}

// MT = M/32 (1..8). One workgroup computes Y[0:M, n0:n0+128] over k-range
// [k0, k1). Lane l of wave w holds A row (n0 + w*32 + (l&31)), k-chunk
// (l>>5)*8; B col (mt*32 + (l&31)) of X with the same k-chunk.
template <int MT, bool SPLIT>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(
    const unsigned short* __restrict__ W, const unsigned short* __restrict__ X,
    unsigned short* __restrict__ Y, float* __restrict__ P,
    const unsigned short* __restrict__ bias,
    int N, long long K, int kc, int nsplit) {
  const int ntiles = N >> 7;
  const int tile = blockIdx.x % ntiles;
  const int split = blockIdx.x / ntiles;
  const long long k0 = (long long)split * kc;
  const long long k1 = min(k0 + (long long)kc, K);
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int n0 = tile * 128 + wv * 32;
  const int arow = n0 + (lane & 31);
  const long long koff = (lane >> 5) * 8;

  floatx16 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (floatx16)(0.f);

  const unsigned short* wp = W + (size_t)arow * K + k0 + koff;
  const unsigned short* xp = X + (size_t)(lane & 31) * K + k0 + koff;

  long long k = k0;
#pragma unroll 1
  for (; k + 64 <= k1; k += 64) {
    bf16x8 a[4], b[4][MT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = load_bf16x8(wp + u * 16);
#pragma unroll
      for (int t = 0; t < MT; ++t) b[u][t] = load_bf16x8(xp + (size_t)t * 32 * K + u * 16);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < MT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[u], b[u][t], acc[t], 0, 0, 0);
    wp += 64;
    xp += 64;
  }
  for (; k < k1; k += 16) {
    bf16x8 a = load_bf16x8(wp);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      bf16x8 b = load_bf16x8(xp + (size_t)t * 32 * K);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0, 0, 0);
    }
    wp += 16;
    xp += 16;
  }

  // non-grouped: P layout [nsplit, M, N]
  skinny_store_acc<MT, SPLIT>(acc, Y, P, bias, N, split, MT * 32, lane & 31,
                              n0 + 4 * (lane >> 5));
}

// ---------------------------------------------------------------------------
// v2: prepacked-weight variant.  W is pre-shuffled ONCE at load time into
// MFMA A-fragment order: [N/32][K/16][lane 0..63][8 bf16], lane = (k-half)*32
// + n-row — so each A-fragment load is one fully-coalesced wave-wide 1 KB
// stream (v1's fragment-shaped 16 B gathers are TA/load-path-bound: measured
// 2.0 vs 5.3 TB/s).  X is staged cooperatively per 64-k step into a padded
// LDS image (row stride 72 elems = 144 B -> ds_read_b128 bank-conflict-free)
// and read back as B fragments.  K % 64 == 0 required.
// ---------------------------------------------------------------------------

// One 16 B piece of the X stage. SWIGLU: p points at the gate half of the
// fused [rows, 2K] gate|up row (up at +K); returns silu(gate) * up.
template <bool SWIGLU>
DEVINL ushort8 skinny_stage_load(const unsigned short* p, long long K) {
  ushort8 v = *(const ushort8*)p;
  if (SWIGLU) {
    const ushort8 up = *(const ushort8*)(p + K);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = swiglu_bf16(v[j], up[j]);
  }
  return v;
}

// Also the MoE grouped-GEMM kernel (the reference's latent
// MOEExpert/MOELayer scaffolding, llm_utils.py:502-590, never executed): for
// Mixtral-class decode each expert e (blockIdx.y) computes its own
// [C, N] = [C, K] @ Wp_e^T over a fixed per-expert token capacity C — one
// launch covers every expert, weights stream from the stacked prepack.
//
// NW = waves per workgroup = 32-row weight tiles per workgroup. NW = 4 is the
// 128-row tile with one LDS image and two barriers per K-step. NW = 8 (MT >= 4
// only) is the 256-row tile: all 8 waves share one staged X image, so the
// staged X bytes and the staging work per weight byte halve, and the image is
// double-buffered so a K-step costs one barrier. Each wave's A stream, its
// accumulators and its MFMA order are the same in both, and the launcher keeps
// nsplit and kc, so both give the same bits.
//
// W4 = the MXFP4 weight-only A stream (W4A16): OCP e2m1 codes, two per byte,
// with one e8m0 scale per 32 elements along K. The ONE definition of its two
// images (ops.pack_decode_weight_mxfp4 writes them, the CPU test states them
// independently):
//   code image  [N/32][K/64][lane 0..63][16 B], lane = (k-half)*32 + n-row
//     dword u (0..3) of a lane = its 8 elements of k16-chunk u, i.e.
//     k = kstep*64 + u*16 + (k-half)*8 + j, element j in nibble j (lower k in
//     the lower nibble). One 64-k step of a 32-row tile is one coalesced 1 KB
//     wave load (a dwordx4 per lane) and each MFMA A fragment is one dword.
//   scale image [N/32][K/64][n-row 0..31][2 B]: byte i = the e8m0 exponent of
//     the row's 32-block i of that 64-k step (chunks 0,1 -> byte 0; 2,3 -> 1).
//     One 64 B wave load per 64-k step; both k-halves read the same bytes.
// A fragment is dequantized in registers (w4_frag: four packed converts), the
// values are exact in bf16, and everything after the A operand, staging,
// barriers, MFMA order and store, is the bf16 instantiation's, so the result
// has the bits of the bf16 kernel on the dequantized weight. The step's loads
// are a quarter of the bf16 stream's bytes and the whole ring is a few VGPRs, so
// it holds W4_DEPTH steps: 4 KB per wave in flight. Measured (docs/PERF.md): 2 KB
// to 16 KB per wave agree within 3 % on the 70B gate_up and down shapes, so the
// bytes in flight are not what bounds this kernel; 4 KB runs qkv at M=128 15 %
// faster than 8 KB (fewer VGPRs) and is inside that band everywhere else.
template <int BK>
constexpr int W4_DEPTH = 256 / BK;  // 4 steps at BK=64, 2 at BK=128

// one dword of the code image (8 e2m1 codes) times 2^(e8 - 127) -> A fragment
DEVINL bf16x8 w4_frag(unsigned int q, float scale) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, scale, 3);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// e8m0 byte -> fp32 2^(e8 - 127); the pack keeps e8 in [2, 252], a normal fp32
DEVINL float e8m0_scale(unsigned int e8) { return __uint_as_float(e8 << 23); }

//
// GLU = the SwiGLU store of the gate_up projection (skinny_store_acc): Wp is
// the GLU-interleaved pack and Y is [rows, N / 2]. Nothing before the store
// changes. Instantiated for SPLIT = SWIGLU = W4 = false only.
template <int MT, bool SPLIT, int BK, bool SWIGLU = false, int NW = 4, bool W4 = false, bool GLU = false>
__global__ __launch_bounds__(NW * 64) void skinny_gemm_packed_kernel(
    const unsigned short* __restrict__ Wp, const unsigned short* __restrict__ X,
    unsigned short* __restrict__ Y, float* __restrict__ P,
    const unsigned short* __restrict__ bias,
    int N, long long K, int kc, int nsplit, long long ldx = 0,
    const unsigned char* __restrict__ Ws = nullptr) {
  // SWIGLU: X is the fused [rows, 2K] gate|up GEMM output; the staging
  // computes silu(gate)*up on the fly (row stride ldx = 2K, up at +K) —
  // the intermediate activation tensor never exists (saves its write +
  // read, ~29 MB/layer at 70B B=128, and one launch per layer).
  if (!SWIGLU) ldx = K;
  constexpr int BKC = BK / 16;   // MFMA k-chunks (A fragments) per K-step
  constexpr int XROW = BK + 8;   // padded LDS row stride (elems): conflict-free b128
  constexpr int NT = NW * 64;    // threads
  constexpr int XBUFS = NW == 8 ? 2 : 1;  // LDS images (double-buffered on the wide tile)
  constexpr int XIMG = MT * 32 * XROW;    // elems per image
  const int ntiles = N / (NW * 32);
  const int tile = blockIdx.x % ntiles;
  const int split = blockIdx.x / ntiles;
  // grouped mode: expert blockIdx.y owns rows [e*MT*32, (e+1)*MT*32) of X/Y
  // and its own weight block; gridDim.y == 1 degenerates to the plain GEMM.
  const int e = blockIdx.y;
  if (!W4) Wp += (size_t)e * (size_t)N * (size_t)K;
  X += (size_t)e * (size_t)(MT * 32) * (size_t)K;
  const long long k0 = (long long)split * kc;
  const long long k1 = min(k0 + (long long)kc, K);
  if (k0 >= k1) return;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int tid = threadIdx.x;

  __shared__ unsigned short xs[XBUFS * XIMG];

  floatx16 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (floatx16)(0.f);

  // A stream: packed row for this wave's 32-n tile
  const int n32 = tile * NW + wv;
  const unsigned short* wp = Wp + ((size_t)n32 * (K >> 4) + (k0 >> 4)) * 512 + (size_t)lane * 8;
  // X stage: thread tid covers 16 B pieces p = tid + i*NT (coalesced);
  // row = p / (BK/8), piece-in-row q = p % (BK/8); global [M, K] row-major.
  constexpr int ROWS_PER_I = NT * 8 / BK;  // rows advanced per i (NT threads)
  constexpr int PPT = (MT * 32 + ROWS_PER_I - 1) / ROWS_PER_I;  // pieces per thread per step
  // odd MT on the wide tile at BK=64: the last piece covers only half the
  // threads (rows past MT*32 are neither loaded nor stored)
  constexpr bool RAGGED = (MT * 32) % ROWS_PER_I != 0;
  const bool tail_ok = !RAGGED || tid / (BK / 8) + (PPT - 1) * ROWS_PER_I < MT * 32;
  const int nsteps = (int)((k1 - k0) >> (BK == 64 ? 6 : 7));
  ushort8 xv[PPT];
  bf16x8 a_buf[2][BKC];
  // W4: the ring of code dwordx4 and scale pairs, one of each per 64 k
  constexpr int QD = W4_DEPTH<BK>;
  constexpr int QH = BK / 64;
  uintx4 q_buf[QD][QH];
  unsigned int s_buf[QD][QH];
  const unsigned char* wq = nullptr;
  const unsigned char* wsc = nullptr;
  if (W4) {
    const size_t step64 = ((size_t)e * (N >> 5) + n32) * (size_t)(K >> 6) + (size_t)(k0 >> 6);
    wq = reinterpret_cast<const unsigned char*>(Wp) + step64 * 1024 + (size_t)lane * 16;
    wsc = Ws + step64 * 64 + (size_t)(lane & 31) * 2;
  }
  // per-thread staging base + uniform per-piece offsets: piece p = tid+i*NT
  // has row = tid/(BK/8) + i*ROWS_PER_I and column-piece q = tid%(BK/8), so
  // one VGPR pointer plus SGPR/immediate strides replaces the old per-piece
  // pointer arrays (saves ~10 VGPRs -> a wave/SIMD at MT=4)
  const unsigned short* xpb = X + k0 + (size_t)(tid / (BK / 8)) * ldx + (tid % (BK / 8)) * 8;
  const int xsb = (tid / (BK / 8)) * XROW + (tid % (BK / 8)) * 8;
  const long long xstride_i = (long long)ROWS_PER_I * ldx;

#define SGP_XLOAD(STEP)                                                                        \
  _Pragma("unroll")                                                                            \
  for (int i = 0; i < PPT; ++i)                                                                \
    if (i < PPT - 1 || tail_ok)                                                                \
      xv[i] = skinny_stage_load<SWIGLU>(xpb + i * xstride_i + (size_t)(STEP) * BK, K);
#define SGP_XSTORE(IMG)                                                                        \
  _Pragma("unroll")                                                                            \
  for (int i = 0; i < PPT; ++i)                                                                \
    if (i < PPT - 1 || tail_ok)                                                                \
      *(ushort8*)(xs + (IMG) * XIMG + xsb + i * ROWS_PER_I * XROW) = xv[i];

  // W4: ring slot BUF <- the step that starts OFF64 64-k chunks past wq / wsc.
  // The codes are read once per launch (non-temporal); two steps' scales share
  // a 128 B line, so those loads stay cached.
#define SGP_W4_LOAD(BUF, OFF64)                                                                \
  _Pragma("unroll")                                                                            \
  for (int h = 0; h < QH; ++h) {                                                               \
    q_buf[BUF][h] = __builtin_nontemporal_load(                                                \
        reinterpret_cast<const uintx4*>(wq + ((OFF64) + h) * 1024));                           \
    s_buf[BUF][h] = *reinterpret_cast<const unsigned short*>(wsc + ((OFF64) + h) * 64);        \
  }

  // prologue: stage step 0, preload A(0) and A(1).  The W stream is read
  // exactly once per launch -> non-temporal (L1-bypass) loads; depth-2
  // prefetch keeps 2*BK*32n*2B per wave in flight across staging barriers.
  const unsigned short* wp1 = (nsteps > 1) ? wp + BKC * 512 : wp;  // clamp: no OOB at nsteps==1
  SGP_XLOAD(0)
  if constexpr (W4) {
    // steps 0 .. QD-1, clamped to the last step of a short split (no OOB)
#pragma unroll
    for (int d = 0; d < QD; ++d) {
      const int sd = min(d, nsteps - 1);
      SGP_W4_LOAD(d, (size_t)sd * QH)
    }
    wq += (size_t)QD * QH * 1024;
    wsc += (size_t)QD * QH * 64;
  } else {
#pragma unroll
    for (int u = 0; u < BKC; ++u) {
      a_buf[0][u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp + u * 512));
      a_buf[1][u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp1 + u * 512));
    }
    wp += 2 * BKC * 512;
  }
  SGP_XSTORE(0)
  __syncthreads();

  // NOTE: the A double-buffer index must be a compile-time constant — a
  // dynamic a_buf[s & 1] spills the whole array to scratch (measured 25-40x).
  // Step s reads LDS image BUF (= s & 1) when double-buffered and fills the
  // other one for step s+1: the barrier that ended step s-1 is what lets every
  // wave overwrite the image step s-1 read, so one barrier per step is enough.
#define SGP_STEP(BUF)                                                                          \
  {                                                                                            \
    constexpr int RD = XBUFS == 2 ? (BUF) : 0;                                                 \
    const bool last = (s == nsteps - 1);                                                       \
    if (!last) { SGP_XLOAD(s + 1) }                                                            \
    _Pragma("unroll")                                                                          \
    for (int u = 0; u < BKC; ++u) {                                                            \
      _Pragma("unroll")                                                                        \
      for (int t = 0; t < MT; ++t) {                                                           \
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(                                     \
            xs + RD * XIMG + t * 32 * XROW + (lane & 31) * XROW + u * 16 + (lane >> 5) * 8);   \
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_buf[BUF][u], b, acc[t], 0, 0, 0);   \
      }                                                                                        \
    }                                                                                          \
    if (s + 2 < nsteps) {                                                                      \
      _Pragma("unroll")                                                                        \
      for (int u = 0; u < BKC; ++u)                                                            \
        a_buf[BUF][u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp + u * 512)); \
      wp += BKC * 512;                                                                         \
    }                                                                                          \
    SGP_STEP_TAIL(BUF)                                                                         \
  }
  // the same step on ring slot BUF (= s % QD, QD even) of the W4 stream
#define SGP_STEP_W4(BUF)                                                                       \
  {                                                                                            \
    constexpr int RD = XBUFS == 2 ? ((BUF) & 1) : 0;                                           \
    const bool last = (s == nsteps - 1);                                                       \
    if (!last) { SGP_XLOAD(s + 1) }                                                            \
    _Pragma("unroll")                                                                          \
    for (int u = 0; u < BKC; ++u) {                                                            \
      const unsigned int sp = s_buf[BUF][u >> 2];                                              \
      const bf16x8 a = w4_frag(q_buf[BUF][u >> 2][u & 3],                                      \
                               e8m0_scale((u & 2) ? sp >> 8 : sp & 0xffu));                    \
      _Pragma("unroll")                                                                        \
      for (int t = 0; t < MT; ++t) {                                                           \
        const bf16x8 b = *reinterpret_cast<const bf16x8*>(                                     \
            xs + RD * XIMG + t * 32 * XROW + (lane & 31) * XROW + u * 16 + (lane >> 5) * 8);   \
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[t], 0, 0, 0);               \
      }                                                                                        \
    }                                                                                          \
    if (s + QD < nsteps) {                                                                     \
      SGP_W4_LOAD(BUF, (size_t)0)                                                              \
      wq += QH * 1024;                                                                         \
      wsc += QH * 64;                                                                          \
    }                                                                                          \
    SGP_STEP_TAIL((BUF) & 1)                                                                   \
  }
  // staging tail of a step that read LDS image BUF: fill the image of step s+1.
  // GLU, last step: the branch around this tail goes from the step's last MFMA
  // to the store, and on that taken edge the compiler pads the MFMA-write ->
  // accumulator-read wait states for the fall-through path only. The GLU store
  // reads acc[15] first; at MT = 1 that read came 7 states after the MFMA and
  // returned the sum without the last k-chunk (measured: every output that uses
  // it, whenever the last step is the odd one after the loop). The nops sit on
  // that edge, ahead of the register copies the store begins with: 20 states
  // cover the longest MFMA. The other instances are compiled as before.
#define SGP_STEP_TAIL(BUF)                                                                   \
    if (!last) {                                                                               \
      if (XBUFS == 1) __syncthreads();                                                         \
      SGP_XSTORE(XBUFS == 2 ? 1 - (BUF) : 0)                                                   \
      __syncthreads();                                                                         \
    } else if (GLU) {                                                                          \
      asm volatile("s_nop 9\n\ts_nop 9");                                                      \
    }

  int s = 0;
  if constexpr (W4) {
    // QD steps per trip, one per ring slot, then the up to QD-1 left over
#define SGP_W4_ITER(BUF) { SGP_STEP_W4(BUF) ++s; }
#define SGP_W4_REST(BUF) if (s < nsteps) SGP_W4_ITER(BUF)
    while (s + QD <= nsteps) {
      SGP_W4_ITER(0) SGP_W4_ITER(1)
      if constexpr (QD == 4) { SGP_W4_ITER(2) SGP_W4_ITER(3) }
    }
    SGP_W4_REST(0)
    if constexpr (QD == 4) { SGP_W4_REST(1) SGP_W4_REST(2) }
#undef SGP_W4_ITER
#undef SGP_W4_REST
  } else {
    while (s + 2 <= nsteps) {
      SGP_STEP(0);
      ++s;
      SGP_STEP(1);
      ++s;
    }
    if (s < nsteps) SGP_STEP(0);
  }
#undef SGP_STEP
#undef SGP_STEP_W4
#undef SGP_STEP_TAIL
#undef SGP_W4_LOAD
#undef SGP_XLOAD
#undef SGP_XSTORE

  // rows_total spans all experts
  skinny_store_acc<MT, SPLIT, false, GLU>(acc, Y, P, bias, N, split, gridDim.y * MT * 32,
                                          e * MT * 32 + (lane & 31),
                                          tile * (NW * 32) + wv * 32 + 4 * (lane >> 5));
}

// ---------------------------------------------------------------------------
// v3: packed-A + register-resident-X variant for the M=128/256 decode shapes.
// The LDS-staged v2 wins at M<=64, but at MT>=4 its X staging doubles
// (16 KB/step), the barrier pairs serialize the A stream, and the staging
// registers push the allocation to 156+ VGPRs (3 waves/SIMD).  Here X is
// never staged: each lane loads its B fragments straight from global
// (16 B per lane, same pattern as v1's B path).  X is tiny (M x K bf16,
// 2-4 MB) and every n-tile re-reads it, so after the first touch the
// fragments come from L2/L3, not HBM -- the gather that made v1's A path
// 2.0 TB/s is harmless on the B side.  No LDS, no barriers; A keeps v2's
// coalesced non-temporal 1 KB wave streams with depth-2 step prefetch.
// B chunks are loaded just-in-time per 16-k chunk (bb[MT] live registers):
// at MT=4 the allocation stays ~128 VGPRs = 4 waves/SIMD, and the vmcnt
// wait on one chunk's L2 hit is covered by the other waves' MFMA clusters.
// ---------------------------------------------------------------------------
template <int MT, bool SPLIT>
__global__ __launch_bounds__(256) void skinny_gemm_packed_xreg_kernel(
    const unsigned short* __restrict__ Wp, const unsigned short* __restrict__ X,
    unsigned short* __restrict__ Y, float* __restrict__ P,
    const unsigned short* __restrict__ bias,
    int N, long long K, int kc, int nsplit) {
  const int ntiles = N >> 7;
  const int tile = blockIdx.x % ntiles;
  const int split = blockIdx.x / ntiles;
  const int e = blockIdx.y;  // grouped mode (gridDim.y == 1 for plain GEMM)
  Wp += (size_t)e * (size_t)N * (size_t)K;
  X += (size_t)e * (size_t)(MT * 32) * (size_t)K;
  const long long k0 = (long long)split * kc;
  const long long k1 = min(k0 + (long long)kc, K);
  if (k0 >= k1) return;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int n32 = tile * 4 + wv;

  const unsigned short* wp = Wp + ((size_t)n32 * (K >> 4) + (k0 >> 4)) * 512 + (size_t)lane * 8;
  // B fragment base per m-tile: row (t*32 + lane&31), k-half (lane>>5)*8
  const unsigned short* xt[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
    xt[t] = X + (size_t)(t * 32 + (lane & 31)) * K + k0 + ((lane >> 5) * 8);

  floatx16 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (floatx16)(0.f);

  const int nsteps = (int)((k1 - k0) >> 6);  // 64-k steps, 4 k16-chunks each
  bf16x8 a_buf[2][4];
  const unsigned short* wp1 = (nsteps > 1) ? wp + 4 * 512 : wp;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    a_buf[0][u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp + u * 512));
    a_buf[1][u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp1 + u * 512));
  }
  wp += 2 * 4 * 512;

#define XRG_STEP(BUF)                                                                         \
  {                                                                                           \
    const long long kk = (long long)s * 64;                                                   \
    _Pragma("unroll")                                                                         \
    for (int u = 0; u < 4; ++u) {                                                             \
      bf16x8 bb[MT];                                                                          \
      _Pragma("unroll")                                                                       \
      for (int t = 0; t < MT; ++t)                                                            \
        bb[t] = *reinterpret_cast<const bf16x8*>(xt[t] + kk + u * 16);                        \
      _Pragma("unroll")                                                                       \
      for (int t = 0; t < MT; ++t)                                                            \
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_buf[BUF][u], bb[t], acc[t], 0, 0, 0); \
    }                                                                                         \
    if (s + 2 < nsteps) {                                                                     \
      _Pragma("unroll")                                                                       \
      for (int u = 0; u < 4; ++u)                                                             \
        a_buf[BUF][u] = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(wp + u * 512)); \
      wp += 4 * 512;                                                                          \
    }                                                                                         \
  }

  int s = 0;
  while (s + 2 <= nsteps) {
    XRG_STEP(0);
    ++s;
    XRG_STEP(1);
    ++s;
  }
  if (s < nsteps) XRG_STEP(0);
#undef XRG_STEP

  skinny_store_acc<MT, SPLIT>(acc, Y, P, bias, N, split, gridDim.y * MT * 32,
                              e * MT * 32 + (lane & 31), tile * 128 + wv * 32 + 4 * (lane >> 5));
}

// fp8 (OCP e4m3) W8A8 variant: same structure as the bf16 packed kernel but
// operands are e4m3 with per-output-channel weight scales s_w[n] and
// per-token activation scales s_x[m] (dynamic, computed by quant_fp8_rows).
// v_mfma_f32_32x32x16_fp8_fp8 has the SAME fragment geometry as the bf16
// form (8 elements/lane), so the prepack layout carries over at half the
// bytes — decode GEMMs are weight-bandwidth-bound, so fp8 approaches 2x.
// Opt-in serving mode (XOT_FP8_GEMM=1); the benchmark path stays bf16.
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(8))) char fp8x8;

DEVINL long as_i64(fp8x8 v) { return *reinterpret_cast<long*>(&v); }

template <int MT, bool SPLIT>
__global__ __launch_bounds__(256) void skinny_gemm_fp8_kernel(
    const unsigned char* __restrict__ Wp, const unsigned char* __restrict__ X8,
    const float* __restrict__ sw, const float* __restrict__ sx,
    unsigned short* __restrict__ Y, float* __restrict__ P,
    const unsigned short* __restrict__ bias,
    int N, long long K, int kc, int nsplit) {
  const int ntiles = N >> 7;
  const int tile = blockIdx.x % ntiles;
  const int split = blockIdx.x / ntiles;
  const int e = blockIdx.y;  // grouped mode (MoE): expert index
  Wp += (size_t)e * (size_t)N * (size_t)K;
  X8 += (size_t)e * (size_t)(MT * 32) * (size_t)K;
  const long long k0 = (long long)split * kc;
  const long long k1 = min(k0 + (long long)kc, K);
  if (k0 >= k1) return;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  const int tid = threadIdx.x;

  __shared__ unsigned char xs8[MT * 32 * 72];  // fp8 rows, 72 B stride (64 + 8 pad)

  floatx16 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (floatx16)(0.f);

  const int n32 = tile * 4 + wv;
  const unsigned char* wp = Wp + ((size_t)n32 * (K >> 4) + (k0 >> 4)) * 512 + (size_t)lane * 8;
  // X8 staging: thread tid covers 8-byte piece q (8 of them per 64-k row)
  const int xr = tid >> 3, xq = tid & 7;
  const unsigned char* xp = X8 + (size_t)xr * K + k0 + xq * 8;
  const int xs_off = xr * 72 + xq * 8;

  const int nsteps = (int)((k1 - k0) >> 6);
  unsigned long long xv[MT];
  fp8x8 a_buf[2][4];

  const unsigned char* wp1 = (nsteps > 1) ? wp + 4 * 512 : wp;
#pragma unroll
  for (int t = 0; t < MT; ++t) xv[t] = *(const unsigned long long*)(xp + (size_t)t * 32 * K);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    a_buf[0][u] = __builtin_nontemporal_load(reinterpret_cast<const fp8x8*>(wp + u * 512));
    a_buf[1][u] = __builtin_nontemporal_load(reinterpret_cast<const fp8x8*>(wp1 + u * 512));
  }
  wp += 8 * 512;
#pragma unroll
  for (int t = 0; t < MT; ++t) *(unsigned long long*)(xs8 + t * 32 * 72 + xs_off) = xv[t];
  __syncthreads();

#define SGF_STEP(BUF)                                                                          \
  {                                                                                            \
    const bool last = (s == nsteps - 1);                                                       \
    if (!last) {                                                                               \
      _Pragma("unroll")                                                                        \
      for (int t = 0; t < MT; ++t)                                                             \
        xv[t] = *(const unsigned long long*)(xp + (size_t)t * 32 * K + (s + 1) * 64);          \
    }                                                                                          \
    _Pragma("unroll")                                                                          \
    for (int u = 0; u < 4; ++u) {                                                              \
      _Pragma("unroll")                                                                        \
      for (int t = 0; t < MT; ++t) {                                                           \
        const fp8x8 b = *reinterpret_cast<const fp8x8*>(                                       \
            xs8 + t * 32 * 72 + (lane & 31) * 72 + u * 16 + (lane >> 5) * 8);                  \
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(                                   \
            as_i64(a_buf[BUF][u]), as_i64(b), acc[t], 0, 0, 0);                                \
      }                                                                                        \
    }                                                                                          \
    if (s + 2 < nsteps) {                                                                      \
      _Pragma("unroll")                                                                        \
      for (int u = 0; u < 4; ++u)                                                              \
        a_buf[BUF][u] = __builtin_nontemporal_load(reinterpret_cast<const fp8x8*>(wp + u * 512)); \
      wp += 4 * 512;                                                                           \
    }                                                                                          \
    if (!last) {                                                                               \
      __syncthreads();                                                                         \
      _Pragma("unroll")                                                                        \
      for (int t = 0; t < MT; ++t) *(unsigned long long*)(xs8 + t * 32 * 72 + xs_off) = xv[t]; \
      __syncthreads();                                                                         \
    }                                                                                          \
  }

  int s = 0;
  while (s + 2 <= nsteps) {
    SGF_STEP(0);
    ++s;
    SGF_STEP(1);
    ++s;
  }
  if (s < nsteps) SGF_STEP(0);
#undef SGF_STEP

  // epilogue: dequantize acc * s_x[m] * s_w[n]
  skinny_store_acc<MT, SPLIT, true>(acc, Y, P, bias, N, split, gridDim.y * MT * 32,
                                    e * MT * 32 + (lane & 31),
                                    tile * 128 + wv * 32 + 4 * (lane >> 5), sx, sw,
                                    (size_t)e * N);
}

// per-row dynamic e4m3 quantization: x [M, K] bf16 -> x8 [M, K] + s_x [M]
// (s_x = rowmax/448; one 256-thread workgroup per row, K <= 64K)
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(
    const unsigned short* __restrict__ x, unsigned char* __restrict__ x8,
    float* __restrict__ sx, long long K) {
  const long long row = blockIdx.x;
  const unsigned short* xr = x + row * K;
  unsigned char* qr = x8 + row * K;
  float mx = 0.f;
  for (long long i = threadIdx.x * 8; i < K; i += 256 * 8) {
    ushort8 v = *(const ushort8*)(xr + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) mx = fmaxf(mx, fabsf(b2f(v[j])));
  }
  mx = wave_max(mx);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  // not e4m3_scale: an all-zero row keeps scale 1 / inv 0 here
  const float scale = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) / 448.f;
  const float inv = (scale > 0.f) ? 1.f / scale : 0.f;
  if (threadIdx.x == 0) sx[row] = (scale > 0.f) ? scale : 1.f;
  for (long long i = threadIdx.x * 8; i < K; i += 256 * 8) {
    *(long*)(qr + i) = to_e4m3x8(*(const bf16x8*)(xr + i), inv);
  }
}

// combine fp32 split-K partials [S, M, N] -> bf16 [M, N] (+bias)
__global__ __launch_bounds__(256) void skinny_combine_kernel(
    const float* __restrict__ P, unsigned short* __restrict__ Y,
    const unsigned short* __restrict__ bias, long long MN, long long N, int nsplit) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i * 4 < MN; i += stride) {
    const long long base = i * 4;
    floatx4 s = *reinterpret_cast<const floatx4*>(P + base);
    for (int sp = 1; sp < nsplit; ++sp) {
      floatx4 v = *reinterpret_cast<const floatx4*>(P + (size_t)sp * MN + base);
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += v[j];
    }
    unsigned short o[4];
    const long long ncol = base % N;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v = s[j];
      if (bias) v += b2f(bias[ncol + j]);
      o[j] = f2b(v);
    }
    *reinterpret_cast<unsigned long long*>(Y + base) = *reinterpret_cast<unsigned long long*>(o);
  }
}

// Row epilogue of the layer's last projection: combine + residual add + the
// NEXT norm in one pass over the row, one workgroup per row.
//   y  = bf16(sum of the fp32 split-K partials in split order + bias)
//        (PARTIALS; what skinny_combine_kernel writes), or a finished bf16 y
//   h' = bf16(y + res)                      (what the bf16 torch add writes)
//   normed = rmsnorm(h') from the ROUNDED h', as rmsnorm_kernel<false> reads
//            it back (w == null: h' only)
// Every rounding point of the three-launch chain is kept, and the sum of
// squares is rmsnorm_kernel's own: thread t of 256 owns elements
// t*8 + c*2048 (c = 0..7), accumulates them in (c, j) order, then wave_sum and
// the 4 wave partials. So h' and normed are bit-identical to the chain.
// The workgroup is 1024 threads all the same: thread (q, t) = (tid >> 8,
// tid & 255) streams chunks q and q + 4 of thread t's elements (a 128-row
// decode batch is only 128 workgroups; 4 waves each leave the partials'
// stream latency-bound at under half the combine's rate), parks the rounded
// h' in LDS, and the first 256 threads replay rmsnorm_kernel's accumulation
// from there.
constexpr int EPI_Q = 4;  // 256-thread groups per workgroup

template <bool PARTIALS>
__global__ __launch_bounds__(EPI_Q * 256) void skinny_epilogue_kernel(
    const float* __restrict__ P, const unsigned short* __restrict__ y,
    const unsigned short* __restrict__ bias, const unsigned short* __restrict__ res,
    const unsigned short* __restrict__ w, unsigned short* __restrict__ h_out,
    unsigned short* __restrict__ n_out, long long MN, int D, int nsplit, float eps, float w_bias) {
  __shared__ ushort8 hrow[8][256];  // the rounded h' row, [c][t]
  __shared__ float red[4];
  const int row = blockIdx.x;
  const size_t off = (size_t)row * D;
  const int t = threadIdx.x & 255, q = threadIdx.x >> 8;
  float vals[8 / EPI_Q][8];
#pragma unroll
  for (int k = 0; k < 8 / EPI_Q; ++k) {
    const int c = q + k * EPI_Q;
    const int i = t * 8 + c * 256 * 8;
    if (i < D) {
      float yv[8];
      if constexpr (PARTIALS) {
        const float* p = P + off + i;
        floatx4 s0 = *reinterpret_cast<const floatx4*>(p);
        floatx4 s1 = *reinterpret_cast<const floatx4*>(p + 4);
#pragma unroll 8
        for (int sp = 1; sp < nsplit; ++sp) {
          const floatx4 v0 = *reinterpret_cast<const floatx4*>(p + (size_t)sp * MN);
          const floatx4 v1 = *reinterpret_cast<const floatx4*>(p + (size_t)sp * MN + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) { s0[j] += v0[j]; s1[j] += v1[j]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { yv[j] = s0[j]; yv[4 + j] = s1[j]; }
        if (bias) {
          const ushort8 bv = *(const ushort8*)(bias + i);
#pragma unroll
          for (int j = 0; j < 8; ++j) yv[j] += b2f(bv[j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) yv[j] = b2f(f2b(yv[j]));
      } else {
        const ushort8 v = *(const ushort8*)(y + off + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) yv[j] = b2f(v[j]);
      }
      const ushort8 r = *(const ushort8*)(res + off + i);
      ushort8 s;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s[j] = f2b(yv[j] + b2f(r[j]));
        vals[k][j] = b2f(s[j]);
      }
      *(ushort8*)(h_out + off + i) = s;
      hrow[c][t] = s;
    }
  }
  if (w == nullptr) return;
  __syncthreads();
  if (q == 0) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (t * 8 + c * 256 * 8 < D) {
        const ushort8 s = hrow[c][t];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = b2f(s[j]);
          acc += f * f;
        }
      }
    }
    // wave reduce then cross-wave through LDS
    acc = wave_sum(acc);
    if ((t & 63) == 0) red[t >> 6] = acc;
  }
  __syncthreads();
  const float total = red[0] + red[1] + red[2] + red[3];
  const float inv = rsqrtf(total / (float)D + eps);
#pragma unroll
  for (int k = 0; k < 8 / EPI_Q; ++k) {
    const int i = t * 8 + (q + k * EPI_Q) * 256 * 8;
    if (i < D) {
      ushort8 wv = *(const ushort8*)(w + i);
      ushort8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2b(vals[k][j] * inv * (b2f(wv[j]) + w_bias));
      *(ushort8*)(n_out + off + i) = o;
    }
  }
}

// ===========================================================================
// host bindings
// ===========================================================================

#define CHK(x) TORCH_CHECK(x, #x)

static inline hipStream_t cur_stream() {
  return (hipStream_t)c10::hip::getCurrentHIPStream().stream();
}

// runtime value -> compile-time tag handed to a generic lambda
template <int V>
using IntC = std::integral_constant<int, V>;

// v in 1..8 -> f(IntC<v>)
template <class F>
static void dispatch_1to8(int v, const char* what, F&& f) {
  switch (v) {
    case 1: f(IntC<1>{}); break;
    case 2: f(IntC<2>{}); break;
    case 3: f(IntC<3>{}); break;
    case 4: f(IntC<4>{}); break;
    case 5: f(IntC<5>{}); break;
    case 6: f(IntC<6>{}); break;
    case 7: f(IntC<7>{}); break;
    case 8: f(IntC<8>{}); break;
    default: TORCH_CHECK(false, what, " out of range: ", v);
  }
}

// v -> f(std::true_type / std::false_type)
template <class F>
static void dispatch_bool(bool v, F&& f) {
  if (v) f(std::true_type{}); else f(std::false_type{});
}

// head dim of the fragment-packed GQA cache -> IntC<128> / IntC<256>
template <typename F>
static void dispatch_packed_hd(int hd, const char* what, F&& f) {
  switch (hd) {
    case 128: f(IntC<128>{}); break;
    case 256: f(IntC<256>{}); break;
    default: TORCH_CHECK(false, what, ": head_dim must be 128 or 256, got ", hd);
  }
}

// kp [B, KVH, T32/16, hd/32, 64, 8] and vp [B, KVH, hd/16, T32/32, 64, 8] of one head dim
static void check_packed_gqa_shapes(const char* what, const torch::Tensor& kp, const torch::Tensor& vp, int hd) {
  TORCH_CHECK(kp.dim() == 6 && vp.dim() == 6 && kp.size(3) == hd / 32 && vp.size(2) == hd / 16
              && vp.size(3) * 2 == kp.size(2),
              what, ": packed cache copies do not match head_dim ", hd,
              " (accepted head dims: 128, 256; kp [B, KVH, T32/16, hd/32, 64, 8], vp [B, KVH, hd/16, T32/32, 64, 8])");
}

// packed-cache arguments of the append kernels: bf16 copies, or e4m3 copies
// (uint8 tensors), which come with fp32 scale tensors
struct PackedCachePtrs {
  unsigned short* kp = nullptr;
  unsigned short* vp = nullptr;
  unsigned char* kp8 = nullptr;
  unsigned char* vp8 = nullptr;
};

static PackedCachePtrs packed_cache_ptrs(const torch::Tensor& kp, const torch::Tensor& vp) {
  CHK(kp.is_contiguous() && vp.is_contiguous());
  PackedCachePtrs p;
  if (kp.dtype() == torch::kUInt8) {
    p.kp8 = (unsigned char*)kp.data_ptr();
    p.vp8 = (unsigned char*)vp.data_ptr();
  } else {
    p.kp = (unsigned short*)kp.data_ptr();
    p.vp = (unsigned short*)vp.data_ptr();
  }
  return p;
}

static float* fp8_scale_ptr(const c10::optional<torch::Tensor>& s) {
  CHK(s.has_value() && s->dtype() == torch::kFloat32 && s->is_contiguous());
  return s->data_ptr<float>();
}

// split-K tile threshold for the skinny GEMMs: if the n-tile grid alone
// reaches ~1.5 blocks/CU (384 on MI355X's 256 CUs), splitting K only adds
// partial-write + combine overhead (measured: gate_up 448 tiles 176 -> 162 us
// unsplit); below it, split K until ~2 blocks/CU. Overridable for tuning.
// Read per call, like XOT_SKINNY_BK64 and XOT_SKINNY_BN: the equality tests of
// the unsplit GLU launch set it to get an unsplit plain plan to compare with.
static int skinny_target_blocks() {
  const char* e = getenv("XOT_SKINNY_TARGET");
  return e ? atoi(e) : 384;
}

torch::Tensor rmsnorm(torch::Tensor x, torch::Tensor w, double eps, double w_bias) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.is_contiguous());
  const int D = x.size(-1);
  CHK(D % 8 == 0 && D <= 16384);
  const int rows = x.numel() / D;
  auto out = torch::empty_like(x);
  hipLaunchKernelGGL((rmsnorm_kernel<false>), dim3(rows), dim3(256), 0, cur_stream(),
                     (const unsigned short*)x.data_ptr(), nullptr,
                     (const unsigned short*)w.data_ptr(), (unsigned short*)out.data_ptr(),
                     nullptr, D, (float)eps, (float)w_bias);
  return out;
}

std::vector<torch::Tensor> rmsnorm_residual(torch::Tensor x, torch::Tensor res, torch::Tensor w, double eps,
                                            double w_bias) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.is_contiguous() && res.is_contiguous());
  const int D = x.size(-1);
  CHK(D % 8 == 0 && D <= 16384);
  const int rows = x.numel() / D;
  auto out = torch::empty_like(x);
  auto res_out = torch::empty_like(x);
  hipLaunchKernelGGL((rmsnorm_kernel<true>), dim3(rows), dim3(256), 0, cur_stream(),
                     (const unsigned short*)x.data_ptr(), (const unsigned short*)res.data_ptr(),
                     (const unsigned short*)w.data_ptr(), (unsigned short*)out.data_ptr(),
                     (unsigned short*)res_out.data_ptr(), D, (float)eps, (float)w_bias);
  return {out, res_out};
}

void rope_qkv_append(torch::Tensor qkv, torch::Tensor cos, torch::Tensor sin,
                     torch::Tensor positions, c10::optional<torch::Tensor> kc,
                     c10::optional<torch::Tensor> vc, int64_t n_heads, int64_t n_kv_heads, int64_t head_dim,
                     c10::optional<torch::Tensor> kp, c10::optional<torch::Tensor> vp,
                     c10::optional<torch::Tensor> q_norm, c10::optional<torch::Tensor> k_norm,
                     double norm_eps,
                     c10::optional<torch::Tensor> k_scale, c10::optional<torch::Tensor> v_scale) {
  CHK(qkv.is_cuda() && qkv.dtype() == torch::kBFloat16 && qkv.is_contiguous());
  // kc / vc absent: a packed-only cache (kp / vp required), T is then T32
  const bool plain = kc.has_value();
  CHK(plain == vc.has_value());
  if (plain) CHK(kc->is_contiguous() && vc->is_contiguous());
  TORCH_CHECK(plain || (kp.has_value() && vp.has_value()),
              "rope_qkv_append: no plain cache and no packed copies to append to");
  CHK(positions.dtype() == torch::kInt32 && positions.is_cuda());
  const int B = qkv.size(0), S = qkv.size(1);
  const int H = (int)n_heads, KVH = (int)n_kv_heads, hd = (int)head_dim;
  CHK(qkv.size(2) == (H + 2 * KVH) * hd);
  CHK(hd <= 256 && hd % 2 == 0);
  const int npos = (int)positions.numel();
  CHK(npos == S || npos == B * S);
  CHK(positions.is_contiguous());
  PackedCachePtrs pc;
  float* skp = nullptr;
  float* svp = nullptr;
  int T32 = 0;
  if (kp.has_value() && vp.has_value()) {
    TORCH_CHECK(GQA_PACKED_HD(hd), "rope_qkv_append: packed cache copies need head_dim 128 or 256, got ", hd);
    check_packed_gqa_shapes("rope_qkv_append", *kp, *vp, hd);
    T32 = (int)kp->size(2) * 16;
    pc = packed_cache_ptrs(*kp, *vp);
    if (pc.kp8) {
      skp = fp8_scale_ptr(k_scale);
      svp = fp8_scale_ptr(v_scale);
    }
  }
  const int T = plain ? (int)kc->size(2) : T32;
  const unsigned short* qnp = nullptr;
  const unsigned short* knp = nullptr;
  if (q_norm.has_value()) {
    CHK(q_norm->is_contiguous() && q_norm->dtype() == torch::kBFloat16 && q_norm->numel() == hd);
    qnp = (const unsigned short*)q_norm->data_ptr();
  }
  if (k_norm.has_value()) {
    CHK(k_norm->is_contiguous() && k_norm->dtype() == torch::kBFloat16 && k_norm->numel() == hd);
    knp = (const unsigned short*)k_norm->data_ptr();
  }
  const int waves = B * S * (H + 2 * KVH);
  const int blocks = (waves + 3) / 4;
  // rotate pairs per lane: 1 up to hd = 128, 2 up to 256
  dispatch_bool(hd > 128, [&](auto wide) {
    hipLaunchKernelGGL((rope_qkv_append_kernel<decltype(wide)::value ? 2 : 1>), dim3(blocks), dim3(256), 0,
                       cur_stream(),
                       (unsigned short*)qkv.data_ptr(), cos.data_ptr<float>(), sin.data_ptr<float>(),
                       positions.data_ptr<int>(),
                       plain ? (unsigned short*)kc->data_ptr() : nullptr,
                       plain ? (unsigned short*)vc->data_ptr() : nullptr, B, S, H, KVH, hd, T, pc.kp, pc.vp, T32,
                       qnp, knp, (float)norm_eps, npos, pc.kp8, pc.vp8, skp, svp);
  });
}

// Split-KV decode scaffolding shared by attn_decode, attn_decode_mfma and
// attn_decode_mla: the fp32 partial workspace (o[hd] and (m, l) per
// (b * H + head, split)), the bf16 output, and the merge launch.
struct SplitKV {
  torch::Tensor ws_o, ws_ml, out;
  int BH, nsplit, hd;
  // workspace = false: the kernel merges in the workgroup and writes `out`
  // itself — no partials are allocated and merge() is not called
  SplitKV(const torch::Tensor& q, at::IntArrayRef out_shape, int BH, int nsplit, int hd,
          bool workspace = true)
      : BH(BH), nsplit(nsplit), hd(hd) {
    if (workspace) {
      auto opts = torch::TensorOptions().dtype(torch::kFloat32).device(q.device());
      ws_o = torch::empty({(long)BH * nsplit * hd}, opts);
      ws_ml = torch::empty({(long)BH * nsplit * 2}, opts);
    }
    out = torch::empty(out_shape, torch::TensorOptions().dtype(torch::kBFloat16).device(q.device()));
  }
  float* o() const { return ws_o.defined() ? ws_o.data_ptr<float>() : nullptr; }
  float* ml() const { return ws_ml.defined() ? ws_ml.data_ptr<float>() : nullptr; }
  torch::Tensor merge(hipStream_t stream) const {
    auto launch = [&](auto hdc) {
      constexpr int HD = decltype(hdc)::value;
      hipLaunchKernelGGL((attn_decode_merge<HD>), dim3(BH), dim3(HD > 128 ? 256 : 128), 0, stream,
                         o(), ml(), (unsigned short*)out.data_ptr(), nsplit);
    };
    switch (hd) {
      case 64: launch(IntC<64>{}); break;
      case 128: launch(IntC<128>{}); break;
      case 256: launch(IntC<256>{}); break;
      case MLA_LAT: launch(IntC<MLA_LAT>{}); break;
      default: TORCH_CHECK(false, "split-KV merge: unsupported head dim ", hd);
    }
    return out;
  }
};

torch::Tensor attn_decode(torch::Tensor q, torch::Tensor kc, torch::Tensor vc, torch::Tensor seq_lens) {
  // q may be a strided view into the packed qkv tensor: [B, 1, H, hd] with an
  // arbitrary batch stride but contiguous (head, dim) rows.
  CHK(q.is_cuda() && q.dtype() == torch::kBFloat16);
  CHK(q.stride(3) == 1 && q.stride(2) == q.size(3));
  CHK(seq_lens.dtype() == torch::kInt32 && seq_lens.is_cuda());
  const int B = q.size(0), H = q.size(2), hd = q.size(3);
  const long long q_stride = q.stride(0);
  const int KVH = kc.size(1), T = kc.size(2);
  TORCH_CHECK(hd == 64 || hd == 128, "attn_decode: head_dim must be 64 or 128, got ", hd);
  const int rep = H / KVH;
  // fill the 256 CUs: at least ~512 workgroups, chunks >= 128 positions
  int nsplit = std::max(1, 512 / std::max(1, B * KVH));
  nsplit = std::min<int>(nsplit, std::max(1, (T + 127) / 128));
  const SplitKV kv(q, q.sizes(), B * H, nsplit, hd);
  const float scale = 1.0f / sqrtf((float)hd);
  auto stream = cur_stream();
  // up to 8 q heads of each kv head per partial launch
  for (int qh0 = 0; qh0 < rep; qh0 += 8) {
    dispatch_1to8(std::min(8, rep - qh0), "attn_decode: q-heads-per-kv-head slice", [&](auto nq) {
      dispatch_bool(hd == 128, [&](auto wide) {
        constexpr int NQ = decltype(nq)::value, HD = decltype(wide)::value ? 128 : 64;
        hipLaunchKernelGGL((attn_decode_partial<NQ, HD>), dim3(B * KVH * nsplit), dim3(256), 0, stream,
                           (const unsigned short*)q.data_ptr(), (const unsigned short*)kc.data_ptr(),
                           (const unsigned short*)vc.data_ptr(), seq_lens.data_ptr<int>(),
                           kv.o(), kv.ml(), B, H, KVH, T, nsplit, qh0, scale, q_stride);
      });
    });
  }
  return kv.merge(stream);
}

// q: [B, 1, H, hd], hd 128 or 256 (strided batch OK); kp/vp: the packed cache copies.
torch::Tensor attn_decode_mfma(torch::Tensor q, torch::Tensor kp, torch::Tensor vp,
                               torch::Tensor seq_lens, int64_t t_capacity,
                               double scale_in, double softcap, int64_t window,
                               c10::optional<torch::Tensor> k_scale,
                               c10::optional<torch::Tensor> v_scale) {
  CHK(q.is_cuda() && q.dtype() == torch::kBFloat16);
  CHK(q.stride(3) == 1 && q.stride(2) == q.size(3));
  CHK(seq_lens.dtype() == torch::kInt32 && seq_lens.is_cuda());
  CHK(kp.is_contiguous() && vp.is_contiguous());
  const bool fp8 = kp.dtype() == torch::kUInt8;
  const float* skp = nullptr;
  const float* svp = nullptr;
  if (fp8) {
    CHK(k_scale.has_value() && v_scale.has_value());
    skp = k_scale->data_ptr<float>();
    svp = v_scale->data_ptr<float>();
  }
  const int B = q.size(0), H = q.size(2), hd = q.size(3);
  TORCH_CHECK(GQA_PACKED_HD(hd), "attn_decode_mfma: head_dim must be 128 or 256, got ", hd);
  check_packed_gqa_shapes("attn_decode_mfma", kp, vp, hd);
  const int KVH = kp.size(1);
  // a wave scores all H / KVH query heads of its kv head as the 16 rows of one MFMA tile
  TORCH_CHECK(H % KVH == 0 && H / KVH <= 16,
              "attn_decode_mfma: H must be a multiple of KVH with at most 16 query heads per kv head, got H=",
              H, " KVH=", KVH);
  const int T32 = kp.size(2) * 16;
  const long long q_stride = q.stride(0);
  // one wave per (b, kvh, split); target >= ~2048 waves so 16 waves/CU keep
  // the packed-cache stream deep while chunks stay >= 32 positions
  int nsplit = 1;
  while (B * KVH * nsplit * 2 < 4096 && (T32 / (nsplit * 2)) >= 32 && nsplit < 32) nsplit *= 2;
  // nsplit in {1, 2, 4}: every split of a (b, kv-head) sits in one 4-wave
  // workgroup, which then merges through LDS and writes the bf16 rows itself.
  // XOT_ATTN_FUSED_MERGE=0 (read per call) keeps the workspace + merge launch.
  const char* fm_env = getenv("XOT_ATTN_FUSED_MERGE");
  const bool fused = (nsplit == 1 || nsplit == 2 || nsplit == 4)
                     && ((fm_env == nullptr) || (fm_env[0] != '0'));
  const SplitKV kv(q, q.sizes(), B * H, nsplit, hd, !fused);
  const float scale = (scale_in > 0.0) ? (float)scale_in : 1.0f / sqrtf((float)hd);
  auto stream = cur_stream();
  const int waves = B * KVH * nsplit;
  // default ON: measured -1.1 ms/step on 70B B=128 and -0.8 on 8B B=256
  const char* pf_env = getenv("XOT_ATTN_PREFETCH");
  const bool prefetch = (pf_env == nullptr) || (pf_env[0] != '0');
  dispatch_bool(prefetch, [&](auto pf) {
    dispatch_bool(fp8, [&](auto f8) {
      dispatch_packed_hd(hd, "attn_decode_mfma", [&](auto hdc) {
        hipLaunchKernelGGL((attn_decode_mfma_kernel<decltype(pf)::value, decltype(f8)::value, decltype(hdc)::value>),
                           dim3((waves + 3) / 4), dim3(256), 0, stream,
                           (const unsigned short*)q.data_ptr(), (const unsigned short*)kp.data_ptr(),
                           (const unsigned short*)vp.data_ptr(), seq_lens.data_ptr<int>(),
                           kv.o(), kv.ml(), B, H, KVH, T32, nsplit, scale, q_stride,
                           (float)softcap, (int)window, skp, svp,
                           fused ? (unsigned short*)kv.out.data_ptr() : nullptr);
      });
    });
  });
  return fused ? kv.out : kv.merge(stream);
}

// q: [B, S, H, hd], hd 128 or 256 (strided over b/s OK, head rows contiguous); kp/vp: the
// packed cache copies already holding positions [0, start_pos + S).
torch::Tensor attn_prefill_mfma(torch::Tensor q, torch::Tensor kp, torch::Tensor vp,
                                int64_t start_pos, double scale_in, double softcap,
                                int64_t window) {
  CHK(q.is_cuda() && q.dtype() == torch::kBFloat16);
  CHK(q.stride(3) == 1 && q.stride(2) == q.size(3));
  CHK(kp.is_contiguous() && vp.is_contiguous());
  const int B = q.size(0), S = q.size(1), H = q.size(2), hd = q.size(3);
  TORCH_CHECK(GQA_PACKED_HD(hd), "attn_prefill_mfma: head_dim must be 128 or 256, got ", hd);
  TORCH_CHECK(kp.dtype() == torch::kBFloat16, "attn_prefill_mfma: bf16 packed cache copies only");
  check_packed_gqa_shapes("attn_prefill_mfma", kp, vp, hd);
  const int KVH = kp.size(1);
  const int T32 = kp.size(2) * 16;
  CHK(start_pos + S <= T32);
  auto out = torch::empty({B, S, H, hd},
                          torch::TensorOptions().dtype(torch::kBFloat16).device(q.device()));
  const float scale = (scale_in > 0.0) ? (float)scale_in : 1.0f / sqrtf((float)hd);
  dispatch_packed_hd(hd, "attn_prefill_mfma", [&](auto hdc) {
    constexpr int HD = decltype(hdc)::value, NT = ATTN_PREFILL_NT(HD);
    const int qblocks = (S + 64 * NT - 1) / (64 * NT);
    hipLaunchKernelGGL((attn_prefill_mfma_kernel<HD, NT>), dim3(B * qblocks * H), dim3(256), 0, cur_stream(),
                       (const unsigned short*)q.data_ptr(), (const unsigned short*)kp.data_ptr(),
                       (const unsigned short*)vp.data_ptr(), (unsigned short*)out.data_ptr(),
                       B, S, H, KVH, T32, (int)start_pos, q.stride(0), q.stride(1), scale,
                       (float)softcap, (int)window);
  });
  return out;
}

// logits: [T, E] fp32 gate output -> (idx int32 [T,k], w fp32 [T,k]).
std::vector<torch::Tensor> moe_route(torch::Tensor logits, c10::optional<torch::Tensor> bias,
                                     int64_t k, int64_t mode, int64_t n_group,
                                     int64_t topk_group, double routed_scale, bool norm_topk) {
  CHK(logits.is_cuda() && logits.dtype() == torch::kFloat32 && logits.is_contiguous() && logits.dim() == 2);
  const int T = logits.size(0), E = logits.size(1);
  CHK(E <= 256 && k >= 1 && k <= 8 && n_group >= 1 && n_group <= 8);
  const float* bptr = nullptr;
  if (bias.has_value()) {
    CHK(bias->is_contiguous() && bias->dtype() == torch::kFloat32 && bias->numel() == E);
    bptr = bias->data_ptr<float>();
  }
  auto iopts = torch::TensorOptions().dtype(torch::kInt32).device(logits.device());
  auto fopts = torch::TensorOptions().dtype(torch::kFloat32).device(logits.device());
  auto idx = torch::empty({(long)T, (long)k}, iopts);
  auto w = torch::empty({(long)T, (long)k}, fopts);
  hipLaunchKernelGGL(moe_route_kernel, dim3((T + 3) / 4), dim3(256), 0, cur_stream(),
                     logits.data_ptr<float>(), bptr, idx.data_ptr<int>(), w.data_ptr<float>(),
                     T, E, (int)k, (int)mode, (int)n_group, (int)topk_group,
                     (float)routed_scale, norm_topk ? 1 : 0);
  return {idx, w};
}

// idx: [T, k] int32 expert choices -> (gather_tok int32 [E*C], inv_pos
// int32 [T, k]). One workgroup (counting sort in LDS).
std::vector<torch::Tensor> moe_build(torch::Tensor idx, int64_t E, int64_t C) {
  CHK(idx.is_cuda() && idx.dtype() == torch::kInt32 && idx.is_contiguous() && idx.dim() == 2);
  const int T = idx.size(0), k = idx.size(1);
  CHK(E <= 256 && T * k <= 8192 && T <= C);
  auto opts = torch::TensorOptions().dtype(torch::kInt32).device(idx.device());
  auto gather_tok = torch::empty({E * C}, opts);
  auto inv_pos = torch::empty({T, k}, opts);
  hipLaunchKernelGGL(moe_build_kernel, dim3(1), dim3(256), 0, cur_stream(),
                     idx.data_ptr<int>(), gather_tok.data_ptr<int>(),
                     inv_pos.data_ptr<int>(), T, k, (int)E, (int)C);
  return {gather_tok, inv_pos};
}

// y: [E*C, D] bf16 expert outputs, inv_pos [T,k] int32, w [T,k] fp32 ->
// out [T, D] bf16 (deterministic weighted combine, no atomics).
torch::Tensor moe_combine(torch::Tensor y, torch::Tensor inv_pos, torch::Tensor w) {
  CHK(y.is_cuda() && y.dtype() == torch::kBFloat16 && y.is_contiguous());
  CHK(inv_pos.dtype() == torch::kInt32 && inv_pos.is_contiguous());
  CHK(w.dtype() == torch::kFloat32 && w.is_contiguous());
  const int T = inv_pos.size(0), k = inv_pos.size(1);
  const int D = y.size(-1);
  CHK(D % 8 == 0);
  auto out = torch::empty({(long)T, (long)D},
                          torch::TensorOptions().dtype(torch::kBFloat16).device(y.device()));
  const long long n8 = (long long)T * (D / 8);
  const int blocks = (int)std::min<long long>(1024, (n8 + 255) / 256);
  hipLaunchKernelGGL(moe_combine_kernel, dim3(blocks), dim3(256), 0, cur_stream(),
                     (const unsigned short*)y.data_ptr(), inv_pos.data_ptr<int>(),
                     w.data_ptr<float>(), (unsigned short*)out.data_ptr(), T, k, D);
  return out;
}

// q: [B, 1, H, nope+64] bf16 contiguous (raw projections, nope part is the
// un-roped passthrough); q_lat: [B, 1, H, 512] absorbed latent query;
// returns qfull [B, H, 576] with the roped 64-dim tail appended.
std::vector<torch::Tensor> mla_q_prep(torch::Tensor q, torch::Tensor q_lat, torch::Tensor cos,
                                      torch::Tensor sin, torch::Tensor positions,
                                      int64_t nope, bool interleave, bool fp8) {
  CHK(q.is_cuda() && q.dtype() == torch::kBFloat16 && q.is_contiguous());
  CHK(q_lat.is_cuda() && q_lat.dtype() == torch::kBFloat16 && q_lat.is_contiguous());
  CHK(positions.dtype() == torch::kInt32 && positions.is_contiguous());
  const int B = q.size(0), H = q.size(2);
  CHK(q.size(1) == 1 && q.size(3) == nope + MLA_ROPE);
  CHK(q_lat.numel() == (long long)B * H * MLA_LAT);
  const int npos = (int)positions.numel();
  CHK(npos == 1 || npos == B);
  const int waves = B * H;
  // bf16: {qfull}; fp8: {q8, one scale per (b, h)}
  auto qout = torch::empty({(long)B, (long)H, (long)MLA_DQK},
                           q.options().dtype(fp8 ? torch::kUInt8 : torch::kBFloat16));
  torch::Tensor sq;
  if (fp8) sq = torch::empty({(long)B, (long)H}, q.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(mla_q_prep_kernel, dim3((waves + 3) / 4), dim3(256), 0, cur_stream(),
                     (const unsigned short*)q.data_ptr(), (const unsigned short*)q_lat.data_ptr(),
                     cos.data_ptr<float>(), sin.data_ptr<float>(), positions.data_ptr<int>(),
                     fp8 ? nullptr : (unsigned short*)qout.data_ptr(), B, H,
                     (long long)H * (nope + MLA_ROPE), (int)nope, interleave ? 1 : 0, npos,
                     fp8 ? (unsigned char*)qout.data_ptr() : nullptr,
                     fp8 ? sq.data_ptr<float>() : nullptr);
  if (fp8) return {qout, sq};
  return {qout};
}

// ckv: [B, S, 576] raw kv_a output; w: [512] bf16 norm weight; cos/sin
// fp32 [maxT, 32]; lat_c/rot_c: the plain caches viewed [B, T, 512]/[B, T, 64].
void mla_prep_append(torch::Tensor ckv, torch::Tensor w, torch::Tensor cos,
                     torch::Tensor sin, torch::Tensor positions,
                     torch::Tensor lat_c, torch::Tensor rot_c,
                     torch::Tensor kp, torch::Tensor vp, double eps, bool interleave,
                     c10::optional<torch::Tensor> k_scale) {
  CHK(ckv.is_cuda() && ckv.dtype() == torch::kBFloat16 && ckv.is_contiguous());
  CHK(w.dtype() == torch::kBFloat16 && w.is_contiguous() && w.numel() == MLA_LAT);
  CHK(positions.dtype() == torch::kInt32 && positions.is_contiguous());
  CHK(lat_c.is_contiguous() && rot_c.is_contiguous() && kp.is_contiguous() && vp.is_contiguous());
  const int B = ckv.size(0), S = ckv.size(1);
  CHK(ckv.size(2) == MLA_DQK);
  const int T = lat_c.numel() / (B * MLA_LAT);
  const int T32 = (int)kp.size(1) * 16;
  const int npos = (int)positions.numel();
  CHK(npos == S || npos == B * S);
  const int waves = B * S;
  const PackedCachePtrs pc = packed_cache_ptrs(kp, vp);
  float* ksp = pc.kp8 ? fp8_scale_ptr(k_scale) : nullptr;
  hipLaunchKernelGGL(mla_prep_append_kernel, dim3((waves + 3) / 4), dim3(256), 0, cur_stream(),
                     (const unsigned short*)ckv.data_ptr(), (const unsigned short*)w.data_ptr(),
                     cos.data_ptr<float>(), sin.data_ptr<float>(), positions.data_ptr<int>(),
                     (unsigned short*)lat_c.data_ptr(), (unsigned short*)rot_c.data_ptr(),
                     pc.kp, pc.vp, B, S, T, T32, (float)eps, interleave ? 1 : 0, npos,
                     pc.kp8, pc.vp8, ksp);
}

// lat: [B, S, 512] bf16 (post-RMSNorm latent), rot: [B, S, 64] bf16 (roped
// shared key); kp: [B, T32/16, 18, 64, 8], vp: [B, 32, T32/32, 64, 8].
void mla_append(torch::Tensor lat, torch::Tensor rot, torch::Tensor positions,
                torch::Tensor kp, torch::Tensor vp) {
  CHK(lat.is_cuda() && lat.dtype() == torch::kBFloat16 && lat.is_contiguous());
  CHK(rot.is_cuda() && rot.dtype() == torch::kBFloat16 && rot.is_contiguous());
  CHK(positions.dtype() == torch::kInt32 && positions.is_cuda() && positions.is_contiguous());
  CHK(kp.is_contiguous() && vp.is_contiguous());
  const int B = lat.size(0), S = lat.size(1);
  CHK(lat.size(2) == MLA_LAT && rot.size(2) == MLA_ROPE);
  const int T32 = (int)kp.size(1) * 16;
  const int npos = (int)positions.numel();
  CHK(npos == S || npos == B * S);
  const int waves = B * S;
  hipLaunchKernelGGL(mla_append_kernel, dim3((waves + 3) / 4), dim3(256), 0, cur_stream(),
                     (const unsigned short*)lat.data_ptr(), (const unsigned short*)rot.data_ptr(),
                     positions.data_ptr<int>(), (unsigned short*)kp.data_ptr(),
                     (unsigned short*)vp.data_ptr(), B, S, T32, npos);
}

// q: [B, H, 576] bf16 (absorbed latent+rope query); returns out_lat
// [B, H, 512] bf16 (latent-space attention output, pre kv_b-v expansion).
torch::Tensor attn_decode_mla(torch::Tensor q, torch::Tensor kp, torch::Tensor vp,
                              torch::Tensor seq_lens, double scale_in,
                              c10::optional<torch::Tensor> q_scale,
                              c10::optional<torch::Tensor> k_scale) {
  const bool fp8 = kp.dtype() == torch::kUInt8;
  CHK(q.is_cuda() && q.is_contiguous());
  CHK(fp8 ? (q.dtype() == torch::kUInt8) : (q.dtype() == torch::kBFloat16));
  CHK(seq_lens.dtype() == torch::kInt32 && seq_lens.is_cuda());
  CHK(kp.is_contiguous() && vp.is_contiguous());
  const int B = q.size(0), H = q.size(1);
  CHK(q.size(2) == MLA_DQK);
  const int T32 = (int)kp.size(1) * 16;
  const int hgroups = (H + 15) / 16;
  // fill the chip: B*hgroups is small for lite MLA configs (64 x 1), so
  // split the kv range aggressively — one 32-pos tile per split is fine
  // (empty splits merge as -inf partials). 128 WGs on 256 CUs measured
  // 1.1 TB/s; 256+ WGs is the floor for the packed stream.
  int nsplit = 1;
  while (B * hgroups * nsplit * 2 < 4096 && (T32 / (nsplit * 2)) >= 16 && nsplit < 64) nsplit *= 2;
  const SplitKV kv(q, {(long)B, (long)H, (long)MLA_LAT}, B * H, nsplit, MLA_LAT);
  const float scale = (scale_in > 0.0) ? (float)scale_in : 1.0f / sqrtf((float)MLA_DQK);
  auto stream = cur_stream();
  const int waves = B * hgroups * nsplit;
  const float* sqp = nullptr;
  const float* ksp = nullptr;
  if (fp8) {
    CHK(q_scale.has_value() && k_scale.has_value());
    sqp = q_scale->data_ptr<float>();
    ksp = k_scale->data_ptr<float>();
  }
  dispatch_bool(fp8, [&](auto f8) {
    hipLaunchKernelGGL((attn_decode_mla_kernel<decltype(f8)::value>), dim3((waves + 3) / 4), dim3(256),
                       0, stream, (const unsigned short*)q.data_ptr(),
                       (const unsigned short*)kp.data_ptr(), (const unsigned short*)vp.data_ptr(),
                       seq_lens.data_ptr<int>(), kv.o(), kv.ml(), B, H, T32, nsplit, scale, sqp, ksp);
  });
  return kv.merge(stream);
}

torch::Tensor mfma16_probe(torch::Tensor a, torch::Tensor b) {
  CHK(a.is_cuda() && a.dtype() == torch::kBFloat16 && a.is_contiguous() && a.numel() == 16 * 32);
  CHK(b.is_cuda() && b.dtype() == torch::kBFloat16 && b.is_contiguous() && b.numel() == 32 * 16);
  auto d = torch::empty({16, 16}, torch::TensorOptions().dtype(torch::kFloat32).device(a.device()));
  hipLaunchKernelGGL(mfma16_probe_kernel, dim3(1), dim3(64), 0, cur_stream(),
                     (const unsigned short*)a.data_ptr(), (const unsigned short*)b.data_ptr(),
                     d.data_ptr<float>());
  return d;
}

torch::Tensor swiglu(torch::Tensor g, torch::Tensor u) {
  CHK(g.is_cuda() && g.dtype() == torch::kBFloat16 && g.is_contiguous() && u.is_contiguous());
  CHK(g.numel() % 8 == 0);
  auto out = torch::empty_like(g);
  const long long n8 = g.numel() / 8;
  const int blocks = (int)std::min<long long>(2048, (n8 + 255) / 256);
  hipLaunchKernelGGL(swiglu_kernel, dim3(blocks), dim3(256), 0, cur_stream(),
                     (const unsigned short*)g.data_ptr(), (const unsigned short*)u.data_ptr(),
                     (unsigned short*)out.data_ptr(), n8);
  return out;
}

torch::Tensor swiglu_packed(torch::Tensor gu) {
  CHK(gu.is_cuda() && gu.dtype() == torch::kBFloat16 && gu.is_contiguous());
  const int twoI = gu.size(-1);
  CHK(twoI % 16 == 0);
  const int I = twoI / 2;
  const long long rows = gu.numel() / twoI;
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  auto out = torch::empty(sizes, gu.options());
  const long long n8 = rows * (I / 8);
  const int blocks = (int)std::min<long long>(2048, (n8 + 255) / 256);
  hipLaunchKernelGGL(swiglu_packed_kernel, dim3(blocks), dim3(256), 0, cur_stream(),
                     (const unsigned short*)gu.data_ptr(), (unsigned short*)out.data_ptr(), rows, I);
  return out;
}

torch::Tensor geglu_packed(torch::Tensor gu) {
  CHK(gu.is_cuda() && gu.dtype() == torch::kBFloat16 && gu.is_contiguous());
  const int twoI = gu.size(-1);
  CHK(twoI % 16 == 0);
  const int I = twoI / 2;
  const long long rows = gu.numel() / twoI;
  auto sizes = gu.sizes().vec();
  sizes.back() = I;
  auto out = torch::empty(sizes, gu.options());
  const long long n8 = rows * (I / 8);
  const int blocks = (int)std::min<long long>(2048, (n8 + 255) / 256);
  hipLaunchKernelGGL(geglu_packed_kernel, dim3(blocks), dim3(256), 0, cur_stream(),
                     (const unsigned short*)gu.data_ptr(), (unsigned short*)out.data_ptr(), rows, I);
  return out;
}

// ---------------------------------------------------------------------------
// Skinny decode GEMM launchers. The six bound functions below only check
// their arguments and derive shapes; the split-K plan, the compile-time
// kernel dispatch and the allocate / launch / combine sequence live here once.
// ---------------------------------------------------------------------------

struct SkinnyPlan {
  int ntiles;  // 128-wide n-tiles
  int nsplit;  // K splits; 1 = the kernel writes bf16 directly, no combine
  int kc;      // k-range per split, a multiple of k_align
  bool bk128;  // BK=128 staging (packed bf16 kernel only)
};

// E = experts sharing the launch (grid.y); k_align = 16 for the unpacked v1
// kernel, 64 for everything on the prepack. unsplit = never split K (the GLU
// store needs final sums); the BK rule then applies to kc = K.
static SkinnyPlan skinny_plan(long long N, long long K, long long E, int k_align, bool has_bk128,
                              bool unsplit = false) {
  const int ntiles = (int)(N / 128);
  // oversubscribe the 256 CUs (>=2 blocks/CU) while keeping K/SPLITK >= ~1024
  int nsplit = 1;
  const int target = unsplit ? 0 : skinny_target_blocks();
  while (ntiles * nsplit * E < target && (K / (nsplit * 2)) >= 1024 && nsplit < 16) nsplit *= 2;
  const int kc = (int)((K / nsplit + k_align - 1) / k_align * k_align);
  while ((long long)kc * (nsplit - 1) >= K) nsplit--;  // drop empty splits
  // BK=128 halves the staging-barrier count per byte; needs 128-aligned
  // splits. The override is read per call (the GEMM race tool toggles it).
  const bool bk128 = has_bk128 && (K % 128 == 0) && (kc % 128 == 0) && kc >= 2048
                     && getenv("XOT_SKINNY_BK64") == nullptr;
  return {ntiles, nsplit, kc, bk128};
}

// what a launcher's kernel call needs besides its own operands
struct SkinnyLaunch {
  dim3 grid;
  hipStream_t stream;
  unsigned short* Y;           // null when split
  float* P;                    // null when not split
  const unsigned short* bias;  // null when split (the combine adds it)
  int kc, nsplit;
};

// Optional row epilogue of a launcher (skinny_epilogue_kernel): the residual
// to add and the norm that follows; run() fills h (= y + res) and, when a
// norm weight is given, normed (= rmsnorm(h)).
struct SkinnyEpilogue {
  torch::Tensor res;
  c10::optional<torch::Tensor> w;
  double eps, w_bias;
  torch::Tensor h, normed;

  // exactly one of P (fp32 partials [nsplit, rows, D]) and y (bf16 [rows, D])
  void run(const float* P, const unsigned short* y, const unsigned short* bias, long long rows,
           long long D, int nsplit, hipStream_t stream) {
    CHK(res.is_cuda() && res.dtype() == torch::kBFloat16 && res.is_contiguous());
    CHK(res.numel() == rows * D && D % 8 == 0 && D <= 16384);
    const unsigned short* wptr = nullptr;
    h = torch::empty_like(res);
    if (w.has_value()) {
      CHK(w->is_cuda() && w->dtype() == torch::kBFloat16 && w->is_contiguous() && w->numel() == D);
      wptr = (const unsigned short*)w->data_ptr();
      normed = torch::empty_like(res);
    }
    dispatch_bool(P != nullptr, [&](auto partials) {
      hipLaunchKernelGGL((skinny_epilogue_kernel<decltype(partials)::value>), dim3((unsigned)rows),
                         dim3(EPI_Q * 256), 0, stream, P, y, bias, (const unsigned short*)res.data_ptr(), wptr,
                         (unsigned short*)h.data_ptr(),
                         wptr ? (unsigned short*)normed.data_ptr() : nullptr, rows * D, (int)D, nsplit,
                         (float)eps, (float)w_bias);
    });
  }
  std::vector<torch::Tensor> outputs() const {
    return w.has_value() ? std::vector<torch::Tensor>{h, normed} : std::vector<torch::Tensor>{h};
  }
};

// The packed kernel's weight tile per workgroup for this call: 256 rows (8
// waves sharing one staged X image) or 128. The wide tile needs MT >= 4 (at
// smaller M the staged X is a small share of the load traffic and the 128-row
// grid fills the chip better) and N % 256 == 0. Measured default (docs/PERF.md,
// 256-row tile): at rows < 256 the wide tile wins where a workgroup streams
// kc >= 2048 of K (gate_up, down, lm_head: -4..-11 %) and loses on shorter
// streams (qkv: +14..+18 %), where the 128-row tile at BK=64 keeps three
// workgroups per CU resident against one wide one. At rows = 256 the 128-row
// tile is down to one 4-wave workgroup per CU and the wide tile wins
// (-11..-31 %) unless its grid covers under half of the 256 CUs. MT 5..7 are
// not measured and follow MT = 4. XOT_SKINNY_BN=128|256 overrides the default
// and is read per call (the GEMM race tool and the equality tests toggle it);
// an ineligible shape stays on 128 either way.
static bool skinny_wide_tile(long long rows, long long N, long long E, const SkinnyPlan& p) {
  if (rows < 128 || N % 256 != 0) return false;
  const char* bn = getenv("XOT_SKINNY_BN");
  if (bn != nullptr) {
    CHK(strcmp(bn, "128") == 0 || strcmp(bn, "256") == 0);
    return bn[0] == '2';
  }
  if (rows < 256) return p.kc >= 2048;
  return (long long)(p.ntiles / 2) * p.nsplit * E >= 128;
}

// Shared tail of every launcher: validate bias, allocate y (and the fp32
// partials P [nsplit, E*rows, N] when split), launch the kernel that
// `launch(mt, split, bk, nw, L)` names with MT / SPLIT / BK / NW as
// compile-time constants, then combine. rows = rows per expert. PACKED = the
// launcher runs skinny_gemm_packed_kernel, which has the BK=128 staging and
// the 256-row tile (NW = 8); the plan is made from 128-row tiles either way
// and the wide tile only halves grid.x, so P and the combine do not change.
// With an epilogue the row kernel takes the combine's place (split) or
// follows the GEMM's bf16 y (unsplit); its results are left in *epi and the
// returned y is undefined when split. unsplit = plan without split-K (the
// GLU launcher, whose ysizes end in N / 2).
template <bool PACKED, class F>
static torch::Tensor skinny_run(const torch::Tensor& x, at::IntArrayRef ysizes, long long rows,
                                long long N, long long K, long long E,
                                const c10::optional<torch::Tensor>& bias, int k_align, F&& launch,
                                SkinnyEpilogue* epi = nullptr, bool unsplit = false) {
  const unsigned short* bptr = nullptr;
  if (bias.has_value()) {
    CHK(bias->is_contiguous() && bias->dtype() == torch::kBFloat16 && bias->numel() == N);
    bptr = (const unsigned short*)bias->data_ptr();
  }
  const SkinnyPlan p = skinny_plan(N, K, E, k_align, PACKED, unsplit);
  const bool is_split = p.nsplit > 1;
  const bool wide = PACKED && skinny_wide_tile(rows, N, E, p);
  torch::Tensor y;
  if (!(epi && is_split)) y = torch::empty(ysizes, x.options().dtype(torch::kBFloat16));
  torch::Tensor P;
  if (is_split)
    P = torch::empty({p.nsplit, (long)(E * rows), (long)N}, x.options().dtype(torch::kFloat32));
  const SkinnyLaunch L{dim3((wide ? p.ntiles / 2 : p.ntiles) * p.nsplit, (unsigned)E), cur_stream(),
                       is_split ? nullptr : (unsigned short*)y.data_ptr(),
                       is_split ? P.data_ptr<float>() : nullptr,
                       is_split ? nullptr : bptr, p.kc, p.nsplit};
  dispatch_1to8((int)(rows / 32), "skinny GEMM: MT", [&](auto mt) {
    auto with_bk = [&](auto split, auto bk) {
      if constexpr (PACKED && mt.value >= 4) {
        // MT >= 7 on the wide tile stages BK=64: with two BK=128 images in
        // flight the allocator spills (76-224 B/lane of scratch). Same bits,
        // the k order within a split does not depend on BK.
        if (wide) return launch(mt, split, IntC<(mt.value >= 7 ? 64 : bk.value)>{}, IntC<8>{}, L);
      }
      launch(mt, split, bk, IntC<4>{}, L);
    };
    auto with_split = [&](auto split) {
      if constexpr (PACKED) {
        if (p.bk128) return with_bk(split, IntC<128>{});
      }
      with_bk(split, IntC<64>{});
    };
    if (is_split) with_split(std::true_type{}); else with_split(std::false_type{});
  });
  if (epi) {
    if (is_split) epi->run(P.data_ptr<float>(), nullptr, bptr, E * rows, N, p.nsplit, L.stream);
    else epi->run(nullptr, (const unsigned short*)y.data_ptr(), nullptr, E * rows, N, 1, L.stream);
  } else if (is_split) {
    const long long MN = E * rows * N;
    const int blocks = (int)std::min<long long>(2048, (MN / 4 + 255) / 256);
    hipLaunchKernelGGL(skinny_combine_kernel, dim3(blocks), dim3(256), 0, L.stream,
                       P.data_ptr<float>(), (unsigned short*)y.data_ptr(), bptr, MN, N, p.nsplit);
  }
  return y;
}

// Y = x @ W^T (+bias). x: [M, K] bf16 contiguous rows (M <= 256, M % 32 == 0),
// w: [N, K] bf16 contiguous, bias: optional [N] bf16.
torch::Tensor skinny_gemm(torch::Tensor x, torch::Tensor w,
                          c10::optional<torch::Tensor> bias) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16);
  CHK(w.is_cuda() && w.dtype() == torch::kBFloat16 && w.is_contiguous());
  const long long K = w.size(1);
  const int N = (int)w.size(0);
  const long long M = x.numel() / K;
  CHK(x.is_contiguous());
  CHK(M >= 32 && M <= 256 && M % 32 == 0);
  CHK(N % 128 == 0 && K % 16 == 0);
  auto sizes = x.sizes().vec();
  sizes.back() = N;
  return skinny_run<false>(x, sizes, M, N, K, 1, bias, 16,
                           [&](auto mt, auto split, auto, auto, const SkinnyLaunch& L) {
    hipLaunchKernelGGL((skinny_gemm_kernel<mt.value, split.value>), L.grid, dim3(256), 0, L.stream,
                       (const unsigned short*)w.data_ptr(), (const unsigned short*)x.data_ptr(),
                       L.Y, L.P, L.bias, N, K, L.kc, L.nsplit);
  });
}

// Packed variant. wp: the [N/32, K/16, 64, 8] prepack of w (see
// ops.pack_decode_weight), x: [M, K] bf16, M % 32 == 0, K % 64 == 0.
static torch::Tensor skinny_gemm_packed_impl(const torch::Tensor& x, const torch::Tensor& wp, int64_t N,
                                            const c10::optional<torch::Tensor>& bias,
                                            SkinnyEpilogue* epi) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.is_contiguous());
  CHK(wp.is_cuda() && wp.dtype() == torch::kBFloat16 && wp.is_contiguous());
  const long long K = wp.numel() / N;
  const long long M = x.numel() / K;
  CHK(M >= 32 && M <= 256 && M % 32 == 0);
  CHK(N % 128 == 0 && K % 64 == 0);
  auto sizes = x.sizes().vec();
  sizes.back() = (long)N;
  return skinny_run<true>(x, sizes, M, N, K, 1, bias, 64,
                          [&](auto mt, auto split, auto bk, auto nw, const SkinnyLaunch& L) {
    hipLaunchKernelGGL((skinny_gemm_packed_kernel<mt.value, split.value, bk.value, false, nw.value>),
                       L.grid, dim3(nw.value * 64), 0, L.stream,
                       (const unsigned short*)wp.data_ptr(), (const unsigned short*)x.data_ptr(),
                       L.Y, L.P, L.bias, (int)N, K, L.kc, L.nsplit);
  }, epi);
}

torch::Tensor skinny_gemm_packed(torch::Tensor x, torch::Tensor wp, int64_t N,
                                 c10::optional<torch::Tensor> bias) {
  return skinny_gemm_packed_impl(x, wp, N, bias, nullptr);
}

// gate_up projection with the SwiGLU in its store: wp is the GLU-interleaved
// pack (ops.pack_decode_weight_glu) of the fused [gate; up] weight [N, K],
// N = 2I; returns silu(x @ gate^T) * (x @ up^T) as [.., N / 2], the bits of
// swiglu_packed(skinny_gemm_packed(x, plain pack)) where that plan is unsplit.
// Always unsplit; BK and the tile follow the usual rules for that plan.
torch::Tensor skinny_gemm_packed_glu(torch::Tensor x, torch::Tensor wp, int64_t N) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.is_contiguous());
  CHK(wp.is_cuda() && wp.dtype() == torch::kBFloat16 && wp.is_contiguous());
  const long long K = wp.numel() / N;
  const long long M = x.numel() / K;
  CHK(M >= 32 && M <= 256 && M % 32 == 0);
  CHK(N % 128 == 0 && K % 64 == 0 && x.size(-1) == K);
  auto sizes = x.sizes().vec();
  sizes.back() = (long)(N / 2);
  return skinny_run<true>(x, sizes, M, N, K, 1, c10::nullopt, 64,
                          [&](auto mt, auto split, auto bk, auto nw, const SkinnyLaunch& L) {
    if constexpr (!split.value) {
      CHK(L.bias == nullptr && L.nsplit == 1 && L.kc == K);
      hipLaunchKernelGGL((skinny_gemm_packed_kernel<mt.value, false, bk.value, false, nw.value, false, true>),
                         L.grid, dim3(nw.value * 64), 0, L.stream,
                         (const unsigned short*)wp.data_ptr(), (const unsigned short*)x.data_ptr(),
                         L.Y, L.P, L.bias, (int)N, K, L.kc, L.nsplit);
    } else {
      TORCH_CHECK(false, "skinny_gemm_packed_glu: the plan must not split K");
    }
  }, nullptr, /*unsplit=*/true);
}

// K splits of the packed kernel's ordinary plan for a [N, K] weight (the
// model's pack policy asks: the GLU store is for unsplit shapes only)
int64_t skinny_plan_nsplit(int64_t N, int64_t K) {
  CHK(N >= 128 && N % 128 == 0 && K % 64 == 0);
  return skinny_plan(N, K, 1, 64, true).nsplit;
}

// skinny_gemm_packed + row epilogue: returns {h' = y + res} or, with a norm
// weight, {h', rmsnorm(h')}; res: [M, N] bf16.
std::vector<torch::Tensor> skinny_gemm_packed_epilogue(torch::Tensor x, torch::Tensor wp, int64_t N,
                                                       c10::optional<torch::Tensor> bias,
                                                       torch::Tensor res,
                                                       c10::optional<torch::Tensor> norm_w,
                                                       double eps, double w_bias) {
  SkinnyEpilogue epi{res, norm_w, eps, w_bias};
  skinny_gemm_packed_impl(x, wp, N, bias, &epi);
  return epi.outputs();
}

// v3 (register-resident X) launcher — same contract as skinny_gemm_packed.
torch::Tensor skinny_gemm_packed_xreg(torch::Tensor x, torch::Tensor wp, int64_t N,
                                      c10::optional<torch::Tensor> bias) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.is_contiguous());
  CHK(wp.is_cuda() && wp.dtype() == torch::kBFloat16 && wp.is_contiguous());
  const long long K = wp.numel() / N;
  const long long M = x.numel() / K;
  CHK(M >= 32 && M <= 256 && M % 32 == 0);
  CHK(N % 128 == 0 && K % 64 == 0);
  auto sizes = x.sizes().vec();
  sizes.back() = (long)N;
  return skinny_run<false>(x, sizes, M, N, K, 1, bias, 64,
                           [&](auto mt, auto split, auto, auto, const SkinnyLaunch& L) {
    hipLaunchKernelGGL((skinny_gemm_packed_xreg_kernel<mt.value, split.value>),
                       L.grid, dim3(256), 0, L.stream,
                       (const unsigned short*)wp.data_ptr(), (const unsigned short*)x.data_ptr(),
                       L.Y, L.P, L.bias, (int)N, K, L.kc, L.nsplit);
  });
}

// Fused SwiGLU + down-projection decode GEMM: gu is the [M, 2K] fused
// gate|up GEMM output, wp the prepacked down_proj ([N/32,K/16,64,8]);
// computes y = (silu(gate) * up) @ W_down^T with the activation applied in
// the X-staging — the intermediate [M, K] tensor never materializes.
static torch::Tensor skinny_gemm_packed_swiglu_impl(const torch::Tensor& gu, const torch::Tensor& wp,
                                                   int64_t N, const c10::optional<torch::Tensor>& bias,
                                                   SkinnyEpilogue* epi) {
  CHK(gu.is_cuda() && gu.dtype() == torch::kBFloat16 && gu.is_contiguous());
  CHK(wp.is_cuda() && wp.dtype() == torch::kBFloat16 && wp.is_contiguous());
  const long long K = wp.numel() / N;
  const long long M = gu.numel() / (2 * K);
  CHK(gu.size(-1) == 2 * K);
  CHK(M >= 32 && M <= 256 && M % 32 == 0);
  CHK(N % 128 == 0 && K % 64 == 0);
  auto sizes = gu.sizes().vec();
  sizes.back() = (long)N;
  const long long ldx = 2 * K;
  return skinny_run<true>(gu, sizes, M, N, K, 1, bias, 64,
                          [&](auto mt, auto split, auto bk, auto nw, const SkinnyLaunch& L) {
    hipLaunchKernelGGL((skinny_gemm_packed_kernel<mt.value, split.value, bk.value, true, nw.value>),
                       L.grid, dim3(nw.value * 64), 0, L.stream,
                       (const unsigned short*)wp.data_ptr(), (const unsigned short*)gu.data_ptr(),
                       L.Y, L.P, L.bias, (int)N, K, L.kc, L.nsplit, ldx);
  }, epi);
}

torch::Tensor skinny_gemm_packed_swiglu(torch::Tensor gu, torch::Tensor wp, int64_t N,
                                        c10::optional<torch::Tensor> bias) {
  return skinny_gemm_packed_swiglu_impl(gu, wp, N, bias, nullptr);
}

// skinny_gemm_packed_swiglu + row epilogue (see skinny_gemm_packed_epilogue)
std::vector<torch::Tensor> skinny_gemm_packed_swiglu_epilogue(torch::Tensor gu, torch::Tensor wp, int64_t N,
                                                              c10::optional<torch::Tensor> bias,
                                                              torch::Tensor res,
                                                              c10::optional<torch::Tensor> norm_w,
                                                              double eps, double w_bias) {
  SkinnyEpilogue epi{res, norm_w, eps, w_bias};
  skinny_gemm_packed_swiglu_impl(gu, wp, N, bias, &epi);
  return epi.outputs();
}

// h' = y + res and (with a norm weight) rmsnorm(h'), for a y that did not
// come from a packed launcher (hipBLASLt, MoE); the rounding points of
// torch add -> rmsnorm. y, res: bf16, same shape, contiguous.
std::vector<torch::Tensor> add_rmsnorm(torch::Tensor y, torch::Tensor res,
                                       c10::optional<torch::Tensor> norm_w, double eps, double w_bias) {
  CHK(y.is_cuda() && y.dtype() == torch::kBFloat16 && y.is_contiguous() && y.numel() == res.numel());
  const long long D = y.size(-1);
  SkinnyEpilogue epi{res, norm_w, eps, w_bias};
  epi.run(nullptr, (const unsigned short*)y.data_ptr(), nullptr, y.numel() / D, D, 1, cur_stream());
  return epi.outputs();
}

// MoE grouped decode GEMM: x [E, C, K] (C = per-expert token capacity,
// 32..256, %32), wp: stacked prepacks [E, N/32, K/16, 64, 8] -> y [E, C, N].
// One launch for all experts (blockIdx.y = expert).
torch::Tensor skinny_gemm_grouped(torch::Tensor x, torch::Tensor wp, int64_t E, int64_t N) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.is_contiguous());
  CHK(wp.is_cuda() && wp.dtype() == torch::kBFloat16 && wp.is_contiguous());
  const long long K = wp.numel() / (E * N);
  const long long C = x.numel() / (K * E);
  CHK(C >= 32 && C <= 256 && C % 32 == 0);
  CHK(N % 128 == 0 && K % 64 == 0 && E >= 1 && E <= 256);
  return skinny_run<true>(x, {(long)E, (long)C, (long)N}, C, N, K, E, c10::nullopt, 64,
                          [&](auto mt, auto split, auto bk, auto nw, const SkinnyLaunch& L) {
    hipLaunchKernelGGL((skinny_gemm_packed_kernel<mt.value, split.value, bk.value, false, nw.value>),
                       L.grid, dim3(nw.value * 64), 0, L.stream,
                       (const unsigned short*)wp.data_ptr(), (const unsigned short*)x.data_ptr(),
                       L.Y, L.P, L.bias, (int)N, K, L.kc, L.nsplit);
  });
}

// MXFP4 weight-only (W4A16) decode GEMM on the two images of
// ops.pack_decode_weight_mxfp4: wq [E][N/32][K/64][64][16] code bytes, ws
// [E][N/32][K/64][32][2] e8m0 bytes. E == 1: x [.., K] bf16 -> [.., N];
// E > 1: grouped, x [E, C, K] -> [E, C, N]. Same plan, tiles and bits as
// skinny_gemm_packed / skinny_gemm_grouped on the dequantized weight.
static torch::Tensor skinny_gemm_mxfp4_impl(const torch::Tensor& x, const torch::Tensor& wq,
                                           const torch::Tensor& ws, int64_t E, int64_t N,
                                           const c10::optional<torch::Tensor>& bias,
                                           SkinnyEpilogue* epi) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.is_contiguous());
  CHK(wq.is_cuda() && wq.dtype() == torch::kUInt8 && wq.is_contiguous());
  CHK(ws.is_cuda() && ws.dtype() == torch::kUInt8 && ws.is_contiguous());
  CHK(E >= 1 && E <= 256 && N >= 128 && N % 128 == 0);
  const long long K = x.size(-1);
  CHK(K % 64 == 0 && wq.numel() * 2 == E * N * K && ws.numel() * 32 == E * N * K);
  const long long M = x.numel() / (K * E);  // rows per expert
  CHK(M >= 32 && M <= 256 && M % 32 == 0 && x.numel() == E * M * K);
  std::vector<int64_t> sizes = x.sizes().vec();
  if (E > 1) sizes = {(long)E, (long)M, (long)N};
  else sizes.back() = (long)N;
  return skinny_run<true>(x, sizes, M, N, K, E, bias, 64,
                          [&](auto mt, auto split, auto bk, auto nw, const SkinnyLaunch& L) {
    hipLaunchKernelGGL((skinny_gemm_packed_kernel<mt.value, split.value, bk.value, false, nw.value, true>),
                       L.grid, dim3(nw.value * 64), 0, L.stream,
                       (const unsigned short*)wq.data_ptr(), (const unsigned short*)x.data_ptr(),
                       L.Y, L.P, L.bias, (int)N, K, L.kc, L.nsplit, 0LL,
                       (const unsigned char*)ws.data_ptr());
  }, epi);
}

torch::Tensor skinny_gemm_mxfp4(torch::Tensor x, torch::Tensor wq, torch::Tensor ws, int64_t E,
                                int64_t N, c10::optional<torch::Tensor> bias) {
  return skinny_gemm_mxfp4_impl(x, wq, ws, E, N, bias, nullptr);
}

// skinny_gemm_mxfp4 (E = 1) + row epilogue (see skinny_gemm_packed_epilogue)
std::vector<torch::Tensor> skinny_gemm_mxfp4_epilogue(torch::Tensor x, torch::Tensor wq,
                                                      torch::Tensor ws, int64_t N,
                                                      c10::optional<torch::Tensor> bias,
                                                      torch::Tensor res,
                                                      c10::optional<torch::Tensor> norm_w,
                                                      double eps, double w_bias) {
  SkinnyEpilogue epi{res, norm_w, eps, w_bias};
  skinny_gemm_mxfp4_impl(x, wq, ws, 1, N, bias, &epi);
  return epi.outputs();
}

// x: [M, K] bf16 -> (x8 uint8 [M, K], s_x fp32 [M])
std::vector<torch::Tensor> quant_fp8_rows(torch::Tensor x) {
  CHK(x.is_cuda() && x.dtype() == torch::kBFloat16 && x.is_contiguous());
  const long long K = x.size(-1);
  const long long M = x.numel() / K;
  CHK(K % 8 == 0);
  auto x8 = torch::empty({M, K}, torch::TensorOptions().dtype(torch::kUInt8).device(x.device()));
  auto sx = torch::empty({M}, torch::TensorOptions().dtype(torch::kFloat32).device(x.device()));
  hipLaunchKernelGGL(quant_fp8_rows_kernel, dim3((unsigned)M), dim3(256), 0, cur_stream(),
                     (const unsigned short*)x.data_ptr(), (unsigned char*)x8.data_ptr(),
                     sx.data_ptr<float>(), K);
  return {x8, sx};
}

// W8A8 e4m3 decode GEMM. x8/sx from quant_fp8_rows; wp8: fp8 prepack
// [E][N/32][K/16][64][8] bytes; sw: [E, N] fp32 per-channel scales. E == 1
// for plain GEMMs; E > 1 = MoE grouped mode (x8 is [E, C, K]).
torch::Tensor skinny_gemm_fp8(torch::Tensor x8, torch::Tensor sx, torch::Tensor wp8,
                              torch::Tensor sw, int64_t E, int64_t N,
                              c10::optional<torch::Tensor> bias) {
  CHK(x8.is_cuda() && x8.dtype() == torch::kUInt8 && x8.is_contiguous());
  CHK(wp8.is_cuda() && wp8.dtype() == torch::kUInt8 && wp8.is_contiguous());
  CHK(sx.dtype() == torch::kFloat32 && sw.dtype() == torch::kFloat32);
  CHK(sw.is_contiguous() && sx.is_contiguous());
  const long long K = wp8.numel() / (E * N);
  const long long M = x8.numel() / (K * E);  // rows per expert
  CHK(M >= 32 && M <= 256 && M % 32 == 0);
  CHK(N % 128 == 0 && K % 64 == 0 && sw.numel() == E * N && sx.numel() == E * M);
  return skinny_run<false>(x8, {(long)(E * M), (long)N}, M, N, K, E, bias, 64,
                           [&](auto mt, auto split, auto, auto, const SkinnyLaunch& L) {
    hipLaunchKernelGGL((skinny_gemm_fp8_kernel<mt.value, split.value>),
                       L.grid, dim3(256), 0, L.stream,
                       (const unsigned char*)wp8.data_ptr(), (const unsigned char*)x8.data_ptr(),
                       sw.data_ptr<float>(), sx.data_ptr<float>(),
                       L.Y, L.P, L.bias, (int)N, K, L.kc, L.nsplit);
  });
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("quant_fp8_rows", &quant_fp8_rows, "per-row dynamic e4m3 quantization");
  m.def("skinny_gemm_fp8", &skinny_gemm_fp8,
        "W8A8 e4m3 decode GEMM on prepacked weights (per-channel/per-token scales)",
        py::arg("x8"), py::arg("sx"), py::arg("wp8"), py::arg("sw"), py::arg("n_experts"),
        py::arg("n"), py::arg("bias") = py::none());
  m.def("skinny_gemm", &skinny_gemm, "decode GEMM y = x @ w^T (+bias), bf16 MFMA weight-streaming",
        py::arg("x"), py::arg("w"), py::arg("bias") = py::none());
  m.def("skinny_gemm_packed_xreg", &skinny_gemm_packed_xreg,
        "decode GEMM on prepacked weights, register-resident X (M=128/256 shapes)",
        py::arg("x"), py::arg("wp"), py::arg("N"), py::arg("bias") = py::none());
  m.def("skinny_gemm_packed_swiglu", &skinny_gemm_packed_swiglu,
        "fused silu(gate)*up + down-proj decode GEMM on the prepacked weight",
        py::arg("gu"), py::arg("wp"), py::arg("n"), py::arg("bias") = py::none());
  m.def("skinny_gemm_packed", &skinny_gemm_packed,
        "decode GEMM on prepacked weights (MFMA fragment order)",
        py::arg("x"), py::arg("wp"), py::arg("n"), py::arg("bias") = py::none());
  m.def("skinny_gemm_packed_glu", &skinny_gemm_packed_glu,
        "gate_up decode GEMM on the GLU-interleaved prepack with SwiGLU in the store -> [.., n / 2]",
        py::arg("x"), py::arg("wp"), py::arg("n"));
  m.def("skinny_plan_nsplit", &skinny_plan_nsplit,
        "K splits of the packed decode GEMM's plan for a [n, k] weight", py::arg("n"), py::arg("k"));
  m.def("skinny_gemm_packed_epilogue", &skinny_gemm_packed_epilogue,
        "skinny_gemm_packed + fused combine / residual add / following RMSNorm -> [h', normed]",
        py::arg("x"), py::arg("wp"), py::arg("n"), py::arg("bias"), py::arg("res"),
        py::arg("norm_w") = py::none(), py::arg("eps") = 1e-6, py::arg("w_bias") = 0.0);
  m.def("skinny_gemm_packed_swiglu_epilogue", &skinny_gemm_packed_swiglu_epilogue,
        "skinny_gemm_packed_swiglu + fused combine / residual add / following RMSNorm",
        py::arg("gu"), py::arg("wp"), py::arg("n"), py::arg("bias"), py::arg("res"),
        py::arg("norm_w") = py::none(), py::arg("eps") = 1e-6, py::arg("w_bias") = 0.0);
  m.def("add_rmsnorm", &add_rmsnorm,
        "h' = y + res and rmsnorm(h') of the rounded h' in one launch -> [h', normed]",
        py::arg("y"), py::arg("res"), py::arg("norm_w") = py::none(), py::arg("eps") = 1e-6,
        py::arg("w_bias") = 0.0);
  m.def("skinny_gemm_grouped", &skinny_gemm_grouped,
        "MoE grouped decode GEMM on stacked prepacked expert weights",
        py::arg("x"), py::arg("wp"), py::arg("n_experts"), py::arg("n"));
  m.def("skinny_gemm_mxfp4", &skinny_gemm_mxfp4,
        "W4A16 MXFP4 decode GEMM on packed e2m1 codes + e8m0 block scales; grouped when n_experts > 1",
        py::arg("x"), py::arg("wq"), py::arg("ws"), py::arg("n_experts"), py::arg("n"),
        py::arg("bias") = py::none());
  m.def("skinny_gemm_mxfp4_epilogue", &skinny_gemm_mxfp4_epilogue,
        "skinny_gemm_mxfp4 + fused combine / residual add / following RMSNorm -> [h', normed]",
        py::arg("x"), py::arg("wq"), py::arg("ws"), py::arg("n"), py::arg("bias"), py::arg("res"),
        py::arg("norm_w") = py::none(), py::arg("eps") = 1e-6, py::arg("w_bias") = 0.0);
  m.def("swiglu_packed", &swiglu_packed, "SwiGLU on the packed [gate|up] GEMM output");
  m.def("geglu_packed", &geglu_packed, "GeGLU (tanh gelu) on the packed [gate|up] GEMM output");
  m.def("rmsnorm", &rmsnorm, "RMSNorm (bf16, CDNA4); w_bias=1 gives gemma-style (1+w)",
        py::arg("x"), py::arg("w"), py::arg("eps"), py::arg("w_bias") = 0.0);
  m.def("rmsnorm_residual", &rmsnorm_residual, "fused residual add + RMSNorm",
        py::arg("x"), py::arg("res"), py::arg("w"), py::arg("eps"), py::arg("w_bias") = 0.0);
  m.def("rope_qkv_append", &rope_qkv_append,
        "fused (qk-RMSNorm +) RoPE + KV-cache append on packed qkv",
        py::arg("qkv"), py::arg("cos"), py::arg("sin"), py::arg("positions"), py::arg("kc"),
        py::arg("vc"), py::arg("n_heads"), py::arg("n_kv_heads"), py::arg("head_dim"),
        py::arg("kp") = py::none(), py::arg("vp") = py::none(),
        py::arg("q_norm") = py::none(), py::arg("k_norm") = py::none(),
        py::arg("norm_eps") = 1e-6,
        py::arg("k_scale") = py::none(), py::arg("v_scale") = py::none());
  m.def("attn_decode", &attn_decode, "GQA decode attention (flash-decoding split-KV)");
  m.def("attn_decode_mfma", &attn_decode_mfma,
        "GQA decode attention on matrix cores (packed cache, hd=128); "
        "softcap/window: gemma2 logit soft-capping and sliding window",
        py::arg("q"), py::arg("kp"), py::arg("vp"), py::arg("seq_lens"), py::arg("t_capacity"),
        py::arg("scale") = 0.0, py::arg("softcap") = 0.0, py::arg("window") = 0,
        py::arg("k_scale") = py::none(), py::arg("v_scale") = py::none());
  m.def("attn_prefill_mfma", &attn_prefill_mfma,
        "causal GQA prefill flash attention on matrix cores (packed cache, hd=128)",
        py::arg("q"), py::arg("kp"), py::arg("vp"), py::arg("start_pos"),
        py::arg("scale") = 0.0, py::arg("softcap") = 0.0, py::arg("window") = 0);
  m.def("moe_route", &moe_route,
        "fused MoE router: softmax-topk (mode 0) / sigmoid+group-limited (mode 1)",
        py::arg("logits"), py::arg("bias") = py::none(), py::arg("k") = 2,
        py::arg("mode") = 0, py::arg("n_group") = 1, py::arg("topk_group") = 1,
        py::arg("routed_scale") = 1.0, py::arg("norm_topk") = false);
  m.def("moe_build", &moe_build,
        "MoE decode routing: counting-sort token-expert pairs to padded per-expert slots");
  m.def("moe_combine", &moe_combine,
        "MoE decode combine: out[t] = sum_j w[t,j] * y[pos(t,j)] (deterministic)");
  m.def("mla_q_prep", &mla_q_prep,
        "MLA absorbed-query finisher: rope the 64-dim tail + assemble [B,H,576]; "
        "fp8=True returns (q8, per-head scales)",
        py::arg("q"), py::arg("q_lat"), py::arg("cos"), py::arg("sin"), py::arg("positions"),
        py::arg("nope"), py::arg("interleave") = false, py::arg("fp8") = false);
  m.def("mla_prep_append", &mla_prep_append,
        "fused MLA kv prep: latent RMSNorm + shared-key rope + both cache layouts",
        py::arg("ckv"), py::arg("w"), py::arg("cos"), py::arg("sin"), py::arg("positions"),
        py::arg("lat_c"), py::arg("rot_c"), py::arg("kp"), py::arg("vp"), py::arg("eps"),
        py::arg("interleave") = false, py::arg("k_scale") = py::none());
  m.def("mla_append", &mla_append,
        "append MLA latent+rope token stream into the fragment-packed cache");
  m.def("attn_decode_mla", &attn_decode_mla,
        "MLA decode attention (absorbed latent MQA) on matrix cores; fp8 cache mode",
        py::arg("q"), py::arg("kp"), py::arg("vp"), py::arg("seq_lens"),
        py::arg("scale") = 0.0, py::arg("q_scale") = py::none(), py::arg("k_scale") = py::none());
  m.def("mfma16_probe", &mfma16_probe, "v_mfma_f32_16x16x32_bf16 layout probe (tests)");
  m.def("swiglu", &swiglu, "SwiGLU activation");
}
