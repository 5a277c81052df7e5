// Shared helpers for the gfx950 (MI355X / CDNA4) kernels of distributed_llm_inferencing_amd.
//
// Conventions used by every kernel in this directory:
//  * wave = 64 lanes; block sizes are multiples of 64.
//  * bf16 tensors are moved as 16-byte vectors (8 x bf16) wherever the row allows it.
//  * fp32 accumulation everywhere; f32->bf16 through __float2bfloat16, which lowers to
//    v_cvt_pk_bf16_f32 on gfx950 (round-to-nearest-even, NaN-preserving).
//  * every launcher is `extern "C" int dli_*(..., hipStream_t)` returning a hipError_t.
// Comments cite cdna_hip_programming.md and MI355X_MICROARCH.md: the CDNA4 programming guide
// and the measured MI355X microarchitecture notes of the build image (/opt/skills/guides/),
// not files of this repository.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#define DLI_WAVE 64

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint16_t u16;

struct alignas(16) U16x8 { u16 v[8]; };
struct alignas(8) U16x4 { u16 v[4]; };

__device__ __forceinline__ float bf2f(u16 h) { return __uint_as_float(((uint32_t)h) << 16); }

__device__ __forceinline__ u16 f2bf(float f) {
  __hip_bfloat16 b = __float2bfloat16(f);
  return *reinterpret_cast<u16*>(&b);
}

__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
  return (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
}

// 8 bf16 (one 16-B word) -> fp32
__device__ __forceinline__ void unpack8bf(const uint4 v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}

__device__ __forceinline__ void load8(const u16* p, float* f) {
  unpack8bf(*reinterpret_cast<const uint4*>(p), f);
}

__device__ __forceinline__ void store8(u16* p, const float* f) {
  uint4 v;
  v.x = pack2bf(f[0], f[1]); v.y = pack2bf(f[2], f[3]);
  v.z = pack2bf(f[4], f[5]); v.w = pack2bf(f[6], f[7]);
  *reinterpret_cast<uint4*>(p) = v;
}

// FP8 KV cache (ops/reference.py quantize_kv): one OCP e4m3fn byte per element (gfx950's native
// FP8, not the fnuz form), stored = rne(clamp(x * inv_scale, -448, 448)), read = byte * scale.
// The clamp is written out: nothing here relies on the conversion to saturate. (A NaN comes
// out of fminf / fmaxf as a bound, where the reference keeps it; K and V hold none.)
typedef uint8_t fp8;
constexpr float FP8_E4M3_MAX = 448.f;

// The (kv_fp8, scale, scale) tail of the cache writers and readers: an FP8 cache's scales (or
// their inverses) are > 0 (a NaN fails), and only an FP8 cache has scales other than 1
static inline bool kv_scales_ok(int kv_fp8, float k_scale, float v_scale) {
  return kv_fp8 ? k_scale > 0.f && v_scale > 0.f : k_scale == 1.f && v_scale == 1.f;
}

// 8 fp32 -> 8 e4m3fn bytes (one 8-byte store; v_cvt_pk_fp8_f32 rounds to nearest even)
__device__ __forceinline__ void store8_fp8(fp8* p, const float* f, float inv_scale) {
  float c[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
    c[j] = fminf(fmaxf(f[j] * inv_scale, -FP8_E4M3_MAX), FP8_E4M3_MAX);
  uint2 v = make_uint2(0u, 0u);
  v.x = __builtin_amdgcn_cvt_pk_fp8_f32(c[0], c[1], v.x, false);
  v.x = __builtin_amdgcn_cvt_pk_fp8_f32(c[2], c[3], v.x, true);
  v.y = __builtin_amdgcn_cvt_pk_fp8_f32(c[4], c[5], v.y, false);
  v.y = __builtin_amdgcn_cvt_pk_fp8_f32(c[6], c[7], v.y, true);
  *reinterpret_cast<uint2*>(p) = v;
}

// 2 e4m3fn bytes (the low or the high half of w) -> 2 bf16 in one word; exact, every e4m3fn
// value is a bf16 value (v_cvt_scalef32_pk_bf16_fp8 with scale 1)
template <bool HI>
__device__ __forceinline__ uint32_t fp8x2_to_bf16x2(uint32_t w) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const bf16x2_t h = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, HI);
  return __builtin_bit_cast(uint32_t, h);
}

// 16 e4m3fn bytes (one 16-B load) -> 16 bf16 in element order: lo = bytes 0..7, hi = 8..15
__device__ __forceinline__ void fp8x16_to_bf16(const uint4 v, uint4& lo, uint4& hi) {
  lo.x = fp8x2_to_bf16x2<false>(v.x); lo.y = fp8x2_to_bf16x2<true>(v.x);
  lo.z = fp8x2_to_bf16x2<false>(v.y); lo.w = fp8x2_to_bf16x2<true>(v.y);
  hi.x = fp8x2_to_bf16x2<false>(v.z); hi.y = fp8x2_to_bf16x2<true>(v.z);
  hi.z = fp8x2_to_bf16x2<false>(v.w); hi.w = fp8x2_to_bf16x2<true>(v.w);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Block-wide sum for blockDim.x <= 1024; `red` must hold >= 16 floats.
__device__ __forceinline__ float block_sum(float v, float* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  float t = 0.f;
  for (int i = 0; i < nw; ++i) t += red[i];
  return t;
}

// MoE gate (moe.hip moe_route / moe_router kernels, fused_reduce.hip add + RMSNorm + gate):
// softmax over the E logits -> top-k (HF: lowest index on ties) -> weights p / sum(all),
// divided by the sum of the picks when norm_topk (Mixtral; Qwen3-MoE's norm_topk_prob). One
// wave per token; lane l holds the NR <= 4 experts e = l + 64 i in x[i] (E <= 64 NR; an expert
// >= E holds -inf). NR is a compile-time count and every loop over it unrolls, so the logits
// stay in NR registers (no indexed per-thread array). NR = 1 is the E <= 64 gate as it was:
// the lane-local max / sum / argmax over one value are the value itself.
template <int NR>
__device__ __forceinline__ void route_pick_n(const float (&x)[NR], int lane, int E, int k, int t,
                                             float* __restrict__ topk_w,
                                             int* __restrict__ topk_ids, bool norm_topk) {
  float lm = x[0];
#pragma unroll
  for (int i = 1; i < NR; ++i) lm = fmaxf(lm, x[i]);
  const float mx = wave_max(lm);
  float p[NR], ls = 0.f;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    p[i] = lane + 64 * i < E ? __expf(x[i] - mx) : 0.f;
    ls = i == 0 ? p[0] : ls + p[i];
  }
  const float s = wave_sum(ls);
  float mine = 0.f, wsum = 0.f;                        // lane j keeps the j-th pick's weight
  for (int j = 0; j < k; ++j) {
    float bv = lane < E ? p[0] : -3.f;
    int bi = lane;
#pragma unroll
    for (int i = 1; i < NR; ++i) {                     // the lane's own experts, ascending index
      const float v = lane + 64 * i < E ? p[i] : -3.f;
      if (v > bv) { bv = v; bi = lane + 64 * i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                 // argmax, lowest index on ties (HF)
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    const float w = bv / s;
    wsum += w;
    if (lane == j) { mine = w; topk_ids[t * k + j] = bi; }
#pragma unroll
    for (int i = 0; i < NR; ++i)
      if (lane + 64 * i == bi) p[i] = -2.f;            // taken
  }
  if (lane < k) topk_w[t * k + lane] = norm_topk ? mine / wsum : mine;
}

// the E <= 64 gate: lane e < E holds logit e, the others -inf
__device__ __forceinline__ void route_pick(float x, int lane, int E, int k, int t,
                                           float* __restrict__ topk_w,
                                           int* __restrict__ topk_ids, bool norm_topk = true) {
  const float xs[1] = {x};
  route_pick_n<1>(xs, lane, E, k, t, topk_w, topk_ids, norm_topk);
}


// XCD-aware bijective remap of a linear block id (cdna_hip_programming.md §5 'XCD swizzle must be
// bijective'): consecutive logical tiles land on the same XCD (shared L2). Speed only.
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + (orig >> 3);
}

#define DLI_RETURN_LAUNCH() return (int)hipGetLastError()

// fp16 split-K partials (the EPI_SLAB16 GEMM epilogue and its consumers): value x 1/16 in
// fp16 (RNE), read back x 16 — half the bytes of fp32 slabs, |partial| up to ~1e6 in range
constexpr float SLAB16_SCALE = 0.0625f, SLAB16_UNSCALE = 16.f;
__device__ __forceinline__ uint32_t pack2h(float a, float b) {
  const _Float16 ha = (_Float16)a, hb = (_Float16)b;
  return (uint32_t)__builtin_bit_cast(uint16_t, ha) |
         ((uint32_t)__builtin_bit_cast(uint16_t, hb) << 16);
}
__device__ __forceinline__ float h2f(uint32_t bits16) {
  return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
}
// 8 fp16 slab values (one 16-B load) -> fp32, unscaled
__device__ __forceinline__ void unpack8h(const uint4 u, float* f) {
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = h2f(w[i] & 0xffffu) * SLAB16_UNSCALE;
    f[2 * i + 1] = h2f(w[i] >> 16) * SLAB16_UNSCALE;
  }
}

// What a consumer of a GEMM output reads: the bf16 rows themselves, or the split-K partial
// slabs of a GEMM called with C == nullptr, fp32 or fp16 x 1/16 (fmt 1 of the launchers).
enum class QkvSrc { ROWS, SLAB32, SLAB16 };
constexpr int qkv_src_bytes(QkvSrc s) { return s == QkvSrc::SLAB32 ? 4 : 2; }

// Reader of 8 consecutive columns of SPL slabs (ROWS: of the one row), in two phases because
// the callers put their other loads (residual, norm weight, router rows) between them:
// issue() starts every load (SPL x 16 B, fp32 slabs 2 x 16 B each), sum() gives the fp32 sum
// in slab order 0..S-1, starting from +0 as every consumer of the slabs must (a sum of -0
// partials is +0). `off` and `stride` (slab to slab) count elements of the source.
// SPL == 0: `splits` slabs in a runtime loop, nothing in flight ahead of the first add.
template <QkvSrc SRC, int SPL>
struct Slab8 {
  static constexpr int W = SRC == QkvSrc::SLAB32 ? 2 : 1;      // 16-B words per slab
  uint4 u[SPL][W];
  __device__ __forceinline__ void load(int s, const void* src, long off, long stride) {
    static_assert(SRC != QkvSrc::ROWS || SPL == 1, "a row is one source");
    const char* p = static_cast<const char*>(src) + (s * stride + off) * qkv_src_bytes(SRC);
#pragma unroll
    for (int i = 0; i < W; ++i) u[s][i] = reinterpret_cast<const uint4*>(p)[i];
  }
  // (the count is the template's; the last argument exists so that callers of this form and
  // of the runtime-loop form read alike, and a value other than SPL is not looked at)
  __device__ __forceinline__ void issue(const void* src, long off, long stride, int = SPL) {
#pragma unroll
    for (int s = 0; s < SPL; ++s) load(s, src, off, stride);
  }
  __device__ __forceinline__ void sum(float* x) const {
    if constexpr (SRC == QkvSrc::ROWS) {
      unpack8bf(u[0][0], x);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = 0.f;
#pragma unroll
      for (int s = 0; s < SPL; ++s) add8(x, u[s]);
    }
  }
  static __device__ __forceinline__ void add8(float* x, const uint4* v) {
    static_assert(SRC != QkvSrc::ROWS, "a row is read, not summed");
    float f[8];
    if constexpr (SRC == QkvSrc::SLAB16) {
      unpack8h(v[0], f);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        f[4 * i] = __uint_as_float(v[i].x); f[4 * i + 1] = __uint_as_float(v[i].y);
        f[4 * i + 2] = __uint_as_float(v[i].z); f[4 * i + 3] = __uint_as_float(v[i].w);
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] += f[j];
  }
};
template <QkvSrc SRC>
struct Slab8<SRC, 0> {
  const char* p;
  long step;
  int n;
  __device__ __forceinline__ void issue(const void* src, long off, long stride, int splits) {
    p = static_cast<const char*>(src) + off * qkv_src_bytes(SRC);
    step = stride * qkv_src_bytes(SRC);
    n = splits;
  }
  __device__ __forceinline__ void sum(float* x) const {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = 0.f;
    for (int s = 0; s < n; ++s) {
      uint4 v[Slab8<SRC, 1>::W];
#pragma unroll
      for (int i = 0; i < Slab8<SRC, 1>::W; ++i)
        v[i] = reinterpret_cast<const uint4*>(p + s * step)[i];
      Slab8<SRC, 1>::add8(x, v);
    }
  }
};

// issue() of a lane's two column groups (a head's RoPE partners), slab by slab: the order
// under which the 8-slab forms keep the parent's register count (profiles/r9/README.md)
template <QkvSrc SRC, int SPL>
__device__ __forceinline__ void slab8_issue2(Slab8<SRC, SPL>& a, Slab8<SRC, SPL>& b,
                                             const void* src, long off_a, long off_b,
                                             long stride, int splits = SPL) {
  if constexpr (SPL > 0) {
#pragma unroll
    for (int s = 0; s < SPL; ++s) {
      a.load(s, src, off_a, stride);
      b.load(s, src, off_b, stride);
    }
  } else {
    a.issue(src, off_a, stride, splits);
    b.issue(src, off_b, stride, splits);
  }
}
