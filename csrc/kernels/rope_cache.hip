// RoPE (rotate-half, HF Llama convention) applied IN PLACE to q and k inside the fused QKV
// activation, fused with the paged KV-cache write — SURVEY.md §2.4 K5/K6.
//
// One lane owns 8 dims of the first half of a head and the matching 8 dims of the second
// half (16-B loads of each), so a head of 128 dims is 8 lanes and the rotation needs no
// cross-lane traffic. cos/sin come from a host-precomputed fp32 table [max_pos, hd]
// (cdna_hip_programming.md App. B: no on-device trig in memory-bound elementwise ops).
//
// Cache layouts (see ops/reference.py): k_cache and v_cache both [nblk, Hkv, bs, hd].
//
// X (dli_rope_cache_x, the Qwen families): before the rotation, bias [(hq+2hkv)*hd] (or
// null) is added to the row and rounded to bf16, then every q and k head is RMS-normalised
// over its hd dims with q_norm_w / k_norm_w [hd] (or null) and rounded to bf16 (dli_rmsnorm's
// rounding: fp32 sum of squares, x * rstd * w, one rounding); v gets the bias only. The
// hd / 16 lanes of a head are consecutive, aligned in the wave and leave together at the
// gid guard, so the sum of squares is log2(hd / 16) xor-shuffles.
#include "common.h"

template <bool X>
__device__ __forceinline__ void rope_cache_body(
    u16* __restrict__ qkv, int row_stride, const int* __restrict__ positions,
    const int* __restrict__ slot_mapping, const float* __restrict__ cos_sin,
    u16* __restrict__ k_cache, u16* __restrict__ v_cache, int T, int hq, int hkv, int hd,
    int block_size, int use_rope, const u16* __restrict__ bias,
    const u16* __restrict__ q_norm_w, const u16* __restrict__ k_norm_w, float qk_eps) {
  const int lanes_per_head = hd >> 4;            // each lane: 8 dims + their partner 8 dims
  const int heads = hq + 2 * hkv;
  const long total = (long)T * heads * lanes_per_head;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const int c = (int)(gid % lanes_per_head);
  const long th = gid / lanes_per_head;
  const int h = (int)(th % heads);
  const int t = (int)(th / heads);
  const int half = hd >> 1;
  u16* base = qkv + (long)t * row_stride + (long)h * hd;
  const int d0 = c * 8;                         // dims [d0, d0+8) and [half+d0, half+d0+8)
  float x1[8], x2[8];
  load8(base + d0, x1);
  load8(base + half + d0, x2);
  const bool is_q = h < hq, is_k = !is_q && h < hq + hkv;
  if constexpr (X) {
    if (bias != nullptr) {
      float b1[8], b2[8];
      load8(bias + (long)h * hd + d0, b1);
      load8(bias + (long)h * hd + half + d0, b2);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x1[j] = bf2f(f2bf(x1[j] + b1[j]));
        x2[j] = bf2f(f2bf(x2[j] + b2[j]));
      }
    }
    if (q_norm_w != nullptr) {
      float ss = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += x1[j] * x1[j] + x2[j] * x2[j];
      // every lane of the wave that passed the guard shuffles (v heads too, unused there)
      for (int o = 1; o < lanes_per_head; o <<= 1) ss += __shfl_xor(ss, o, 64);
      if (is_q || is_k) {
        const float rstd = rsqrtf(ss / hd + qk_eps);
        const u16* wn = is_q ? q_norm_w : k_norm_w;
        float w1[8], w2[8];
        load8(wn + d0, w1);
        load8(wn + half + d0, w2);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          x1[j] = bf2f(f2bf(x1[j] * rstd * w1[j]));
          x2[j] = bf2f(f2bf(x2[j] * rstd * w2[j]));
        }
      }
    }
  }
  if (use_rope && (is_q || is_k)) {
    const float* cs = cos_sin + (long)positions[t] * hd;
    float o1[8], o2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float co = cs[d0 + j], si = cs[half + d0 + j];
      o1[j] = x1[j] * co - x2[j] * si;
      o2[j] = x2[j] * co + x1[j] * si;
    }
    store8(base + d0, o1);
    store8(base + half + d0, o2);
    // cache receives exactly the bf16 values now stored in qkv
#pragma unroll
    for (int j = 0; j < 8; ++j) { x1[j] = bf2f(f2bf(o1[j])); x2[j] = bf2f(f2bf(o2[j])); }
  } else if constexpr (X) {
    store8(base + d0, x1);                      // the biased (normalised) row
    store8(base + half + d0, x2);
  }
  if (is_q || k_cache == nullptr) return;
  const int slot = slot_mapping[t];
  if (slot < 0) return;
  const int blk = slot / block_size, off = slot - blk * block_size;
  // K and V share the token-major [blk, head, off, hd] layout: whole-row 16-B stores (a
  // transposed V made every decode step a 2-byte scatter, i.e. a read-modify-write of a
  // memory sector per element)
  u16* dst = is_k ? k_cache + (((long)blk * hkv + (h - hq)) * block_size + off) * hd
                  : v_cache + (((long)blk * hkv + (h - hq - hkv)) * block_size + off) * hd;
  store8(dst + d0, x1);
  store8(dst + half + d0, x2);
}

__global__ void __launch_bounds__(256) rope_cache_kernel(
    u16* __restrict__ qkv, int row_stride, const int* __restrict__ positions,
    const int* __restrict__ slot_mapping, const float* __restrict__ cos_sin,
    u16* __restrict__ k_cache, u16* __restrict__ v_cache, int T, int hq, int hkv, int hd,
    int block_size, int use_rope) {
  rope_cache_body<false>(qkv, row_stride, positions, slot_mapping, cos_sin, k_cache, v_cache, T,
                         hq, hkv, hd, block_size, use_rope, nullptr, nullptr, nullptr, 0.f);
}

__global__ void __launch_bounds__(256) rope_cache_x_kernel(
    u16* __restrict__ qkv, int row_stride, const int* __restrict__ positions,
    const int* __restrict__ slot_mapping, const float* __restrict__ cos_sin,
    u16* __restrict__ k_cache, u16* __restrict__ v_cache, int T, int hq, int hkv, int hd,
    int block_size, int use_rope, const u16* __restrict__ bias,
    const u16* __restrict__ q_norm_w, const u16* __restrict__ k_norm_w, float qk_eps) {
  rope_cache_body<true>(qkv, row_stride, positions, slot_mapping, cos_sin, k_cache, v_cache, T,
                        hq, hkv, hd, block_size, use_rope, bias, q_norm_w, k_norm_w, qk_eps);
}

// bias / q_norm_w / k_norm_w: bf16, 16-B aligned, or null (the two norm weights together);
// all null = dli_rope_cache
extern "C" int dli_rope_cache_x(void* qkv, int row_stride, const int* positions,
                                const int* slot_mapping, const float* cos_sin, void* k_cache,
                                void* v_cache, int T, int hq, int hkv, int hd, int block_size,
                                int use_rope, const void* bias, const void* q_norm_w,
                                const void* k_norm_w, float qk_eps, hipStream_t st) {
  if (T <= 0) return 0;
  if (hd % 16 != 0) return (int)hipErrorInvalidValue;
  const long total = (long)T * (hq + 2 * hkv) * (hd / 16);
  const int blocks = (int)((total + 255) / 256);
  if (bias == nullptr && q_norm_w == nullptr && k_norm_w == nullptr) {
    rope_cache_kernel<<<blocks, 256, 0, st>>>((u16*)qkv, row_stride, positions, slot_mapping,
                                               cos_sin, (u16*)k_cache, (u16*)v_cache, T, hq, hkv,
                                               hd, block_size, use_rope);
    DLI_RETURN_LAUNCH();
  }
  const int lph = hd / 16;                       // the head's lanes must be a shuffle group
  if ((q_norm_w == nullptr) != (k_norm_w == nullptr) ||
      (q_norm_w != nullptr && ((lph & (lph - 1)) || lph > 64)) ||
      (((uintptr_t)bias | (uintptr_t)q_norm_w | (uintptr_t)k_norm_w) & 15))
    return (int)hipErrorInvalidValue;
  rope_cache_x_kernel<<<blocks, 256, 0, st>>>(
      (u16*)qkv, row_stride, positions, slot_mapping, cos_sin, (u16*)k_cache, (u16*)v_cache, T,
      hq, hkv, hd, block_size, use_rope, (const u16*)bias, (const u16*)q_norm_w,
      (const u16*)k_norm_w, qk_eps);
  DLI_RETURN_LAUNCH();
}

extern "C" int dli_rope_cache(void* qkv, int row_stride, const int* positions,
                              const int* slot_mapping, const float* cos_sin, void* k_cache,
                              void* v_cache, int T, int hq, int hkv, int hd, int block_size,
                              int use_rope, hipStream_t st) {
  return dli_rope_cache_x(qkv, row_stride, positions, slot_mapping, cos_sin, k_cache, v_cache, T,
                          hq, hkv, hd, block_size, use_rope, nullptr, nullptr, nullptr, 0.f, st);
}
