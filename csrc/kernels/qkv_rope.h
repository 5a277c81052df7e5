// What happens to a QKV GEMM output on its way to attention: bias -> one rounding to bf16
// (the GEMM output's) -> per-head q/k RMSNorm (Qwen3) -> rotate-half RoPE (HF Llama
// convention) -> row store -> paged K/V cache write. One definition for the kernels of
// rope_cache.hip (bf16 rows in place) and fused_reduce.hip (split-K slabs). The fused decode
// kernel of attention_decode.hip does the same steps in its own lane layout, in its own words
// (see the note above it); it shares QkvSrc, kv_cache_row and, in its launcher, qkv_extras_ok.
//
// One lane owns 8 dims of the first half of a head and the matching 8 dims of the second
// half (16-B loads of each), so a head of 128 dims is 8 lanes and the rotation needs no
// cross-lane traffic. cos/sin come from a host-precomputed fp32 table [max_pos, hd]
// (cdna_hip_programming.md App. B: no on-device trig in memory-bound elementwise ops).
// Cache layouts (see ops/reference.py): k_cache and v_cache both [nblk, Hkv, bs, hd].
//
// X (the Qwen families): bias [(hq+2hkv)*hd] (or null) is added in fp32 ahead of the one
// rounding; then every q and k head is RMS-normalised over its hd dims with q_norm_w /
// k_norm_w [hd] (or null) and rounded to bf16 (dli_rmsnorm's rounding: fp32 sum of squares,
// x * rstd * w, one rounding); v gets the bias only. The hd / 16 lanes of a head are
// consecutive, aligned in the wave and leave together at the gid guard, so the sum of
// squares is log2(hd / 16) xor-shuffles.
#pragma once
#include "common.h"

// element offset of (slot, kv head)'s row in a [nblk, Hkv, bs, hd] cache. K and V share the
// token-major layout: whole-row 16-B stores (a transposed V made every decode step a 2-byte
// scatter, i.e. a read-modify-write of a memory sector per element)
__device__ __forceinline__ long kv_cache_row(int slot, int block_size, int hkv, int kvh,
                                             int hd) {
  const int blk = slot / block_size, off = slot - blk * block_size;
  return (((long)blk * hkv + kvh) * block_size + off) * hd;
}

// bias / q_norm_w / k_norm_w of the launchers: bf16, 16-B aligned, or null, the two norm
// weights together; a normalised head's hd / 16 lanes must be a shuffle group
static inline bool qkv_extras_ok(const void* bias, const void* q_norm_w, const void* k_norm_w,
                                 int hd) {
  const int lph = hd / 16;
  return (q_norm_w == nullptr) == (k_norm_w == nullptr) &&
         (q_norm_w == nullptr || (!(lph & (lph - 1)) && lph <= 64)) &&
         !(((uintptr_t)bias | (uintptr_t)q_norm_w | (uintptr_t)k_norm_w) & 15);
}

// The body of rope_cache[_x]_kernel (SRC = ROWS: qkv rows of stride row_stride in place,
// src unused) and splitk_rope_cache[_x]_kernel (slabs [S, T, row_stride] -> qkv rows).
// SPL as in Slab8; the slab forms load positions[t] ahead of the slab loads, and the plain
// ROWS form does not rewrite rows it did not change (v, and all of them with use_rope == 0).
// KV: the cache element, u16 (bf16, the rows as stored in qkv) or fp8 (common.h: the same
// values times k_inv_scale / v_inv_scale, clamped, one 8-byte store per half).
template <QkvSrc SRC, int SPL, bool X, typename KV = u16>
__device__ __forceinline__ void qkv_rope_cache_body(
    u16* __restrict__ qkv, int row_stride, const void* src, int splits,
    const int* __restrict__ positions, const int* __restrict__ slot_mapping,
    const float* __restrict__ cos_sin, KV* __restrict__ k_cache, KV* __restrict__ v_cache,
    int T, int hq, int hkv, int hd, int block_size, int use_rope, const u16* __restrict__ bias,
    const u16* __restrict__ q_norm_w, const u16* __restrict__ k_norm_w, float qk_eps,
    [[maybe_unused]] float k_inv_scale = 1.f, [[maybe_unused]] float v_inv_scale = 1.f) {
  constexpr bool ROWS = SRC == QkvSrc::ROWS;
  const int lanes_per_head = hd >> 4;            // each lane: 8 dims + their partner 8 dims
  const int heads = hq + 2 * hkv;
  const long total = (long)T * heads * lanes_per_head;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= total) return;
  const int c = (int)(gid % lanes_per_head);
  const long th = gid / lanes_per_head;
  const int h = (int)(th % heads);
  const int t = (int)(th / heads);
  const int half = hd >> 1, d0 = c * 8;         // dims [d0, d0+8) and [half+d0, half+d0+8)
  const long col1 = (long)h * hd + d0, col2 = col1 + half;
  const bool is_q = h < hq, is_k = !is_q && h < hq + hkv;
  const bool rope = use_rope && (is_q || is_k);
  int pos = 0;
  if constexpr (!ROWS) pos = rope ? positions[t] : 0;
  u16* row = qkv + (long)t * row_stride;
  float x1[8], x2[8];
  {
    Slab8<SRC, SPL> r1, r2;
    const void* from = ROWS ? qkv : src;         // in place: read through the pointer written
    const long slab = (long)T * row_stride;
    slab8_issue2(r1, r2, from, (long)t * row_stride + col1, (long)t * row_stride + col2, slab,
                 splits);
    r1.sum(x1);
    r2.sum(x2);
  }
  if constexpr (X) {
    if (bias != nullptr) {
      float b1[8], b2[8];
      load8(bias + col1, b1);
      load8(bias + col2, b2);
#pragma unroll
      for (int j = 0; j < 8; ++j) { x1[j] += b1[j]; x2[j] += b2[j]; }
    }
  }
  if constexpr (!ROWS || X) {                    // (a no-op on bf16 rows without a bias)
#pragma unroll
    for (int j = 0; j < 8; ++j) { x1[j] = bf2f(f2bf(x1[j])); x2[j] = bf2f(f2bf(x2[j])); }
  }
  if constexpr (X) {
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
  if (rope) {
    if constexpr (ROWS) pos = positions[t];
    const float* cs = cos_sin + (long)pos * hd;
    // the cache receives exactly the bf16 values stored in qkv
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float co = cs[d0 + j], si = cs[half + d0 + j];
      const float o1 = x1[j] * co - x2[j] * si, o2 = x2[j] * co + x1[j] * si;
      x1[j] = bf2f(f2bf(o1));
      x2[j] = bf2f(f2bf(o2));
    }
  }
  if (rope || !ROWS || X) {
    store8(row + col1, x1);
    store8(row + col2, x2);
  }
  if (is_q || k_cache == nullptr) return;
  const int slot = slot_mapping[t];
  if (slot < 0) return;
  KV* dst = (is_k ? k_cache : v_cache) +
            kv_cache_row(slot, block_size, hkv, is_k ? h - hq : h - hq - hkv, hd);
  if constexpr (sizeof(KV) == 1) {
    const float inv = is_k ? k_inv_scale : v_inv_scale;
    store8_fp8(dst + d0, x1, inv);
    store8_fp8(dst + half + d0, x2, inv);
  } else {
    store8(dst + d0, x1);
    store8(dst + half + d0, x2);
  }
}
