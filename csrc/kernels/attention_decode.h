// What the paged decode attention kernels share (attention_decode.hip: bf16 cache;
// attention_decode_fp8.hip: FP8 cache): the block-table window, the sliding-window bound, the
// Q^T fragment load, the S^T MFMAs, the online-softmax update, the tile loop of the
// one-tile-per-round kernels and the finalize step; and, on the host, the checks and the KV-split
// geometry of dli_decode_attention. See the note at the top of attention_decode.hip for the work
// decomposition and the layouts.
#pragma once
#include "qkv_rope.h"
#include <limits.h>
#include <stdlib.h>

#define DEC_WAVES 4
#define DEC_TILE 32

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// The first 64-block window of the block-table row of tokens [s_begin, s_end), one block id
// per lane (decode_attn_loop's bt_lane0): loaded by the caller so that the load can be
// issued ahead of the prologue's cache write and its fence.
__device__ __forceinline__ int decode_bt_window(const int* __restrict__ block_tables,
                                                int max_blocks, int b, int s_begin, int s_end,
                                                int block_size, int lane) {
  const int last_blk = max(s_end - 1, 0) / block_size;
  return block_tables[(long)b * max_blocks + min(s_begin / block_size + lane, last_blk)];
}

// Sliding window: the query of a decode step sits at position ctx - 1 and sees the keys
// [max(0, ctx - window), ctx), `window` keys with its own; window <= 0 = full attention. The
// bound is per sequence and aligned to neither a tile nor a KV block: every kernel form
// starts its token range (and with it its tiles and its block-table window) there.
// (Wave-uniform like ctx; readfirstlane puts it, and the tile and block-window counters that
// start from it, in scalar registers: the 128-VGPR kernels have none to spare.)
__device__ __forceinline__ int decode_win_lo(int ctx, int window) {
  return window > 0 ? __builtin_amdgcn_readfirstlane(max(0, ctx - window)) : 0;
}

// [s_begin, s_end) of wave wv when WPI waves split the tokens [lo, ctx) by whole tiles
template <int WPI>
__device__ __forceinline__ void decode_wg_range(int lo, int ctx, int wv, int& s_begin,
                                                int& s_end) {
  const int tiles = (ctx - lo + DEC_TILE - 1) / DEC_TILE;
  const int per = (tiles + WPI - 1) / WPI;
  s_begin = min(ctx, lo + wv * per * DEC_TILE);
  s_end = min(ctx, s_begin + per * DEC_TILE);
}

// Q^T fragments (B operand) of item (b, kvh) from bf16 rows: head = col, k-step kk holds dims
// 32kk + 8grp .. +7, or (K8: the k order of the FP8 K rows, see decode_attn_loop)
// 64(kk >> 1) + 16grp + 8(kk & 1) .. +7
template <int HD, bool K8 = false>
__device__ __forceinline__ void load_q_frags(const u16* __restrict__ q, int q_stride, int b,
                                             int kvh, int G, int lane, bf16x8 (&qf)[HD / 32]) {
  const int col = lane & 15, grp = lane >> 4;
  const bool valid = col < G;
  const u16* qp = q + (long)b * q_stride + (long)(kvh * G + (valid ? col : 0)) * HD;
#pragma unroll
  for (int kk = 0; kk < HD / 32; ++kk) {
    const u16* qd = K8 ? qp + 64 * (kk >> 1) + 16 * grp + 8 * (kk & 1) : qp + kk * 32 + grp * 8;
    uint4 v = valid ? *reinterpret_cast<const uint4*>(qd) : make_uint4(0, 0, 0, 0);
    qf[kk] = *reinterpret_cast<bf16x8*>(&v);
  }
}

// S^T = K . Q^T for the two 16-token subtiles of a tile (kreg: the K rows as loaded); the
// lane then holds S^T[tok = t0 + 16s + 4grp + r][head = col]
template <int HD>
__device__ __forceinline__ void decode_scores(uint4 (&kreg)[2][HD / 32],
                                              const bf16x8 (&qf)[HD / 32], f32x4 (&s_acc)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    s_acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < HD / 32; ++kk)
      s_acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          *reinterpret_cast<bf16x8*>(&kreg[s][kk]), qf[kk], s_acc[s], 0, 0, 0);
  }
}

// Online-softmax update of a tile at t0 (tokens >= s_end masked): new running max and partial
// denominator, O rows rescaled, and the tile's P in p: P[head=col][k = 8grp + j] in the
// permuted token order pi(grp, j) = 16(j>>2) + 4grp + (j&3). HW_EXP2: v_exp_f32 as it is (the
// pipelined kernel) instead of exp2f.
template <int HD, bool HW_EXP2>
__device__ __forceinline__ void decode_softmax_update(const f32x4 (&s_acc)[2], int t0,
                                                      int s_end, int grp, float scale_log2,
                                                      float& m_run, float& l_part,
                                                      f32x4 (&o_acc)[HD / 16], float (&p)[8]) {
  auto ex2 = [](float x) { return HW_EXP2 ? __builtin_amdgcn_exp2f(x) : exp2f(x); };
  float tmax = -INFINITY;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int tok = t0 + 16 * s + 4 * grp + r;
      const float v = tok < s_end ? s_acc[s][r] * scale_log2 : -INFINITY;
      p[s * 4 + r] = v;
      tmax = fmaxf(tmax, v);
    }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
  const float m_new = fmaxf(m_run, tmax);
  const float alpha = ex2(m_run - m_new);                      // m_run=-inf -> 0
  m_run = m_new;
  float psum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) { p[j] = ex2(p[j] - m_new); psum += p[j]; }
  l_part = l_part * alpha + psum;
  // rescale O rows (heads 4grp + r) by their head's alpha (held by lane 4grp + r)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float a = __shfl(alpha, 4 * grp + r, 64);
#pragma unroll
    for (int i = 0; i < HD / 16; ++i) o_acc[i][r] *= a;
  }
}

// P as the A operand of P . V (the loop kernels stage their V tile between the update and this)
__device__ __forceinline__ bf16x8 decode_pack_p(const float (&p)[8]) {
  bf16x8 pa;
#pragma unroll
  for (int j = 0; j < 8; ++j) pa[j] = (__bf16)p[j];
  return pa;
}

// The tile loop of the one-tile-per-round kernels: one wave = one (sequence, kv head, split)
// item with its Q^T fragments already in registers. Over tokens [s_begin, s_end) it leaves
// the unnormalised O rows in o_acc, the running max of head `col` in m_run and this lane's
// partial denominator in l_part.
// KV = fp8 (attention_decode_fp8.hip): a K row of hd bytes is hd / 16 chunks of 16 B; the 4
// lanes of token `col` load chunks grp, grp + 4 (one 16-B load each), so lane (col, grp) holds
// dims 64j + 16grp .. +15 and feeds k-step kk = 2j + h with dims 64j + 16grp + 8h .. +7. The
// MFMA sums over k whatever the order, so the Q^T fragment takes the same dims
// (load_q_frags<HD, true>) and nothing is shuffled. V rows: 16-B loads, dequantised on their
// way into the per-wave LDS tile, whose bf16 image and transposing reads are the bf16 cache's.
template <int HD, typename KV = u16>
__device__ __forceinline__ void decode_attn_loop(
    const bf16x8 (&qf)[HD / 32], u16* vt, int lane, int b, int kvh, int s_begin, int s_end,
    const KV* __restrict__ k_cache, const KV* __restrict__ v_cache,
    const int* __restrict__ block_tables, int max_blocks, int hkv, int block_size,
    float scale_log2, int bt_lane0, f32x4 (&o_acc)[HD / 16], float& m_run, float& l_part) {
  constexpr bool FP8 = sizeof(KV) == 1;
  constexpr int DB = HD / 16;     // 16-wide output column blocks
  constexpr int KK = HD / 32;     // MFMA k-steps over head_dim
  constexpr int KC = HD / 64;     // FP8: 16-B chunks of a K row per lane
  constexpr int VROW = HD + 16;   // padded LDS row of the (bf16) V tile, in u16
  constexpr int VE = 16 / sizeof(KV);       // elements per 16-B chunk
  constexpr int VCH = HD / VE;              // 16-B chunks per V row
  constexpr int VP = DEC_TILE * VCH / 64;   // V chunks per lane per tile
  const int col = lane & 15, grp = lane >> 4;
  const int* bt = block_tables + (long)b * max_blocks;
  // the split's block ids, one per lane, read once per 64-block window (token -> block by a
  // lane shuffle): the per-tile K/V loads no longer wait on a dependent block-table load
  const int last_blk = max(s_end - 1, 0) / block_size;
  int win = s_begin / block_size;
  int bt_lane = bt_lane0;
  const long kv_head_stride = (long)block_size * HD;           // elements per (blk, head)
  m_run = -INFINITY;                // running max for head `col` (replicated over groups)
  l_part = 0.f;                     // this lane's partial denominator for head `col`
#pragma unroll
  for (int i = 0; i < DB; ++i) o_acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t0 = s_begin; t0 < s_end; t0 += DEC_TILE) {
    if ((min(t0 + DEC_TILE, s_end) - 1) / block_size - win >= 64) {   // wave-uniform
      win = t0 / block_size;
      bt_lane = bt[min(win + lane, last_blk)];
    }
    // ---- issue every global load of the tile up front (K fragments AND V fragments)
    uint4 kreg[2][KK];
    [[maybe_unused]] uint4 k8[2][KC];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      int tok = t0 + 16 * s + col;
      tok = tok < s_end ? tok : s_end - 1;                     // clamp: always-written rows
      const int blk = __shfl(bt_lane, tok / block_size - win, 64), off = tok % block_size;
      const KV* kp = k_cache + ((long)blk * hkv + kvh) * kv_head_stride + (long)off * HD;
      if constexpr (FP8) {
#pragma unroll
        for (int j = 0; j < KC; ++j)
          k8[s][j] = *reinterpret_cast<const uint4*>(kp + 64 * j + 16 * grp);
      } else {
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
          kreg[s][kk] = *reinterpret_cast<const uint4*>(kp + kk * 32 + grp * 8);
      }
    }
    // V rows t0 .. t0+31 (row-major, 16-B chunks; piece lane + 64m = row r, chunk c)
    uint4 vreg[VP];
#pragma unroll
    for (int m = 0; m < VP; ++m) {
      const int piece = lane + 64 * m, r = piece / VCH, c = piece % VCH;
      const int tok = min(t0 + r, s_end - 1);                  // clamp: always-written rows
      const int blk = __shfl(bt_lane, tok / block_size - win, 64), off = tok % block_size;
      vreg[m] = *reinterpret_cast<const uint4*>(
          v_cache + ((long)blk * hkv + kvh) * kv_head_stride + (long)off * HD + c * VE);
    }
    if constexpr (FP8) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int j = 0; j < KC; ++j) fp8x16_to_bf16(k8[s][j], kreg[s][2 * j], kreg[s][2 * j + 1]);
    }
    f32x4 s_acc[2];
    decode_scores<HD>(kreg, qf, s_acc);
    float p[8];
    decode_softmax_update<HD, false>(s_acc, t0, s_end, grp, scale_log2, m_run, l_part, o_acc, p);
    // stage the V tile as bf16 in this wave's LDS rows (previous tile's reads retired below)
#pragma unroll
    for (int m = 0; m < VP; ++m) {
      const int piece = lane + 64 * m, r = piece / VCH, c = piece % VCH;
      if constexpr (FP8) {
        uint4 lo, hi;
        fp8x16_to_bf16(vreg[m], lo, hi);
        *reinterpret_cast<uint4*>(vt + r * VROW + c * 16) = lo;
        *reinterpret_cast<uint4*>(vt + r * VROW + c * 16 + 8) = hi;
      } else {
        *reinterpret_cast<uint4*>(vt + r * VROW + c * 8) = vreg[m];
      }
    }
    const bf16x8 pa = decode_pack_p(p);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // V tile writes landed (same wave)
    // B operand: rows (tokens) 4grp+q and 16+4grp+q, columns 16i + 4p, transposed by
    // ds_read_b64_tr_b16 (lane 4q+p of each 16-lane group names row q, columns 4p..4p+3)
    const int qrow = (lane >> 2) & 3, pcol = lane & 3;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
      const u16* a0 = vt + (4 * grp + qrow) * VROW + 16 * i + 4 * pcol;
      const u16* a1 = vt + (16 + 4 * grp + qrow) * VROW + 16 * i + 4 * pcol;
      s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(a0));
      s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(a1));
      s16x8 w = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      o_acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, *reinterpret_cast<bf16x8*>(&w),
                                                        o_acc[i], 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads done before next overwrite
  }
}

// denominator of head `col` over the 4 lane groups
__device__ __forceinline__ float decode_l_total(float l_part) {
  const float l_tot = l_part + __shfl_xor(l_part, 16, 64);
  return l_tot + __shfl_xor(l_tot, 32, 64);
}

// Finalize an item: rows 4grp + r of O over their denominators to `out` (one split) or,
// with the (m, l) of each head, to the split workspace
template <int HD>
__device__ __forceinline__ void decode_finalize(const f32x4 (&o_acc)[HD / 16], float m_run,
                                                float l_part, int lane, int b, int kvh,
                                                int split, int G, int hq, int num_splits,
                                                u16* __restrict__ out, float* __restrict__ ws_o,
                                                float* __restrict__ ws_ml) {
  constexpr int DB = HD / 16;
  const int col = lane & 15, grp = lane >> 4;
  const float l_tot = decode_l_total(l_part);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int h = 4 * grp + r;
    const float lr = __shfl(l_tot, h, 64);
    const float mr = __shfl(m_run, h, 64);
    if (h >= G) continue;
    const int qh = kvh * G + h;
    const float inv = lr > 0.f ? 1.f / lr : 0.f;
    if (num_splits == 1) {
      u16* op = out + ((long)b * hq + qh) * HD;
#pragma unroll
      for (int i = 0; i < DB; ++i) op[16 * i + col] = f2bf(o_acc[i][r] * inv);
    } else {
      const long base = ((long)b * hq + qh) * num_splits + split;
      float* wo = ws_o + base * HD;
#pragma unroll
      for (int i = 0; i < DB; ++i) wo[16 * i + col] = o_acc[i][r] * inv;
      if (col == 0) {
        ws_ml[base * 2] = lr > 0.f ? mr : -INFINITY;
        ws_ml[base * 2 + 1] = lr;
      }
    }
  }
}

// The merge of the KV splits' (m, l, O) in the workspace into out [B, hq, hd]
// (decode_reduce_kernel of attention_decode.hip), for every launcher that splits
int decode_reduce_launch(void* out, const float* ws_o, const float* ws_ml, int B, int hq, int hd,
                         int num_splits, hipStream_t st);

// tokens per KV split (whole tiles) when num_splits >= 1 splits divide a span of keys
static inline int decode_split_tokens(int span, int num_splits) {
  const int t = (span + num_splits - 1) / num_splits;
  return t > 0 ? (t + DEC_TILE - 1) / DEC_TILE * DEC_TILE : DEC_TILE;
}

// What dli_decode_attention checks and derives for either cache dtype. window > 0: sliding
// window (decode_win_lo); the splits divide the longest span a sequence can have,
// min(max_context, window) tokens, each offset by its sequence's start, so the work follows
// the window and no split is empty for every sequence.
struct DecodeSplits {
  int window, num_splits, split_tokens;
  float *ws_o, *ws_ml;                    // [B, hq, splits, hd] and [B, hq, splits, 2], or null
};
static inline bool decode_splits(int B, int hq, int hkv, int hd, int block_size,
                                 int max_context, int num_splits, void* workspace, int window,
                                 DecodeSplits& g) {
  if (window < 0) window = 0;
  if (window > 0 && window < max_context) max_context = window;
  if (hq % hkv || hq / hkv > 16 || block_size % 16 || (hd != 64 && hd != 128)) return false;
  if (num_splits < 1) num_splits = 1;
  if (num_splits > 1 && workspace == nullptr) return false;
  g.window = window;
  g.num_splits = num_splits;
  g.split_tokens = decode_split_tokens(max_context, num_splits);
  g.ws_o = (float*)workspace;
  g.ws_ml = g.ws_o ? g.ws_o + (long)B * hq * num_splits * hd : nullptr;
  return true;
}

// dli_decode_attention over an FP8 cache (attention_decode_fp8.hip), arguments checked
int decode_attention_fp8_launch(void* out, const void* q, int q_stride, const void* k_cache,
                                const void* v_cache, const int* block_tables, int max_blocks,
                                const int* context_lens, int B, int hq, int hkv, int hd,
                                int block_size, float scale, const DecodeSplits& g,
                                float k_scale, float v_scale, hipStream_t st);
