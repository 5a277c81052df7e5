// What the paged decode attention kernels share (attention_decode.hip: bf16 cache;
// attention_decode_fp8.hip: FP8 cache): the block-table window, the sliding-window bound, the
// Q^T fragment load, the S^T MFMAs, the online-softmax update and the finalize step. See the
// note at the top of attention_decode.hip for the work decomposition and the layouts.
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

// Q^T fragments (B operand) of item (b, kvh) from bf16 rows: head = col, dims 32kk + 8grp .. +7
template <int HD>
__device__ __forceinline__ void load_q_frags(const u16* __restrict__ q, int q_stride, int b,
                                             int kvh, int G, int lane, bf16x8 (&qf)[HD / 32]) {
  const int col = lane & 15, grp = lane >> 4;
  const bool valid = col < G;
  const u16* qp = q + (long)b * q_stride + (long)(kvh * G + (valid ? col : 0)) * HD;
#pragma unroll
  for (int kk = 0; kk < HD / 32; ++kk) {
    uint4 v = valid ? *reinterpret_cast<const uint4*>(qp + kk * 32 + grp * 8)
                    : make_uint4(0, 0, 0, 0);
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
