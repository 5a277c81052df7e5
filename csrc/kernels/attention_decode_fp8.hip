// Paged decode attention over an FP8 (OCP e4m3fn) KV cache: decode_attn_kernel of
// attention_decode.hip (one wave per (sequence, kv head, KV split) item, 32-token tiles, head
// dim 64 / 128, sliding window, block-table windows of 64 blocks) reading half the bytes.
//
// Cache: k_cache and v_cache [nblk, Hkv, bs, hd], one byte per element, value = byte * scale
// with one fp32 scale per cache (common.h, ops/reference.py quantize_kv). K and V are
// dequantised to bf16 in registers (exact: every e4m3fn value is a bf16 value) and the
// products stay mfma_f32_16x16x32_bf16; Q and P are bf16 as in the bf16 kernel. Neither scale
// costs a multiply per element: k_scale is folded into the score scale, v_scale into the
// final 1 / l (the denominator handed to decode_finalize is l / v_scale, in every split
// alike, so the merge of the splits' (m, l, O) is unchanged).
//
// K rows: a row of hd bytes is hd / 16 chunks of 16 B; the 4 lanes of token `col` load chunks
// grp, grp + 4 (one 16-B load each), so lane (col, grp) holds dims 64j + 16grp .. +15 and
// feeds k-step kk = 2j + h with dims 64j + 16grp + 8h .. +7. The MFMA sums over k whatever
// the order, so the Q^T fragment takes the same dims (load_q_frags_kv8) and nothing is
// shuffled. V rows: 16-B loads, dequantised on their way into the per-wave LDS tile, whose
// bf16 image and transposing reads (ds_read_b64_tr_b16) are the bf16 kernel's.
//
// Not built for FP8: the fused QKV prologue, the workgroup-per-item and the pipelined forms.
#include "attention_decode.h"

// Q^T fragments (B operand) in the k order of the FP8 K rows: head = col, k-step kk holds
// dims 64(kk >> 1) + 16grp + 8(kk & 1) .. +7
template <int HD>
__device__ __forceinline__ void load_q_frags_kv8(const u16* __restrict__ q, int q_stride, int b,
                                                 int kvh, int G, int lane,
                                                 bf16x8 (&qf)[HD / 32]) {
  const int col = lane & 15, grp = lane >> 4;
  const bool valid = col < G;
  const u16* qp = q + (long)b * q_stride + (long)(kvh * G + (valid ? col : 0)) * HD;
#pragma unroll
  for (int kk = 0; kk < HD / 32; ++kk) {
    uint4 v = valid ? *reinterpret_cast<const uint4*>(qp + 64 * (kk >> 1) + 16 * grp +
                                                      8 * (kk & 1))
                    : make_uint4(0, 0, 0, 0);
    qf[kk] = *reinterpret_cast<bf16x8*>(&v);
  }
}

// decode_attn_loop of attention_decode.hip over FP8 rows: tokens [s_begin, s_end) of one item
template <int HD>
__device__ __forceinline__ void decode_attn_loop_kv8(
    const bf16x8 (&qf)[HD / 32], u16* vt, int lane, int b, int kvh, int s_begin, int s_end,
    const fp8* __restrict__ k_cache, const fp8* __restrict__ v_cache,
    const int* __restrict__ block_tables, int max_blocks, int hkv, int block_size,
    float scale_log2, int bt_lane0, f32x4 (&o_acc)[HD / 16], float& m_run, float& l_part) {
  constexpr int DB = HD / 16;     // 16-wide output column blocks
  constexpr int KK = HD / 32;     // MFMA k-steps over head_dim
  constexpr int KC = HD / 64;     // 16-B chunks of a K row per lane
  constexpr int VROW = HD + 16;   // padded LDS row of the (bf16) V tile, in u16
  constexpr int VCH = HD / 16;    // 16-B chunks per FP8 V row
  constexpr int VP = DEC_TILE * VCH / 64;   // V chunks per lane per tile
  const int col = lane & 15, grp = lane >> 4;
  const int* bt = block_tables + (long)b * max_blocks;
  const int last_blk = max(s_end - 1, 0) / block_size;
  int win = s_begin / block_size;
  int bt_lane = bt_lane0;
  const long kv_head_stride = (long)block_size * HD;           // bytes per (blk, head)
  m_run = -INFINITY;
  l_part = 0.f;
#pragma unroll
  for (int i = 0; i < DB; ++i) o_acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t0 = s_begin; t0 < s_end; t0 += DEC_TILE) {
    if ((min(t0 + DEC_TILE, s_end) - 1) / block_size - win >= 64) {   // wave-uniform
      win = t0 / block_size;
      bt_lane = bt[min(win + lane, last_blk)];
    }
    // ---- every global load of the tile up front
    uint4 k8[2][KC];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      int tok = t0 + 16 * s + col;
      tok = tok < s_end ? tok : s_end - 1;                     // clamp: always-written rows
      const int blk = __shfl(bt_lane, tok / block_size - win, 64), off = tok % block_size;
      const fp8* kp = k_cache + ((long)blk * hkv + kvh) * kv_head_stride + (long)off * HD;
#pragma unroll
      for (int j = 0; j < KC; ++j)
        k8[s][j] = *reinterpret_cast<const uint4*>(kp + 64 * j + 16 * grp);
    }
    // V rows t0 .. t0+31 (row-major, 16-B chunks; piece lane + 64m = row r, chunk c)
    uint4 v8[VP];
#pragma unroll
    for (int m = 0; m < VP; ++m) {
      const int piece = lane + 64 * m, r = piece / VCH, c = piece % VCH;
      const int tok = min(t0 + r, s_end - 1);                  // clamp: always-written rows
      const int blk = __shfl(bt_lane, tok / block_size - win, 64), off = tok % block_size;
      v8[m] = *reinterpret_cast<const uint4*>(
          v_cache + ((long)blk * hkv + kvh) * kv_head_stride + (long)off * HD + c * 16);
    }
    uint4 kreg[2][KK];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < KC; ++j) fp8x16_to_bf16(k8[s][j], kreg[s][2 * j], kreg[s][2 * j + 1]);
    f32x4 s_acc[2];
    decode_scores<HD>(kreg, qf, s_acc);
    float p[8];
    decode_softmax_update<HD, false>(s_acc, t0, s_end, grp, scale_log2, m_run, l_part, o_acc, p);
    // stage the V tile as bf16 in this wave's LDS rows (previous tile's reads retired below)
#pragma unroll
    for (int m = 0; m < VP; ++m) {
      const int piece = lane + 64 * m, r = piece / VCH, c = piece % VCH;
      uint4 lo, hi;
      fp8x16_to_bf16(v8[m], lo, hi);
      *reinterpret_cast<uint4*>(vt + r * VROW + c * 16) = lo;
      *reinterpret_cast<uint4*>(vt + r * VROW + c * 16 + 8) = hi;
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

// scale_log2 carries k_scale; inv_v_scale = 1 / v_scale
template <int HD, int MINW>
__global__ void __launch_bounds__(256, MINW) decode_attn_kv8_kernel(
    u16* __restrict__ out, const u16* __restrict__ q, int q_stride,
    const fp8* __restrict__ k_cache, const fp8* __restrict__ v_cache,
    const int* __restrict__ block_tables, int max_blocks, const int* __restrict__ context_lens,
    int B, int hq, int hkv, int block_size, float scale_log2, int num_splits, int split_tokens,
    float* __restrict__ ws_o, float* __restrict__ ws_ml, int window, float inv_v_scale) {
  constexpr int KK = HD / 32;
  constexpr int VROW = HD + 16;
  __shared__ __attribute__((aligned(16))) u16 vtile_all[DEC_WAVES][DEC_TILE * VROW];
  u16* vt = vtile_all[threadIdx.x >> 6];
  const int lane = threadIdx.x & 63;
  const int item = blockIdx.x * DEC_WAVES + (threadIdx.x >> 6);
  if (item >= B * hkv * num_splits) return;                    // wave-uniform exit
  const int split = item % num_splits;
  const int bh = item / num_splits;
  const int kvh = bh % hkv, b = bh / hkv;
  const int G = hq / hkv;
  const int ctx = context_lens[b];
  const int s_begin = decode_win_lo(ctx, window) + split * split_tokens;
  const int s_end = min(ctx, s_begin + split_tokens);
  bf16x8 qf[KK];
  load_q_frags_kv8<HD>(q, q_stride, b, kvh, G, lane, qf);
  const int bt_lane0 =
      decode_bt_window(block_tables, max_blocks, b, s_begin, s_end, block_size, lane);
  f32x4 o_acc[HD / 16];
  float m_run, l_part;
  decode_attn_loop_kv8<HD>(qf, vt, lane, b, kvh, s_begin, s_end, k_cache, v_cache, block_tables,
                           max_blocks, hkv, block_size, scale_log2, bt_lane0, o_acc, m_run,
                           l_part);
  decode_finalize<HD>(o_acc, m_run, l_part * inv_v_scale, lane, b, kvh, split, G, hq,
                      num_splits, out, ws_o, ws_ml);
}

// dli_decode_attention_win over an FP8 cache with the scales k_scale, v_scale (> 0)
extern "C" int dli_decode_attention_kv8(void* out, const void* q, int q_stride,
                                        const void* k_cache, const void* v_cache,
                                        const int* block_tables, int max_blocks,
                                        const int* context_lens, int B, int hq, int hkv, int hd,
                                        int block_size, float scale, int max_context,
                                        int num_splits, void* workspace, int window,
                                        float k_scale, float v_scale, hipStream_t st) {
  if (B <= 0) return 0;
  if (window < 0) window = 0;
  if (window > 0 && window < max_context) max_context = window;
  if (hq % hkv || hq / hkv > 16 || block_size % 16 || (hd != 64 && hd != 128))
    return (int)hipErrorInvalidValue;
  if (!(k_scale > 0.f) || !(v_scale > 0.f)) return (int)hipErrorInvalidValue;
  if (num_splits < 1) num_splits = 1;
  if (num_splits > 1 && workspace == nullptr) return (int)hipErrorInvalidValue;
  int split_tokens = (max_context + num_splits - 1) / num_splits;
  split_tokens = ((split_tokens + DEC_TILE - 1) / DEC_TILE) * DEC_TILE;
  if (split_tokens <= 0) split_tokens = DEC_TILE;
  float* ws_o = (float*)workspace;
  float* ws_ml = ws_o ? ws_o + (long)B * hq * num_splits * hd : nullptr;
  const float scale_log2 = scale * 1.4426950408889634f * k_scale;
  const float inv_v_scale = 1.f / v_scale;
  const long items = (long)B * hkv * num_splits;
  dim3 grid((int)((items + DEC_WAVES - 1) / DEC_WAVES));
  if (hd == 128)
    decode_attn_kv8_kernel<128, 4><<<grid, 64 * DEC_WAVES, 0, st>>>(
        (u16*)out, (const u16*)q, q_stride, (const fp8*)k_cache, (const fp8*)v_cache,
        block_tables, max_blocks, context_lens, B, hq, hkv, block_size, scale_log2, num_splits,
        split_tokens, ws_o, ws_ml, window, inv_v_scale);
  else
    decode_attn_kv8_kernel<64, 1><<<grid, 64 * DEC_WAVES, 0, st>>>(
        (u16*)out, (const u16*)q, q_stride, (const fp8*)k_cache, (const fp8*)v_cache,
        block_tables, max_blocks, context_lens, B, hq, hkv, block_size, scale_log2, num_splits,
        split_tokens, ws_o, ws_ml, window, inv_v_scale);
  if (num_splits > 1) return decode_reduce_launch(out, ws_o, ws_ml, B, hq, hd, num_splits, st);
  DLI_RETURN_LAUNCH();
}
