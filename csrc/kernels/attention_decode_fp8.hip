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
// The tile loop and the Q^T fragment load are the bf16 kernel's (attention_decode.h,
// decode_attn_loop<HD, fp8> and load_q_frags<HD, true>: the K row chunks and their k order,
// the V staging).
//
// Not built for FP8: the fused QKV prologue, the workgroup-per-item and the pipelined forms.
#include "attention_decode.h"

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
  load_q_frags<HD, true>(q, q_stride, b, kvh, G, lane, qf);
  const int bt_lane0 =
      decode_bt_window(block_tables, max_blocks, b, s_begin, s_end, block_size, lane);
  f32x4 o_acc[HD / 16];
  float m_run, l_part;
  decode_attn_loop<HD>(qf, vt, lane, b, kvh, s_begin, s_end, k_cache, v_cache, block_tables,
                       max_blocks, hkv, block_size, scale_log2, bt_lane0, o_acc, m_run, l_part);
  decode_finalize<HD>(o_acc, m_run, l_part * inv_v_scale, lane, b, kvh, split, G, hq,
                      num_splits, out, ws_o, ws_ml);
}

int decode_attention_fp8_launch(void* out, const void* q, int q_stride, const void* k_cache,
                                const void* v_cache, const int* block_tables, int max_blocks,
                                const int* context_lens, int B, int hq, int hkv, int hd,
                                int block_size, float scale, const DecodeSplits& g,
                                float k_scale, float v_scale, hipStream_t st) {
  const float scale_log2 = scale * 1.4426950408889634f * k_scale;
  const float inv_v_scale = 1.f / v_scale;
  const long items = (long)B * hkv * g.num_splits;
  dim3 grid((int)((items + DEC_WAVES - 1) / DEC_WAVES));
  if (hd == 128)
    decode_attn_kv8_kernel<128, 4><<<grid, 64 * DEC_WAVES, 0, st>>>(
        (u16*)out, (const u16*)q, q_stride, (const fp8*)k_cache, (const fp8*)v_cache,
        block_tables, max_blocks, context_lens, B, hq, hkv, block_size, scale_log2,
        g.num_splits, g.split_tokens, g.ws_o, g.ws_ml, g.window, inv_v_scale);
  else
    decode_attn_kv8_kernel<64, 1><<<grid, 64 * DEC_WAVES, 0, st>>>(
        (u16*)out, (const u16*)q, q_stride, (const fp8*)k_cache, (const fp8*)v_cache,
        block_tables, max_blocks, context_lens, B, hq, hkv, block_size, scale_log2,
        g.num_splits, g.split_tokens, g.ws_o, g.ws_ml, g.window, inv_v_scale);
  if (g.num_splits > 1)
    return decode_reduce_launch(out, g.ws_o, g.ws_ml, B, hq, hd, g.num_splits, st);
  DLI_RETURN_LAUNCH();
}
