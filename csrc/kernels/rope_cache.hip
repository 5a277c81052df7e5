// RoPE (rotate-half, HF Llama convention) applied IN PLACE to q and k inside the fused QKV
// activation, fused with the paged KV-cache write: SURVEY.md §2.4 K5/K6. The work is
// qkv_rope_cache_body of qkv_rope.h on bf16 rows, with or without the QKV bias and the per-head
// q/k RMSNorm of the Qwen families, into a bf16 or an FP8 cache.
#include "qkv_rope.h"

__global__ void __launch_bounds__(256) rope_cache_kernel(
    u16* __restrict__ qkv, int row_stride, const int* __restrict__ positions,
    const int* __restrict__ slot_mapping, const float* __restrict__ cos_sin,
    u16* __restrict__ k_cache, u16* __restrict__ v_cache, int T, int hq, int hkv, int hd,
    int block_size, int use_rope) {
  qkv_rope_cache_body<QkvSrc::ROWS, 1, false>(
      qkv, row_stride, nullptr, 1, positions, slot_mapping, cos_sin, k_cache, v_cache, T, hq,
      hkv, hd, block_size, use_rope, nullptr, nullptr, nullptr, 0.f);
}

__global__ void __launch_bounds__(256) rope_cache_x_kernel(
    u16* __restrict__ qkv, int row_stride, const int* __restrict__ positions,
    const int* __restrict__ slot_mapping, const float* __restrict__ cos_sin,
    u16* __restrict__ k_cache, u16* __restrict__ v_cache, int T, int hq, int hkv, int hd,
    int block_size, int use_rope, const u16* __restrict__ bias,
    const u16* __restrict__ q_norm_w, const u16* __restrict__ k_norm_w, float qk_eps) {
  qkv_rope_cache_body<QkvSrc::ROWS, 1, true>(
      qkv, row_stride, nullptr, 1, positions, slot_mapping, cos_sin, k_cache, v_cache, T, hq,
      hkv, hd, block_size, use_rope, bias, q_norm_w, k_norm_w, qk_eps);
}

// The same rows into an FP8 (e4m3fn) cache: see store8_fp8 of common.h
template <bool X>
__global__ void __launch_bounds__(256) rope_cache_kv8_kernel(
    u16* __restrict__ qkv, int row_stride, const int* __restrict__ positions,
    const int* __restrict__ slot_mapping, const float* __restrict__ cos_sin,
    fp8* __restrict__ k_cache, fp8* __restrict__ v_cache, int T, int hq, int hkv, int hd,
    int block_size, int use_rope, const u16* __restrict__ bias,
    const u16* __restrict__ q_norm_w, const u16* __restrict__ k_norm_w, float qk_eps,
    float k_inv_scale, float v_inv_scale) {
  qkv_rope_cache_body<QkvSrc::ROWS, 1, X, fp8>(
      qkv, row_stride, nullptr, 1, positions, slot_mapping, cos_sin, k_cache, v_cache, T, hq,
      hkv, hd, block_size, use_rope, bias, q_norm_w, k_norm_w, qk_eps, k_inv_scale,
      v_inv_scale);
}

// bias / q_norm_w / k_norm_w: see qkv_extras_ok; all null on a bf16 cache = the plain kernel.
// kv_fp8: the caches [nblk, Hkv, bs, hd] hold one e4m3fn byte per element and k_inv_scale /
// v_inv_scale are 1 / their scales (fp32, computed once by the caller); else bf16 and 1.
extern "C" int dli_rope_cache(void* qkv, int row_stride, const int* positions,
                              const int* slot_mapping, const float* cos_sin, void* k_cache,
                              void* v_cache, int T, int hq, int hkv, int hd, int block_size,
                              int use_rope, const void* bias, const void* q_norm_w,
                              const void* k_norm_w, float qk_eps, int kv_fp8, float k_inv_scale,
                              float v_inv_scale, hipStream_t st) {
  if (T <= 0) return 0;
  if (hd % 16 != 0 || !kv_scales_ok(kv_fp8, k_inv_scale, v_inv_scale) ||
      !qkv_extras_ok(bias, q_norm_w, k_norm_w, hd))
    return (int)hipErrorInvalidValue;
  const long total = (long)T * (hq + 2 * hkv) * (hd / 16);
  const int blocks = (int)((total + 255) / 256);
  const bool extras = bias != nullptr || q_norm_w != nullptr || k_norm_w != nullptr;
#define DLI_RC(KERNEL, KV, ...)                                                              \
  KERNEL<<<blocks, 256, 0, st>>>((u16*)qkv, row_stride, positions, slot_mapping, cos_sin,    \
                                 (KV*)k_cache, (KV*)v_cache, T, hq, hkv, hd, block_size,     \
                                 use_rope, ##__VA_ARGS__)
#define DLI_RC_X (const u16*)bias, (const u16*)q_norm_w, (const u16*)k_norm_w, qk_eps
  if (!kv_fp8 && !extras)
    DLI_RC(rope_cache_kernel, u16);
  else if (!kv_fp8)
    DLI_RC(rope_cache_x_kernel, u16, DLI_RC_X);
  else if (!extras)
    DLI_RC(rope_cache_kv8_kernel<false>, fp8, DLI_RC_X, k_inv_scale, v_inv_scale);
  else
    DLI_RC(rope_cache_kv8_kernel<true>, fp8, DLI_RC_X, k_inv_scale, v_inv_scale);
#undef DLI_RC_X
#undef DLI_RC
  DLI_RETURN_LAUNCH();
}
