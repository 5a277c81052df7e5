// RoPE (rotate-half, HF Llama convention) applied IN PLACE to q and k inside the fused QKV
// activation, fused with the paged KV-cache write: SURVEY.md §2.4 K5/K6. The work is
// qkv_rope_cache_body of qkv_rope.h on bf16 rows; dli_rope_cache_x adds the QKV bias and the
// per-head q/k RMSNorm of the Qwen families.
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

// bias / q_norm_w / k_norm_w: see qkv_extras_ok; all null = dli_rope_cache
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
  if (!qkv_extras_ok(bias, q_norm_w, k_norm_w, hd)) return (int)hipErrorInvalidValue;
  rope_cache_x_kernel<<<blocks, 256, 0, st>>>(
      (u16*)qkv, row_stride, positions, slot_mapping, cos_sin, (u16*)k_cache, (u16*)v_cache, T,
      hq, hkv, hd, block_size, use_rope, (const u16*)bias, (const u16*)q_norm_w,
      (const u16*)k_norm_w, qk_eps);
  DLI_RETURN_LAUNCH();
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

// dli_rope_cache_x with an FP8 cache [nblk, Hkv, bs, hd] of one byte per element;
// k_inv_scale / v_inv_scale: 1 / the cache's scales (fp32, computed once by the caller)
extern "C" int dli_rope_cache_kv8(void* qkv, int row_stride, const int* positions,
                                  const int* slot_mapping, const float* cos_sin, void* k_cache,
                                  void* v_cache, int T, int hq, int hkv, int hd, int block_size,
                                  int use_rope, const void* bias, const void* q_norm_w,
                                  const void* k_norm_w, float qk_eps, float k_inv_scale,
                                  float v_inv_scale, hipStream_t st) {
  if (T <= 0) return 0;
  if (hd % 16 != 0 || !(k_inv_scale > 0.f) || !(v_inv_scale > 0.f))
    return (int)hipErrorInvalidValue;
  if (!qkv_extras_ok(bias, q_norm_w, k_norm_w, hd)) return (int)hipErrorInvalidValue;
  const long total = (long)T * (hq + 2 * hkv) * (hd / 16);
  const int blocks = (int)((total + 255) / 256);
  if (bias == nullptr && q_norm_w == nullptr && k_norm_w == nullptr)
    rope_cache_kv8_kernel<false><<<blocks, 256, 0, st>>>(
        (u16*)qkv, row_stride, positions, slot_mapping, cos_sin, (fp8*)k_cache, (fp8*)v_cache,
        T, hq, hkv, hd, block_size, use_rope, nullptr, nullptr, nullptr, 0.f, k_inv_scale,
        v_inv_scale);
  else
    rope_cache_kv8_kernel<true><<<blocks, 256, 0, st>>>(
        (u16*)qkv, row_stride, positions, slot_mapping, cos_sin, (fp8*)k_cache, (fp8*)v_cache,
        T, hq, hkv, hd, block_size, use_rope, (const u16*)bias, (const u16*)q_norm_w,
        (const u16*)k_norm_w, qk_eps, k_inv_scale, v_inv_scale);
  DLI_RETURN_LAUNCH();
}

extern "C" int dli_rope_cache(void* qkv, int row_stride, const int* positions,
                              const int* slot_mapping, const float* cos_sin, void* k_cache,
                              void* v_cache, int T, int hq, int hkv, int hd, int block_size,
                              int use_rope, hipStream_t st) {
  return dli_rope_cache_x(qkv, row_stride, positions, slot_mapping, cos_sin, k_cache, v_cache, T,
                          hq, hkv, hd, block_size, use_rope, nullptr, nullptr, nullptr, 0.f, st);
}
