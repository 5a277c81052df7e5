// FP8 block-scaled weights (ops/reference.py: q [N, K] e4m3fn, scales [N / 16, ceil(K / 128)]
// fp32, W[n, k] = q[n, k] * s[n >> 4][k >> 7]; activations, sums and outputs as the bf16 path):
//  * dli_gemv_fp8 / dli_gemv_fused_fp8: the M <= 4 weight stream of gemv.h reading one byte
//    per weight (dli_gemm's GEMV tiles and dli_gemv_fused with one more operand, the scales);
//  * dli_dequant_fp8_block: q, s -> the bf16 weight, for every GEMM the stream does not cover
//    (ops.Fp8Weight.bf16: dequantise into a scratch, then the bf16 GEMM).
#include "gemv.h"

// scales: [N / 16, sld] fp32. The epilogues of dli_gemm's GEMV tiles except bias + GELU
// (GPT-2 only, which has no FP8 form).
extern "C" int dli_gemv_fp8(const void* A, int lda, const void* Wq, const void* scales, int sld,
                            int ldw, void* C, int ldc, int M, int N, int K, int epi,
                            int tile_cfg, int splits, const void* bias, void* ws,
                            hipStream_t st) {
  if (M <= 0 || N <= 0) return 0;
  if ((tile_cfg < 29 || tile_cfg > 33) && (tile_cfg < 56 || tile_cfg > 59))
    return (int)hipErrorInvalidValue;
  if (lda % 8 || splits < 1 || (epi == EPI_SILU && N % 32) || (splits > 1 && ws == nullptr))
    return (int)hipErrorInvalidValue;
  const WFp8 W{(const fp8*)Wq, (const float*)scales, sld};
  switch (epi) {
    case EPI_BF16: return dispatch_gemv<EPI_BF16>(tile_cfg, A, lda, W, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_F32: return dispatch_gemv<EPI_F32>(tile_cfg, A, lda, W, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_SILU: return dispatch_gemv<EPI_SILU>(tile_cfg, A, lda, W, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_BIAS: return dispatch_gemv<EPI_BIAS>(tile_cfg, A, lda, W, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    default: return (int)hipErrorInvalidValue;
  }
}

extern "C" int dli_gemv_fused_fp8(const void* A, int lda, const void* nw, float eps,
                                  const void* Wq, const void* scales, int sld, int ldw, void* C,
                                  int ldc, int M, int N, int K, int epi, int tile_cfg,
                                  int splits, void* ws, hipStream_t st) {
  return gemv_fused(A, lda, nw, eps, WFp8{(const fp8*)Wq, (const float*)scales, sld}, ldw, C,
                    ldc, M, N, K, epi, tile_cfg, splits, ws, st);
}

// out[n, k] = bf16(float(q[n, k]) * s[n >> 4][k >> 7]): the fp32 product rounded once. A thread
// takes 16 consecutive K-elements of one row (one 16-B load, two 16-B stores); they lie in
// one 128-column block.
__global__ void __launch_bounds__(256) dequant_fp8_block_kernel(
    u16* __restrict__ out, const fp8* __restrict__ q, const float* __restrict__ s, int N, int K,
    int sld) {
  const int chunks = K >> 4;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)N * chunks) return;
  const int n = (int)(gid / chunks), c = (int)(gid % chunks);
  const float sc = s[(long)(n >> 4) * sld + (c >> 3)];
  uint4 lo, hi;
  fp8x16_to_bf16(*reinterpret_cast<const uint4*>(q + (long)n * K + c * 16), lo, hi);
  float f[16];
  unpack8bf(lo, f);
  unpack8bf(hi, f + 8);
#pragma unroll
  for (int j = 0; j < 16; ++j) f[j] *= sc;
  u16* o = out + (long)n * K + c * 16;
  store8(o, f);
  store8(o + 8, f + 8);
}

// any K: one element per thread
__global__ void __launch_bounds__(256) dequant_fp8_block_scalar_kernel(
    u16* __restrict__ out, const fp8* __restrict__ q, const float* __restrict__ s, int N, int K,
    int sld) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)N * K) return;
  const int n = (int)(gid / K), k = (int)(gid % K);
  const float v = __uint_as_float(fp8x2_to_bf16x2<false>((uint32_t)q[gid]) << 16);
  out[gid] = f2bf(v * s[(long)(n >> 4) * sld + (k >> 7)]);
}

// q [N, K] e4m3fn and out [N, K] bf16, both contiguous; s [N / 16, ceil(K / 128)] fp32
// contiguous
extern "C" int dli_dequant_fp8_block(const void* q, const void* s, void* out, int N, int K,
                                     hipStream_t st) {
  if (N <= 0 || K <= 0) return 0;
  if (N % 16 || q == nullptr || s == nullptr || out == nullptr)
    return (int)hipErrorInvalidValue;
  const int sld = (K + 127) / 128;
  const bool vec = K % 16 == 0 && ((uintptr_t)q | (uintptr_t)out) % 16 == 0;
  if (vec) {
    const long total = (long)N * (K / 16);
    dequant_fp8_block_kernel<<<(int)((total + 255) / 256), 256, 0, st>>>(
        (u16*)out, (const fp8*)q, (const float*)s, N, K, sld);
  } else {
    const long total = (long)N * K;
    dequant_fp8_block_scalar_kernel<<<(int)((total + 255) / 256), 256, 0, st>>>(
        (u16*)out, (const fp8*)q, (const float*)s, N, K, sld);
  }
  DLI_RETURN_LAUNCH();
}
