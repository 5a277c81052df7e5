// 4-bit group-scaled weights (AWQ-style "W4A16"; ops/reference.py pack_w4 / dequantize_weight_w4):
// q_packed [N, K / 2] bytes of nibbles q in 0..15 and sz [N, K / 128] words (fp16 scale bits |
// zero point << 16), W[n, k] = (q[n, k] - z[n][k >> 7]) * s[n][k >> 7]; activations, sums and
// outputs as the bf16 path:
//  * dli_gemv_w4 / dli_gemv_fused_w4: the M <= 4 weight stream of gemv.h reading half a byte
//    per weight (dli_gemm's GEMV tiles and dli_gemv_fused with the sz words as one more operand);
//  * dli_dequant_w4: q_packed, sz -> the bf16 weight, for every GEMM the stream does not cover
//    (ops.W4Weight.bf16: dequantise into the scratch, then the bf16 GEMM).
#include "gemv.h"

// The lane load is 8 B, a chunk of 16 K-elements (gemv.h WInt4<4>; ops/gemm.py W4_CHUNK): the
// FP8 stream's chunk geometry. Against the 16-B load (WInt4<5>) on the Llama-3-8B projections
// it was as fast or faster on QKV, O and gate/up at M = 1 and 4 and 9-12 % slower on down, and
// it keeps every instantiation but one at 2 or more waves per SIMD where the 16-B load left
// the 32-row tiles at one (profiles/w4_weights/README.md).
typedef WInt4<4> W4;

// sz: [N, sld] words. The epilogues of dli_gemv_fp8.
extern "C" int dli_gemv_w4(const void* A, int lda, const void* Wq, const void* sz, int sld,
                           int ldw, void* C, int ldc, int M, int N, int K, int epi, int tile_cfg,
                           int splits, const void* bias, void* ws, hipStream_t st) {
  if (M <= 0 || N <= 0) return 0;
  if ((tile_cfg < 29 || tile_cfg > 33) && (tile_cfg < 56 || tile_cfg > 59))
    return (int)hipErrorInvalidValue;
  if (lda % 8 || splits < 1 || (epi == EPI_SILU && N % 32) || (splits > 1 && ws == nullptr))
    return (int)hipErrorInvalidValue;
  const W4 W{(const uint8_t*)Wq, (const uint32_t*)sz, sld};
  switch (epi) {
    case EPI_BF16: return dispatch_gemv<EPI_BF16>(tile_cfg, A, lda, W, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_F32: return dispatch_gemv<EPI_F32>(tile_cfg, A, lda, W, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_SILU: return dispatch_gemv<EPI_SILU>(tile_cfg, A, lda, W, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_BIAS: return dispatch_gemv<EPI_BIAS>(tile_cfg, A, lda, W, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    default: return (int)hipErrorInvalidValue;
  }
}

extern "C" int dli_gemv_fused_w4(const void* A, int lda, const void* nw, float eps,
                                 const void* Wq, const void* sz, int sld, int ldw, void* C,
                                 int ldc, int M, int N, int K, int epi, int tile_cfg, int splits,
                                 void* ws, hipStream_t st) {
  return gemv_fused(A, lda, nw, eps, W4{(const uint8_t*)Wq, (const uint32_t*)sz, sld}, ldw, C,
                    ldc, M, N, K, epi, tile_cfg, splits, ws, st);
}

// out[n, k] = bf16((q[n, k] - z) * s): the fp32 product (exact: 5 x 11 bits) rounded once. A
// thread takes 32 consecutive K-elements of one row (one 16-B load, one sz word, four 16-B
// stores); they lie in one 128-group.
__global__ void __launch_bounds__(256) dequant_w4_kernel(
    u16* __restrict__ out, const uint8_t* __restrict__ q, const uint32_t* __restrict__ sz, int N,
    int K) {
  const int chunks = K >> 5;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)N * chunks) return;
  const int n = (int)(gid / chunks), c = (int)(gid % chunks);
  const uint32_t zs = sz[(long)n * (K >> 7) + (c >> 2)];
  const float sc = (float)__builtin_bit_cast(_Float16, (uint16_t)(zs & 0xFFFFu));
  const float z = (float)((zs >> 16) & 15u);
  const uint4 v = *reinterpret_cast<const uint4*>(q + (((long)n * K) >> 1) + c * 16);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  u16* o = out + (long)n * K + c * 32;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float f[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = ((float)((w[j] >> (4 * i)) & 15u) - z) * sc;
      f[2 * i + 1] = ((float)((w[j] >> (4 * i + 16)) & 15u) - z) * sc;
    }
    store8(o + 8 * j, f);
  }
}

// q_packed [N, K / 2] bytes and out [N, K] bf16, both contiguous and 16-B aligned;
// sz [N, K / 128] words contiguous; K in whole 128-groups
extern "C" int dli_dequant_w4(const void* q, const void* sz, void* out, int N, int K,
                              hipStream_t st) {
  if (N <= 0 || K <= 0) return 0;
  if (K % 128 || q == nullptr || sz == nullptr || out == nullptr ||
      ((uintptr_t)q | (uintptr_t)out) % 16)
    return (int)hipErrorInvalidValue;
  const long total = (long)N * (K / 32);
  dequant_w4_kernel<<<(int)((total + 255) / 256), 256, 0, st>>>(
      (u16*)out, (const uint8_t*)q, (const uint32_t*)sz, N, K);
  DLI_RETURN_LAUNCH();
}
