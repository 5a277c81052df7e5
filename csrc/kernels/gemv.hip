// Weight-streaming skinny GEMM for M <= 4 rows (tile ids 29-33, 56-59) and the batch-1
// reduce-free forms (dli_gemv_fused: residual-adding epilogue, RMSNorm prologue), bf16
// weights. The kernel, its launcher and the two dispatchers are in gemv.h (shared with the
// FP8-weight entry points of gemv_fp8.hip).
#include "gemv.h"

int gemm_gemv_dispatch(int epi, int tile_cfg, DLI_GEMM_ARGS) {
  if ((tile_cfg < 29 || tile_cfg > 33) && (tile_cfg < 56 || tile_cfg > 59)) return DLI_NOT_MINE;
  if (go != nullptr) return (int)hipErrorInvalidValue;     // no grouped mode
  (void)groups;
  switch (epi) {
    case EPI_BF16: return dispatch_gemv<EPI_BF16>(tile_cfg, A, lda, WBf16{(const u16*)W}, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_F32: return dispatch_gemv<EPI_F32>(tile_cfg, A, lda, WBf16{(const u16*)W}, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_SILU: return dispatch_gemv<EPI_SILU>(tile_cfg, A, lda, WBf16{(const u16*)W}, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_BIAS_GELU: return dispatch_gemv<EPI_BIAS_GELU>(tile_cfg, A, lda, WBf16{(const u16*)W}, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_BIAS: return dispatch_gemv<EPI_BIAS>(tile_cfg, A, lda, WBf16{(const u16*)W}, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    default: return (int)hipErrorInvalidValue;
  }
}

// dli_gemv_fused: see gemv.h gemv_fused
extern "C" int dli_gemv_fused(const void* A, int lda, const void* nw, float eps, const void* W,
                              int ldw, void* C, int ldc, int M, int N, int K, int epi,
                              int tile_cfg, int splits, void* ws, hipStream_t st) {
  return gemv_fused(A, lda, nw, eps, WBf16{(const u16*)W}, ldw, C, ldc, M, N, K, epi, tile_cfg,
                    splits, ws, st);
}
