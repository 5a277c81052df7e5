// FP8 block-scaled weights at decode batches 5..64 (tile ids 70 / 71, dli_gemm_fp8_stream):
// C[M, N] = A[M, K] . W[N, K]^T with A bf16, M <= 64, and W an ops.Fp8Weight (q [N, K] e4m3fn
// bytes, scales [N / 16, ceil(K / 128)] fp32, W[n, k] = q[n, k] * s[n >> 4][k >> 7]). The
// weights are streamed once from HBM as bytes, converted in registers and fed to the MFMAs:
// no bf16 image is written (ops.Fp8Weight.bf16 + dli_gemm, the path of every other M > 4).
//
// A workgroup is 4 waves; a wave owns RG 16-row scale groups of W (tile 70: RG 1, 64 weight
// rows a workgroup; tile 71: RG 2, 128 rows) over the workgroup's K slice, which it walks in
// 128-column scale blocks. Per block and group, lane (fr = lane & 15, fq = lane >> 4) loads
// q[n0 + fr][k0 + 64 h2 + 16 fq .. +16) for the two 64-wide steps h2 as 16-B nontemporal loads
// (guide row 'nt-weights', as gemv.h), DEPTH blocks ahead of their use (a register ring, so
// the stream is not latency-bound). The 16 bytes become two 8 x bf16 fragments
// (fp8x16_to_bf16, exact): MFMA operand A of two v_mfma_f32_16x16x32_bf16, whose operand B is
// x[16 i + fr][k0 + 64 h2 + 16 fq + 8 h .. +8), the same K indices (the K order inside a step
// is a permutation of the sum). Transposed accumulators (gemm_common.h): the lane ends up with
// C[16 i + fr][n0 + 4 fq .. +4), so the quad stores and split-K reduce of the bf16 families
// apply. The scale never meets a convert instruction: the MFMAs of one block start from zero
// and acc += s * block_sum in fp32 (one scale per group and block is wave-uniform).
//
// x (at most 64 x K bf16, L2-resident) is shared by the four waves through LDS: the block's
// x tile [16 MB rows][128] travels with the weights (requested DEPTH blocks ahead by the whole
// workgroup, one 16-B vector per thread and 16 rows), is written to one of two LDS buffers
// when its block comes up, and read from there as B fragments by every wave and group: L2
// bytes read per HBM weight byte are 2 M / R (R = 64 RG weight rows a workgroup). One
// barrier per block: block t writes buffer t & 1, synchronises, reads it; the write of block
// t + 2 comes after the barrier of block t + 1, which every wave reaches after its reads of t.
//
// Tails: rows >= M and groups >= N / 16 are clamped on load and masked on store; chunks past
// the K slice are clamped on load and their weight bytes zeroed (fp8 +0) before the MFMA; no
// lane reads past the scale tensor (group and block clamped). The launcher refuses what the
// kernel cannot take: K or ldw not in whole 16-byte chunks, unaligned operands, a split whose
// slices do not start on a multiple of 128.
//
// dli_gemm_fp8_stream_grouped is the same loop (fp8_stream_tile) for an ops.Fp8Experts stack
// (q [E, N, K], scales [E, N / 16, ceil(K / 128)]) over the permuted rows of a MoE layer, on the
// compact grid of the align step's tile list: see gemm_fp8_stream_grouped_kernel.
#include "gemm_common.h"

typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));

// One workgroup's tile: the 16 MB rows xrow(0 .. M) against the weight rows of column block cb,
// over K slice ks of nks; outputs to rows crow0 + r of C. Shared by the dense grid (the rows of
// A, crow0 0) and the grouped one (an item of an expert's rows, gemm_fp8_stream_grouped_kernel).
template <int MB, int RG, int EPI, int DEPTH, class XRow>
__device__ __forceinline__ void fp8_stream_tile(
    XRow xrow, const fp8* __restrict__ Wq, int ldw, const float* __restrict__ S, int sld,
    void* __restrict__ C, int ldc, int crow0, int M, int N, int K, int k_split_len, int cb, int ks,
    int nks, const u16* __restrict__ bias, float* __restrict__ ws) {
  static_assert(DEPTH % 2 == 0, "block t uses LDS buffer t & 1 = u & 1");
  static_assert(EPI != EPI_SILU || RG <= 2, "a gate/up pair is two groups");
  constexpr int ROWS = 16 * MB;
  constexpr int RS = 17;                        // 16-B vectors per LDS row: 16 + 1 of padding
  __shared__ u32x4s xs[2][ROWS * RS];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int kb = ks * k_split_len;
  const int klen = min(k_split_len, K - kb);
  const int nchunk = klen >> 4;                 // 16-element weight chunks of the slice
  const int nx = klen >> 3;                     // 8-element x vectors of the slice
  const int nblk = (klen + 127) >> 7;           // scale blocks (the last may be partial)
  const int ngrp = N >> 4;
  const int g0 = (cb * 4 + wid) * RG;           // the wave's first scale group
  const u32x4s* wrow[RG];
  const float* srow[RG];
#pragma unroll
  for (int g = 0; g < RG; ++g) {
    const int grp = min(g0 + g, ngrp - 1);
    wrow[g] = reinterpret_cast<const u32x4s*>(Wq + (long)(grp * 16 + fr) * ldw + kb);
    srow[g] = S + (long)grp * sld + (kb >> 7);
  }
  // the x tile of a block: thread t takes vector t & 15 of rows (t >> 4) + 16 j
  const int xr = threadIdx.x >> 4, xc = threadIdx.x & 15;
  const u32x4s* xsrc[MB];
#pragma unroll
  for (int j = 0; j < MB; ++j)
    xsrc[j] = reinterpret_cast<const u32x4s*>(xrow(min(xr + 16 * j, M - 1)) + kb);

  u32x4s w[DEPTH][RG][2];
  float sc[DEPTH][RG];
  u32x4s xg[DEPTH][MB];
  // request block T into ring stage U (indices clamped into the slice)
#define DLI_F8S_ISSUE(U, T)                                                             \
  {                                                                                     \
    const int t_ = (T);                                                                 \
    _Pragma("unroll") for (int g = 0; g < RG; ++g) {                                    \
      _Pragma("unroll") for (int h2 = 0; h2 < 2; ++h2)                                  \
          w[U][g][h2] =                                                                 \
          __builtin_nontemporal_load(wrow[g] + min(t_ * 8 + 4 * h2 + fq, nchunk - 1));  \
      sc[U][g] = srow[g][min(t_, nblk - 1)];                                            \
    }                                                                                   \
    _Pragma("unroll") for (int j = 0; j < MB; ++j)                                      \
        xg[U][j] = xsrc[j][min(t_ * 16 + xc, nx - 1)];                                  \
  }
#pragma unroll
  for (int u = 0; u < DEPTH; ++u) {
    DLI_F8S_ISSUE(u, u)
    // oldest block first, as the loop refills them: the compiler requested the first blocks
    // in reverse, and the wait for block 0 that fits both orders (vmcnt(2)) drained the ring
    // on every trip
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  }

  f32x4 acc[MB][RG];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int g = 0; g < RG; ++g) acc[i][g] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int b = 0; b < nblk; b += DEPTH) {       // blocks past nblk: zero weights, no effect
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      const int t = b + u;
      u32x4s* buf = xs[u & 1];
#pragma unroll
      for (int j = 0; j < MB; ++j) buf[(xr + 16 * j) * RS + xc] = xg[u][j];
      lgkmcnt0();
      raw_barrier();
      f32x4 raw[MB][RG];
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int g = 0; g < RG; ++g) raw[i][g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const bool ok = t * 8 + 4 * h2 + fq < nchunk;
        bf16x8 wl[RG], wh[RG];
#pragma unroll
        for (int g = 0; g < RG; ++g) {
          const u32x4s v = w[u][g][h2];
          uint4 lo, hi;
          fp8x16_to_bf16(make_uint4(ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u),
                         lo, hi);
          wl[g] = __builtin_bit_cast(bf16x8, lo);
          wh[g] = __builtin_bit_cast(bf16x8, hi);
        }
#pragma unroll
        for (int i = 0; i < MB; ++i) {
          const u32x4s* xp = buf + (16 * i + fr) * RS + 8 * h2 + 2 * fq;
          const bf16x8 xa = __builtin_bit_cast(bf16x8, xp[0]);
          const bf16x8 xb = __builtin_bit_cast(bf16x8, xp[1]);
#pragma unroll
          for (int g = 0; g < RG; ++g) {
            raw[i][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[g], xa, raw[i][g], 0, 0, 0);
            raw[i][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[g], xb, raw[i][g], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int g = 0; g < RG; ++g) {
          acc[i][g] += sc[u][g] * raw[i][g];
          // the stage's scale is read before its refill is requested: with the load hoisted
          // above this sum the ring's registers were copied at the loop's end, each copy
          // behind a wait for its load (vmcnt(1) once per DEPTH blocks)
          asm volatile("" : "+v"(acc[i][g]) : : "memory");
        }
      DLI_F8S_ISSUE(u, t + DEPTH)
    }
  }
#undef DLI_F8S_ISSUE

  // epilogue: lane (fr, fq) holds C[16 i + fr][16 (g0 + g) + 4 fq .. +4)
  if (nks > 1) {                                // fp32 partial slab of this K slice (format 0)
    float* slab = ws + (long)ks * M * N;
#pragma unroll
    for (int i = 0; i < MB; ++i) {
      const int row = 16 * i + fr;
#pragma unroll
      for (int g = 0; g < RG; ++g)
        if (row < M && g0 + g < ngrp)
          slab_quad_fp32(slab + (long)row * N + 16 * (g0 + g) + 4 * fq, acc[i][g], 0, true, 4);
    }
    return;
  }
  const bool vec = out_vec<EPI>(C, ldc, N, bias);
  if constexpr (EPI == EPI_SILU) {
    // a 32-row pair is one gate group (even) and its up group (odd)
    if constexpr (RG == 2) {
#pragma unroll
      for (int i = 0; i < MB; ++i) {
        const int row = 16 * i + fr;
        if (row < M && g0 < ngrp)
          store_silu_quad(C, ldc, crow0 + row, (g0 >> 1) * 16 + 4 * fq, acc[i][0], acc[i][1], vec);
      }
    } else {
      // RG 1: wave 2 p holds the gate group, wave 2 p + 1 its up group, met through LDS
      __syncthreads();                          // every wave is done with the x buffers
      f32x4* ex = reinterpret_cast<f32x4*>(&xs[0][0]);   // [2 pairs][MB][64 lanes]
      if (wid & 1) {
#pragma unroll
        for (int i = 0; i < MB; ++i) ex[((wid >> 1) * MB + i) * 64 + lane] = acc[i][0];
      }
      __syncthreads();
      if (!(wid & 1)) {
#pragma unroll
        for (int i = 0; i < MB; ++i) {
          const int row = 16 * i + fr;
          const f32x4 up = ex[((wid >> 1) * MB + i) * 64 + lane];
          if (row < M && g0 < ngrp)
            store_silu_quad(C, ldc, crow0 + row, (g0 >> 1) * 16 + 4 * fq, acc[i][0], up, vec);
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < MB; ++i) {
    const int row = 16 * i + fr;
#pragma unroll
    for (int g = 0; g < RG; ++g)
      if (row < M && g0 + g < ngrp)
        store_quad<EPI>(C, ldc, crow0 + row, 16 * (g0 + g) + 4 * fq, N, acc[i][g], bias, vec);
  }
}

template <int MB, int RG, int EPI, int DEPTH>
__global__ void __launch_bounds__(256) gemm_fp8_stream_kernel(
    const u16* __restrict__ A, int lda, const fp8* __restrict__ Wq, int ldw,
    const float* __restrict__ S, int sld, void* __restrict__ C, int ldc, int M, int N, int K,
    int k_split_len, const u16* __restrict__ bias, float* __restrict__ ws) {
  fp8_stream_tile<MB, RG, EPI, DEPTH>([=](int r) { return A + (long)r * lda; }, Wq, ldw, S, sld,
                                      C, ldc, 0, M, N, K, k_split_len, (int)blockIdx.x,
                                      (int)blockIdx.y, (int)gridDim.y, bias, ws);
}

// The grouped (MoE) form on the compact grid: workgroup y takes item y of the tile list that
// dli_moe_align_tiles wrote for 16 MB-row items (tl[0] items, tl[1] their height, then
// (expert, first row) pairs), and runs the tile of that expert's weights Wq[e] / S[e] over its
// rows [m0, m0 + 16 MB) of the permuted rows go[e] .. go[e + 1). x rows are read through arow
// (the token of each permuted row: the gate/up projection, no gathered copy) or in place;
// outputs go to the permuted rows, masked to the item's rows of its expert. An item at or past
// the count, a list of another height or an expert out of range ends the whole workgroup
// before its first barrier. No split-K.
template <int MB, int RG, int EPI, int DEPTH>
__global__ void __launch_bounds__(256) gemm_fp8_stream_grouped_kernel(
    const u16* __restrict__ A, int lda, const fp8* __restrict__ Wq, int ldw,
    const float* __restrict__ S, int sld, void* __restrict__ C, int ldc, int N, int K,
    const int* __restrict__ arow, const int* __restrict__ go, int groups,
    const int* __restrict__ tl) {
  const int it = blockIdx.y;
  if (it >= tl[0] || tl[1] != 16 * MB) return;
  const int e = tl[2 + 2 * it], m0 = tl[3 + 2 * it];
  if (e < 0 || e >= groups || m0 < 0) return;
  const int row0 = go[e] + m0;
  const int Mv = min(16 * MB, go[e + 1] - row0);        // the item's rows of its expert
  if (Mv <= 0) return;
  const fp8* We = Wq + (long)e * N * ldw;
  const float* Se = S + (long)e * (N >> 4) * sld;
  fp8_stream_tile<MB, RG, EPI, DEPTH>(
      [=](int r) { return A + (long)(arow != nullptr ? arow[row0 + r] : row0 + r) * lda; }, We,
      ldw, Se, sld, C, ldc, row0, Mv, N, K, K, (int)blockIdx.x, 0, 1, nullptr, nullptr);
}

template <int MB, int RG, int EPI, int DEPTH>
static int launch_fp8_stream(const void* A, int lda, const void* Wq, const void* S, int sld,
                             int ldw, void* C, int ldc, int M, int N, int K, int splits,
                             const void* bias, void* ws, hipStream_t st) {
  const dim3 grid(((N >> 4) + 4 * RG - 1) / (4 * RG), splits);
  gemm_fp8_stream_kernel<MB, RG, EPI, DEPTH><<<grid, 256, 0, st>>>(
      (const u16*)A, lda, (const fp8*)Wq, ldw, (const float*)S, sld, C, ldc, M, N, K, K / splits,
      (const u16*)bias, (float*)ws);
  if (splits > 1 && C != nullptr) {
    const int outN = (EPI == EPI_SILU) ? N / 2 : N;
    const long total = (long)M * outN;
    splitk_reduce_kernel<EPI><<<(int)((total + 255) / 256), 256, 0, st>>>(
        C, ldc, (const float*)ws, M, N, splits, (const u16*)bias);
  }
  DLI_RETURN_LAUNCH();
}

// tile 70: 64 weight rows a workgroup (a wave holds one group, 4 blocks = 8 steps in flight);
// tile 71: 128 rows (two groups a wave, 2 blocks = 4 steps of both in flight)
template <int EPI>
static int dispatch_fp8_stream(int tile_cfg, const void* A, int lda, const void* Wq,
                               const void* S, int sld, int ldw, void* C, int ldc, int M, int N,
                               int K, int splits, const void* bias, void* ws, hipStream_t st) {
#define DLI_F8S(MB)                                                                           \
  return tile_cfg == 70                                                                       \
             ? launch_fp8_stream<MB, 1, EPI, 4>(A, lda, Wq, S, sld, ldw, C, ldc, M, N, K,      \
                                                splits, bias, ws, st)                         \
             : launch_fp8_stream<MB, 2, EPI, 2>(A, lda, Wq, S, sld, ldw, C, ldc, M, N, K,      \
                                                splits, bias, ws, st)
  if (M <= 16) DLI_F8S(1);
  if (M <= 32) DLI_F8S(2);
  if (M <= 48) DLI_F8S(3);
  DLI_F8S(4);
#undef DLI_F8S
}

// scales: [N / 16, sld] fp32 with sld >= ceil(K / 128). Epilogues: bf16, fp32, SiLU(gate) * up
// (N % 32 == 0), bias; splits > 1: fp32 slabs in ws, reduced into C unless C is null (the
// fused consumers of fused_reduce.hip read them, slab format 0).
extern "C" int dli_gemm_fp8_stream(const void* A, int lda, const void* Wq, const void* scales,
                                   int sld, int ldw, void* C, int ldc, int M, int N, int K,
                                   int epi, int tile_cfg, int splits, const void* bias, void* ws,
                                   hipStream_t st) {
  if (M <= 0 || N <= 0) return 0;
  if (tile_cfg != 70 && tile_cfg != 71) return (int)hipErrorInvalidValue;
  if (M > 64 || N % 16 || K < 16 || K % 16 || ldw % 16 || ldw < K || lda % 8 || lda < K ||
      A == nullptr || Wq == nullptr || scales == nullptr || ((uintptr_t)A | (uintptr_t)Wq) % 16 ||
      sld < (K + 127) / 128)
    return (int)hipErrorInvalidValue;
  if (splits < 1 || K % splits || (splits > 1 && ((K / splits) % 128 || ws == nullptr)) ||
      (C == nullptr && splits < 2))
    return (int)hipErrorInvalidValue;
  if ((epi == EPI_SILU && N % 32) || (epi == EPI_BIAS && bias == nullptr))
    return (int)hipErrorInvalidValue;
  switch (epi) {
    case EPI_BF16: return dispatch_fp8_stream<EPI_BF16>(tile_cfg, A, lda, Wq, scales, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_F32: return dispatch_fp8_stream<EPI_F32>(tile_cfg, A, lda, Wq, scales, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_SILU: return dispatch_fp8_stream<EPI_SILU>(tile_cfg, A, lda, Wq, scales, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_BIAS: return dispatch_fp8_stream<EPI_BIAS>(tile_cfg, A, lda, Wq, scales, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    default: return (int)hipErrorInvalidValue;
  }
}

template <int EPI>
static int dispatch_fp8_stream_grouped(int tile_cfg, int mb, const void* A, int lda,
                                       const void* Wq, const void* S, int sld, int ldw, void* C,
                                       int ldc, int N, int K, const int* arow, const int* go,
                                       int groups, const int* tl, int tl_max, hipStream_t st) {
#define DLI_F8G(MB, RG, DEPTH)                                                                \
  gemm_fp8_stream_grouped_kernel<MB, RG, EPI, DEPTH>                                          \
      <<<dim3(((N >> 4) + 4 * RG - 1) / (4 * RG), tl_max), 256, 0, st>>>(                     \
          (const u16*)A, lda, (const fp8*)Wq, ldw, (const float*)S, sld, C, ldc, N, K, arow,  \
          go, groups, tl)
#define DLI_F8G_MB(MB)                                                                        \
  case MB:                                                                                    \
    if (tile_cfg == 70) DLI_F8G(MB, 1, 4);                                                    \
    else DLI_F8G(MB, 2, 2);                                                                   \
    break
  switch (mb) {
    DLI_F8G_MB(1);
    DLI_F8G_MB(2);
    DLI_F8G_MB(3);
    DLI_F8G_MB(4);
    default: return (int)hipErrorInvalidValue;
  }
#undef DLI_F8G_MB
#undef DLI_F8G
  DLI_RETURN_LAUNCH();
}

// The grouped FP8 weight stream: Wq [groups, N, ldw] e4m3fn, scales [groups, N / 16, sld] fp32,
// M the total permuted rows, group_off int[groups + 1] their offsets per expert, tile_list what
// dli_moe_align_tiles wrote for bm-row items (bm 16 / 32 / 48 / 64) and max_items
// (>= ceil(M / bm) + groups) the host bound on its count that sizes the grid. arow (nullable):
// the row of A behind each permuted row. Epilogues bf16, fp32 and SiLU(gate) * up; splits 1.
extern "C" int dli_gemm_fp8_stream_grouped(const void* A, int lda, const void* Wq,
                                           const void* scales, int sld, int ldw, void* C, int ldc,
                                           int M, int N, int K, int epi, int tile_cfg, int splits,
                                           int bm, const int* arow, const int* group_off,
                                           int groups, const int* tile_list, int max_items,
                                           hipStream_t st) {
  if (tile_cfg != 70 && tile_cfg != 71) return (int)hipErrorInvalidValue;
  if (splits != 1 || group_off == nullptr || tile_list == nullptr || groups < 1 || bm < 16 ||
      bm > 64 || bm % 16)
    return (int)hipErrorInvalidValue;
  if (M < 0 || max_items > 65535 || (long)max_items < ((long)M + bm - 1) / bm + groups)
    return (int)hipErrorInvalidValue;
  if (M == 0 || N <= 0) return 0;
  if (N % 16 || K < 16 || K % 16 || ldw % 16 || ldw < K || lda % 8 || lda < K || A == nullptr ||
      Wq == nullptr || scales == nullptr || C == nullptr ||
      ((uintptr_t)A | (uintptr_t)Wq) % 16 || sld < (K + 127) / 128)
    return (int)hipErrorInvalidValue;
  if (epi == EPI_SILU && N % 32) return (int)hipErrorInvalidValue;
  switch (epi) {
    case EPI_BF16: return dispatch_fp8_stream_grouped<EPI_BF16>(tile_cfg, bm / 16, A, lda, Wq, scales, sld, ldw, C, ldc, N, K, arow, group_off, groups, tile_list, max_items, st);
    case EPI_F32: return dispatch_fp8_stream_grouped<EPI_F32>(tile_cfg, bm / 16, A, lda, Wq, scales, sld, ldw, C, ldc, N, K, arow, group_off, groups, tile_list, max_items, st);
    case EPI_SILU: return dispatch_fp8_stream_grouped<EPI_SILU>(tile_cfg, bm / 16, A, lda, Wq, scales, sld, ldw, C, ldc, N, K, arow, group_off, groups, tile_list, max_items, st);
    default: return (int)hipErrorInvalidValue;
  }
}
