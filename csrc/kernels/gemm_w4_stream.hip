// 4-bit group-scaled weights at decode batches 5..64 (tile ids 74 / 75, dli_gemm_w4_stream):
// C[M, N] = A[M, K] . W[N, K]^T with A bf16, 4 < M <= 64, and W an ops.W4Weight (q_packed
// [N, K / 2] bytes of nibbles, sz [N, K / 128] words; value, nibble order and sz word as gemv.h
// WInt4 / ops/reference.py have them). The nibbles are streamed once from HBM, widened in
// registers and fed to the MFMAs: no bf16 image is written (ops.W4Weight.bf16 + dli_gemm, the
// path of every other M > 4). The loop is gemm_fp8_stream.hip's where the formats agree.
//
// A workgroup is 4 waves; a wave owns RG 16-row groups of W (tile 74: RG 1, 64 weight rows a
// workgroup; tile 75: RG 2, 128 rows) over the workgroup's K slice, which it walks in
// 128-column blocks, the W4 groups. Per block and group, lane (fr = lane & 15, fq = lane >> 4)
// loads q[n0 + fr][k0 + 32 fq .. +32) as one 16-B nontemporal load, DEPTH blocks ahead of its
// use (a register ring). Word m of the load is the 8 elements k0 + 32 fq + 8 m .. +8, and
// ((word >> 4 i) & 0x000F000F) | 0x43004300, i = 0..3, are their bf16 pairs 128 + q in the
// natural order (exact): operand A of one v_mfma_f32_16x16x32_bf16, whose operand B is
// x[16 i + fr][k0 + 32 fq + 8 m .. +8), one 16-B LDS read. Four MFMAs per (x row block i,
// group g) and block, started from zero. Transposed accumulators (gemm_common.h): the lane
// ends up with C[16 i + fr][n0 + 4 fq .. +4), so the quad stores and the split-K reduce of the
// bf16 families apply.
//
// Scale and zero point leave in fp32, per block:
//   acc[i][g][c] += s[n] * (raw[i][g][c] - (128 + z[n]) * xsum[16 i + fr]),  n = n0 + 4 fq + c,
// xsum the block's sum of the x row. A lane's four columns are four weight rows with an sz word
// each: four dword loads per group and block that ride the ring with the nibbles.
//
// x (at most 64 x K bf16, L2-resident) is shared by the four waves through LDS as in the FP8
// stream: the block's x tile [16 MB rows][128] travels with the weights (one 16-B vector per
// thread and 16 rows), is written to one of two LDS buffers when its block comes up, and read
// from there as B fragments by every wave and group. The 16 threads that carry one x row are
// one DPP row: each sums its 8 elements, the row is reduced by four rotate-adds and its first
// lane writes xsum beside the tile (16 MB floats per buffer). One barrier per block.
//
// Tails: K and every K slice are whole blocks (the launcher refuses the rest). Ring stages past
// the slice's last block still arrive: their indices (nibbles, sz, x) are clamped into the
// slice and the stage is skipped, which is uniform over the workgroup (a zero nibble would be
// 128.0, not 0). Rows >= M and groups >= N / 16 are clamped on load and masked on store.
//
// dli_gemm_w4_stream_grouped is the same loop (w4_stream_tile) for an ops.W4Experts stack
// (q_packed [E, N, K / 2], sz [E, N, K / 128], every expert a W4Weight of its own) over the
// permuted rows of a MoE layer, on the compact grid of the align step's tile list: see
// gemm_w4_stream_grouped_kernel.
#include "gemv.h"

typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));

// the sum over the 16 lanes of a DPP row, in every lane of it (row_ror 8, 4, 2, 1)
__device__ __forceinline__ float row16_sum(float v) {
#define DLI_ROR_ADD(CTRL)                                                                  \
  v += __builtin_bit_cast(                                                                 \
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false))
  DLI_ROR_ADD(0x128);
  DLI_ROR_ADD(0x124);
  DLI_ROR_ADD(0x122);
  DLI_ROR_ADD(0x121);
#undef DLI_ROR_ADD
  return v;
}

// the fp32 sum of 8 bf16 values: four dot2 against bf16 ones (gemv.h XChunk<WInt4>'s xsum)
__device__ __forceinline__ float sum8_bf16(const u32x4s v) {
  const u32x4s one = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
  return dot8_acc(__builtin_bit_cast(bf16x8v, one), __builtin_bit_cast(bf16x8v, v), 0.f);
}

// One workgroup's tile: the 16 MB rows xrow(0 .. M) against the weight rows of column block cb,
// over K slice ks of nks; outputs to rows crow0 + r of C. Shared by the dense grid (the rows of
// A, crow0 0) and the grouped one (an item of an expert's rows, gemm_w4_stream_grouped_kernel).
template <int MB, int RG, int EPI, int DEPTH, class XRow>
__device__ __forceinline__ void w4_stream_tile(
    XRow xrow, const uint8_t* __restrict__ Wq, int ldw, const uint32_t* __restrict__ SZ, int sld,
    void* __restrict__ C, int ldc, int crow0, int M, int N, int k_split_len, int cb, int ks,
    int nks, const u16* __restrict__ bias, float* __restrict__ ws) {
  static_assert(DEPTH % 2 == 0, "block t uses LDS buffer t & 1 = u & 1");
  static_assert(EPI != EPI_SILU || RG <= 2, "a gate/up pair is two groups");
  constexpr int ROWS = 16 * MB;
  constexpr int RS = 17;                        // 16-B vectors per LDS row: 16 + 1 of padding
  __shared__ u32x4s xs[2][ROWS * RS];
  __shared__ float xsum[2][ROWS];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
  const int kb = ks * k_split_len;
  const int nblk = k_split_len >> 7;            // blocks of the slice (whole: the launcher)
  const int ngrp = N >> 4;
  const int g0 = (cb * 4 + wid) * RG;           // the wave's first group
  const u32x4s* wrow[RG];
  const uint32_t* srow[RG];                     // sz of the lane's first column, this slice
#pragma unroll
  for (int g = 0; g < RG; ++g) {
    const int grp = min(g0 + g, ngrp - 1);
    wrow[g] = reinterpret_cast<const u32x4s*>(Wq + (((long)(grp * 16 + fr) * ldw + kb) >> 1));
    srow[g] = SZ + (long)(grp * 16 + 4 * fq) * sld + (kb >> 7);
  }
  // the x tile of a block: thread t takes vector t & 15 of rows (t >> 4) + 16 j
  const int xr = threadIdx.x >> 4, xc = threadIdx.x & 15;
  const u32x4s* xsrc[MB];
#pragma unroll
  for (int j = 0; j < MB; ++j)
    xsrc[j] = reinterpret_cast<const u32x4s*>(xrow(min(xr + 16 * j, M - 1)) + kb);

  u32x4s w[DEPTH][RG];
  uint32_t zs[DEPTH][RG][4];
  u32x4s xg[DEPTH][MB];
  // request block T into ring stage U (the block clamped into the slice)
#define DLI_W4S_ISSUE(U, T)                                                             \
  {                                                                                     \
    const int t_ = min((T), nblk - 1);                                                  \
    _Pragma("unroll") for (int g = 0; g < RG; ++g) {                                    \
      w[U][g] = __builtin_nontemporal_load(wrow[g] + t_ * 4 + fq);                      \
      _Pragma("unroll") for (int c = 0; c < 4; ++c) zs[U][g][c] = srow[g][c * sld + t_]; \
    }                                                                                   \
    _Pragma("unroll") for (int j = 0; j < MB; ++j) xg[U][j] = xsrc[j][t_ * 16 + xc];    \
  }
#pragma unroll
  for (int u = 0; u < DEPTH; ++u) {
    DLI_W4S_ISSUE(u, u)
    // oldest block first, as the loop refills them (gemm_fp8_stream.hip)
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  }

  f32x4 acc[MB][RG];
#pragma unroll
  for (int i = 0; i < MB; ++i)
#pragma unroll
    for (int g = 0; g < RG; ++g) acc[i][g] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int b = 0; b < nblk; b += DEPTH) {
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
      const int t = b + u;
      if (t < nblk) {                           // (uniform over the workgroup: the barrier)
        u32x4s* buf = xs[u & 1];
        float* bsum = xsum[u & 1];
#pragma unroll
        for (int j = 0; j < MB; ++j) {
          buf[(xr + 16 * j) * RS + xc] = xg[u][j];
          const float s = row16_sum(sum8_bf16(xg[u][j]));
          if (xc == 0) bsum[xr + 16 * j] = s;
        }
        lgkmcnt0();
        raw_barrier();
        f32x4 raw[MB][RG];
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
          for (int g = 0; g < RG; ++g) raw[i][g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          bf16x8 wf[RG];
#pragma unroll
          for (int g = 0; g < RG; ++g) {
            const uint32_t v = w[u][g][m];
            const u32x4s p = {(v & 0x000F000Fu) | 0x43004300u,
                              ((v >> 4) & 0x000F000Fu) | 0x43004300u,
                              ((v >> 8) & 0x000F000Fu) | 0x43004300u,
                              ((v >> 12) & 0x000F000Fu) | 0x43004300u};
            wf[g] = __builtin_bit_cast(bf16x8, p);
          }
#pragma unroll
          for (int i = 0; i < MB; ++i) {
            const bf16x8 xf = __builtin_bit_cast(bf16x8, buf[(16 * i + fr) * RS + 4 * fq + m]);
#pragma unroll
            for (int g = 0; g < RG; ++g)
              raw[i][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[g], xf, raw[i][g], 0, 0, 0);
          }
        }
        float xsv[MB];
#pragma unroll
        for (int i = 0; i < MB; ++i) xsv[i] = bsum[16 * i + fr];
#pragma unroll
        for (int g = 0; g < RG; ++g)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            // 128 + z as fp32: 0x43000000 has ulp 2^-16, so z sits at bit 16, where sz keeps it
            const uint32_t word = zs[u][g][c];
            const float zf = __uint_as_float(0x43000000u | (word & 0x000F0000u));
            const float sc = (float)__builtin_bit_cast(_Float16, (uint16_t)(word & 0xFFFFu));
#pragma unroll
            for (int i = 0; i < MB; ++i)
              acc[i][g][c] = fmaf(sc, fmaf(-zf, xsv[i], raw[i][g][c]), acc[i][g][c]);
          }
        // the stage is read before its refill is requested (gemm_fp8_stream.hip)
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
          for (int g = 0; g < RG; ++g) asm volatile("" : "+v"(acc[i][g]) : : "memory");
        DLI_W4S_ISSUE(u, t + DEPTH)
      }
    }
  }
#undef DLI_W4S_ISSUE

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
__global__ void __launch_bounds__(256) gemm_w4_stream_kernel(
    const u16* __restrict__ A, int lda, const uint8_t* __restrict__ Wq, int ldw,
    const uint32_t* __restrict__ SZ, int sld, void* __restrict__ C, int ldc, int M, int N, int K,
    int k_split_len, const u16* __restrict__ bias, float* __restrict__ ws) {
  w4_stream_tile<MB, RG, EPI, DEPTH>([=](int r) { return A + (long)r * lda; }, Wq, ldw, SZ, sld,
                                     C, ldc, 0, M, N, k_split_len, (int)blockIdx.x,
                                     (int)blockIdx.y, (int)gridDim.y, bias, ws);
}

// The grouped (MoE) form on the compact grid: workgroup y takes item y of the tile list that
// dli_moe_align_tiles wrote for 16 MB-row items (tl[0] items, tl[1] their height, then
// (expert, first row) pairs), and runs the tile of that expert's weights Wq[e] / SZ[e] over its
// rows [m0, m0 + 16 MB) of the permuted rows go[e] .. go[e + 1). x rows are read through arow
// (the token of each permuted row: the gate/up projection, no gathered copy) or in place;
// outputs go to the permuted rows, masked to the item's rows of its expert. An item at or past
// the count, a list of another height, an expert out of range or a negative row ends the whole
// workgroup before its first barrier. No split-K: the slice is all of K.
template <int MB, int RG, int EPI, int DEPTH>
__global__ void __launch_bounds__(256) gemm_w4_stream_grouped_kernel(
    const u16* __restrict__ A, int lda, const uint8_t* __restrict__ Wq, int ldw,
    const uint32_t* __restrict__ SZ, int sld, void* __restrict__ C, int ldc, int N, int K,
    const int* __restrict__ arow, const int* __restrict__ go, int groups,
    const int* __restrict__ tl) {
  const int it = blockIdx.y;
  if (it >= tl[0] || tl[1] != 16 * MB) return;
  const int e = tl[2 + 2 * it], m0 = tl[3 + 2 * it];
  if (e < 0 || e >= groups || m0 < 0) return;
  const int row0 = go[e] + m0;
  const int Mv = min(16 * MB, go[e + 1] - row0);        // the item's rows of its expert
  if (Mv <= 0) return;
  const uint8_t* We = Wq + (((long)e * N * ldw) >> 1);
  const uint32_t* Se = SZ + (long)e * N * sld;
  w4_stream_tile<MB, RG, EPI, DEPTH>(
      [=](int r) { return A + (long)(arow != nullptr ? arow[row0 + r] : row0 + r) * lda; }, We,
      ldw, Se, sld, C, ldc, row0, Mv, N, K, (int)blockIdx.x, 0, 1, nullptr, nullptr);
}

template <int MB, int RG, int EPI, int DEPTH>
static int launch_w4_stream(const void* A, int lda, const void* Wq, const void* sz, int sld,
                            int ldw, void* C, int ldc, int M, int N, int K, int splits,
                            const void* bias, void* ws, hipStream_t st) {
  const dim3 grid(((N >> 4) + 4 * RG - 1) / (4 * RG), splits);
  gemm_w4_stream_kernel<MB, RG, EPI, DEPTH><<<grid, 256, 0, st>>>(
      (const u16*)A, lda, (const uint8_t*)Wq, ldw, (const uint32_t*)sz, sld, C, ldc, M, N, K,
      K / splits, (const u16*)bias, (float*)ws);
  if (splits > 1 && C != nullptr) {
    const int outN = (EPI == EPI_SILU) ? N / 2 : N;
    const long total = (long)M * outN;
    splitk_reduce_kernel<EPI><<<(int)((total + 255) / 256), 256, 0, st>>>(
        C, ldc, (const float*)ws, M, N, splits, (const u16*)bias);
  }
  DLI_RETURN_LAUNCH();
}

// tile 74: 64 weight rows a workgroup (a wave holds one group, D74 blocks in flight);
// tile 75: 128 rows (two groups a wave, D75 blocks of both in flight). The ring depth per MB is
// what keeps every instantiation at two waves per SIMD without scratch
// (profiles/w4_weights/README.md)
template <int EPI>
static int dispatch_w4_stream(int tile_cfg, const void* A, int lda, const void* Wq,
                              const void* sz, int sld, int ldw, void* C, int ldc, int M, int N,
                              int K, int splits, const void* bias, void* ws, hipStream_t st) {
#define DLI_W4S(MB, D74, D75)                                                                 \
  return tile_cfg == 74                                                                       \
             ? launch_w4_stream<MB, 1, EPI, D74>(A, lda, Wq, sz, sld, ldw, C, ldc, M, N, K,    \
                                                 splits, bias, ws, st)                        \
             : launch_w4_stream<MB, 2, EPI, D75>(A, lda, Wq, sz, sld, ldw, C, ldc, M, N, K,    \
                                                 splits, bias, ws, st)
  if (M <= 16) DLI_W4S(1, 8, 4);
  if (M <= 32) DLI_W4S(2, 8, 4);
  if (M <= 48) DLI_W4S(3, 6, 4);
  DLI_W4S(4, 6, 4);
#undef DLI_W4S
}

// sz: [N, sld] words with sld >= K / 128; ldw: the row stride of Wq in K-elements (ldw / 2
// bytes). Epilogues: bf16, fp32, SiLU(gate) * up (N % 32 == 0), bias; splits > 1: fp32 slabs
// in ws, reduced into C unless C is null (the fused consumers of fused_reduce.hip read them,
// slab format 0).
extern "C" int dli_gemm_w4_stream(const void* A, int lda, const void* Wq, const void* sz,
                                  int sld, int ldw, void* C, int ldc, int M, int N, int K,
                                  int epi, int tile_cfg, int splits, const void* bias, void* ws,
                                  hipStream_t st) {
  if (M <= 0 || N <= 0) return 0;
  if (tile_cfg != 74 && tile_cfg != 75) return (int)hipErrorInvalidValue;
  if (M > 64 || N % 16 || K < 128 || K % 128 || ldw % 32 || ldw < K || lda % 8 || lda < K ||
      A == nullptr || Wq == nullptr || sz == nullptr || ((uintptr_t)A | (uintptr_t)Wq) % 16 ||
      (uintptr_t)sz % 4 || sld < K / 128)
    return (int)hipErrorInvalidValue;
  if (splits < 1 || K % splits || (K / splits) % 128 || (splits > 1 && ws == nullptr) ||
      (C == nullptr && splits < 2))
    return (int)hipErrorInvalidValue;
  if ((epi == EPI_SILU && N % 32) || (epi == EPI_BIAS && bias == nullptr))
    return (int)hipErrorInvalidValue;
  switch (epi) {
    case EPI_BF16: return dispatch_w4_stream<EPI_BF16>(tile_cfg, A, lda, Wq, sz, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_F32: return dispatch_w4_stream<EPI_F32>(tile_cfg, A, lda, Wq, sz, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_SILU: return dispatch_w4_stream<EPI_SILU>(tile_cfg, A, lda, Wq, sz, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_BIAS: return dispatch_w4_stream<EPI_BIAS>(tile_cfg, A, lda, Wq, sz, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    default: return (int)hipErrorInvalidValue;
  }
}

// The grouped ring: the expert K of interest is short (Qwen3-30B-A3B's down projection is 6
// blocks), so tile 74 holds 6 blocks at every MB (the dense 8 at MB 1 / 2 would refill two
// clamped stages per trip there) and tile 75 the dense 4; registers and occupancy in
// profiles/w4_experts/README.md.
template <int EPI>
static int dispatch_w4_stream_grouped(int tile_cfg, int mb, const void* A, int lda,
                                      const void* Wq, const void* sz, int sld, int ldw, void* C,
                                      int ldc, int N, int K, const int* arow, const int* go,
                                      int groups, const int* tl, int tl_max, hipStream_t st) {
#define DLI_W4G(MB, RG, DEPTH)                                                                \
  gemm_w4_stream_grouped_kernel<MB, RG, EPI, DEPTH>                                           \
      <<<dim3(((N >> 4) + 4 * RG - 1) / (4 * RG), tl_max), 256, 0, st>>>(                     \
          (const u16*)A, lda, (const uint8_t*)Wq, ldw, (const uint32_t*)sz, sld, C, ldc, N, K, \
          arow, go, groups, tl)
#define DLI_W4G_MB(MB)                                                                        \
  case MB:                                                                                    \
    if (tile_cfg == 74) DLI_W4G(MB, 1, 6);                                                    \
    else DLI_W4G(MB, 2, 4);                                                                   \
    break
  switch (mb) {
    DLI_W4G_MB(1);
    DLI_W4G_MB(2);
    DLI_W4G_MB(3);
    DLI_W4G_MB(4);
    default: return (int)hipErrorInvalidValue;
  }
#undef DLI_W4G_MB
#undef DLI_W4G
  DLI_RETURN_LAUNCH();
}

// The grouped W4 weight stream: Wq [groups, N, ldw / 2] nibble bytes, sz [groups, N, sld] words,
// M the total permuted rows, group_off int[groups + 1] their offsets per expert, tile_list what
// dli_moe_align_tiles wrote for bm-row items (bm 16 / 32 / 48 / 64) and max_items
// (>= ceil(M / bm) + groups) the host bound on its count that sizes the grid. arow (nullable):
// the row of A behind each permuted row. Epilogues bf16, fp32 and SiLU(gate) * up; splits 1.
extern "C" int dli_gemm_w4_stream_grouped(const void* A, int lda, const void* Wq, const void* sz,
                                          int sld, int ldw, void* C, int ldc, int M, int N, int K,
                                          int epi, int tile_cfg, int splits, int bm,
                                          const int* arow, const int* group_off, int groups,
                                          const int* tile_list, int max_items, hipStream_t st) {
  if (tile_cfg != 74 && tile_cfg != 75) return (int)hipErrorInvalidValue;
  if (splits != 1 || group_off == nullptr || tile_list == nullptr || groups < 1 || bm < 16 ||
      bm > 64 || bm % 16)
    return (int)hipErrorInvalidValue;
  if (M < 0 || max_items > 65535 || (long)max_items < ((long)M + bm - 1) / bm + groups)
    return (int)hipErrorInvalidValue;
  if (M == 0 || N <= 0) return 0;
  if (N % 16 || K < 128 || K % 128 || ldw % 32 || ldw < K || lda % 8 || lda < K || A == nullptr ||
      Wq == nullptr || sz == nullptr || C == nullptr || ((uintptr_t)A | (uintptr_t)Wq) % 16 ||
      ((uintptr_t)sz | (uintptr_t)arow | (uintptr_t)group_off | (uintptr_t)tile_list) % 4 ||
      sld < K / 128)
    return (int)hipErrorInvalidValue;
  if (epi == EPI_SILU && N % 32) return (int)hipErrorInvalidValue;
  switch (epi) {
    case EPI_BF16: return dispatch_w4_stream_grouped<EPI_BF16>(tile_cfg, bm / 16, A, lda, Wq, sz, sld, ldw, C, ldc, N, K, arow, group_off, groups, tile_list, max_items, st);
    case EPI_F32: return dispatch_w4_stream_grouped<EPI_F32>(tile_cfg, bm / 16, A, lda, Wq, sz, sld, ldw, C, ldc, N, K, arow, group_off, groups, tile_list, max_items, st);
    case EPI_SILU: return dispatch_w4_stream_grouped<EPI_SILU>(tile_cfg, bm / 16, A, lda, Wq, sz, sld, ldw, C, ldc, N, K, arow, group_off, groups, tile_list, max_items, st);
    default: return (int)hipErrorInvalidValue;
  }
}
