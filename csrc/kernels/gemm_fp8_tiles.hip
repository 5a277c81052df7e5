// FP8 block-scaled weights past 64 rows (tile ids 72 / 73, dli_gemm_fp8_tiles):
// C[M, N] = epi(A[M, K] . W[N, K]^T) with A bf16 and W an ops.Fp8Weight (q [N, K] e4m3fn bytes,
// scales [N / 16, K / 128] fp32, W[n, k] = q[n, k] * s[n >> 4][k >> 7]), K a multiple of 128.
// The definition is the stream tiles' (gemm_fp8_stream.hip): no rounded bf16 W is formed, the
// MFMAs of one 128-column scale block start from zero and acc += s * block_sum in fp32, so an
// output keeps its definition when a batch crosses 64 rows. What differs is the data path: at
// 65..512 rows the operand that must be tiled through LDS is x, and the weight bytes must be
// shared by the waves that split M, so this is an LDS-tiled kernel of the gemm_tiles.hip shape
// whose weight K-tile stays FP8 until it is in registers.
//
// One K-tile is one scale block. Its W part is BN rows x 128 BYTES, its A part BM x 128 bf16
// as two 64-column half tiles of BM rows x 128 B: every part has the 128-B row geometry of the
// bf16 family, so one global_load_lds wave instruction stages 8 rows and 16-B chunk c of a row
// lands at chunk c ^ ((row >> 1) & 7) (the swizzle of read_frag). All parts are filled by
// LDS-DMA into a ring of NS stages; a counted vmcnt retires the oldest K-tile only and a raw
// s_barrier publishes it (the loop of gemm_bf16_kernel's NS >= 3 form; with NS 2 nothing stays
// in flight across the barrier, but the next tile's DMA still runs under this tile's MFMAs).
//
// Fragments: lane (fr = lane & 15, fq = lane >> 4) reads, for weight block j and step h2, chunk
// 4 h2 + fq of weight row 16 j + fr: 16 K-elements in one ds_read_b128, which fp8x16_to_bf16
// (exact) turns into two bf16x8 MFMA operands, K indices 64 h2 + 16 fq + 8 h .. +8 for
// h = 0, 1. They meet the x fragments of the same K indices: chunks 2 fq + h of half tile h2.
// The weight fragment is MFMA operand A (transposed accumulators, gemm_common.h): the lane
// holds C[16 i + fr][16 j + 4 fq .. +4), so the quad stores, the SiLU pairing, the fp32 slab
// stores and the split-K reduce of the bf16 families apply as they are.
//
// The scale s[(n0 + 16 j) >> 4][block] is wave-uniform: the wave index is made scalar
// (readfirstlane), so the NI scales of a block are scalar loads, issued after the block's
// barrier and used after its MFMAs.
//
// Tails: rows >= M and weight rows >= N are clamped on load and masked on store (N is a
// multiple of 16, not of BN); the scale group is clamped with the weight row. No partial K
// block exists: the launcher refuses K or a K slice that is no multiple of 128 (LDS-DMA cannot
// zero a partial block), and such a call keeps the dequantise path.
#include "gemm_common.h"

// 16-B chunk c of tile row `row` of an LDS part of 128-B rows (read_frag's swizzle)
__device__ __forceinline__ uint4 lds_chunk(const char* part, int row, int c) {
  return *reinterpret_cast<const uint4*>(part + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
}

template <int BM, int BN, int NS, int WM, int WN, int EPI>
__global__ void __launch_bounds__(64 * WM * WN) gemm_fp8_tiles_kernel(
    const u16* __restrict__ A, int lda, const fp8* __restrict__ Wq, int ldw,
    const float* __restrict__ S, int sld, void* __restrict__ C, int ldc, int M, int N, int K,
    int k_split_len, const u16* __restrict__ bias, float* __restrict__ ws) {
  constexpr int NW = WM * WN;                      // waves: WM along M x WN along N
  constexpr int TM = BM / WM, TN = BN / WN;        // wave tile
  constexpr int MI = TM / 16, NI = TN / 16;        // 16x16 MFMA blocks per wave
  constexpr int AH_BYTES = BM * 128;               // one 64-column half tile of x
  constexpr int A_BYTES = 2 * AH_BYTES, W_BYTES = BN * 128, BUF = A_BYTES + W_BYTES;
  // one glds wave-instruction stages 8 rows x 128 B; all NW waves share each part
  constexpr int AH_INSTR = BM / (8 * NW), W_INSTR = BN / (8 * NW);
  constexpr int INSTR = 2 * AH_INSTR + W_INSTR;
  static_assert(AH_INSTR * 8 * NW == BM && W_INSTR * 8 * NW == BN, "tile vs waves");
  static_assert(NS >= 2 && TM % 16 == 0 && TN % 32 == 0, "ring; whole gate/up pairs a wave");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // ---- tile coordinates: block_coord's dense form (XCD remap, split-major with split-K)
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  int tile, ks, m0, n0;
  split_tile(tiles_m * tiles_n, false, tile, ks);
  tile_origin<BM, BN, 1>(tile, tiles_m, tiles_n, m0, n0);
  const int kb = ks * k_split_len;
  const int nk = min(k_split_len, K - kb) >> 7;    // scale blocks of this K slice

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid % WN;

  // ---- per-lane glds sources (row clamped in range; swizzled chunk): 8 bf16 / 16 fp8 a lane
  const u16* a_src[AH_INSTR];
  const fp8* w_src[W_INSTR];
#pragma unroll
  for (int i = 0; i < AH_INSTR; ++i) {
    const int r = (i * NW + wid) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    a_src[i] = A + (long)min(m0 + r, M - 1) * lda + kb + c * 8;
  }
#pragma unroll
  for (int i = 0; i < W_INSTR; ++i) {
    const int r = (i * NW + wid) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    w_src[i] = Wq + (long)min(n0 + r, N - 1) * ldw + kb + c * 16;
  }
  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * BUF;
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
      for (int i = 0; i < AH_INSTR; ++i)
        __builtin_amdgcn_global_load_lds(
            (gbl_void*)(a_src[i] + kt * 128 + h2 * 64),
            (lds_void*)(base + h2 * AH_BYTES + (i * NW + wid) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < W_INSTR; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void*)(w_src[i] + kt * 128),
                                       (lds_void*)(base + A_BYTES + (i * NW + wid) * 1024), 16,
                                       0, 0);
  };

  // ---- the wave's scale rows (scalar: group clamped as the weight rows are)
  const float* srow[NI];
#pragma unroll
  for (int j = 0; j < NI; ++j)
    srow[j] = S + (long)min(((n0 + wn * TN) >> 4) + j, (N >> 4) - 1) * sld + (kb >> 7);

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  int a_row[MI], w_row[NI];
#pragma unroll
  for (int i = 0; i < MI; ++i) a_row[i] = wm * TM + i * 16 + fr;
#pragma unroll
  for (int j = 0; j < NI; ++j) w_row[j] = wn * TN + j * 16 + fr;

  // one scale block from buffer buf: raw = sum over its 128 columns, then acc += s * raw
  auto compute = [&](int buf, const float (&sc)[NI]) {
    const char* abuf = smem + buf * BUF;
    const char* wbuf = abuf + A_BYTES;
    f32x4 raw[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) raw[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      bf16x8 wl[NI], wh[NI];
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        uint4 lo, hi;
        fp8x16_to_bf16(lds_chunk(wbuf, w_row[j], 4 * h2 + fq), lo, hi);
        wl[j] = __builtin_bit_cast(bf16x8, lo);
        wh[j] = __builtin_bit_cast(bf16x8, hi);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const char* half = abuf + h2 * AH_BYTES;
        const bf16x8 xa = __builtin_bit_cast(bf16x8, lds_chunk(half, a_row[i], 2 * fq));
        const bf16x8 xb = __builtin_bit_cast(bf16x8, lds_chunk(half, a_row[i], 2 * fq + 1));
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          raw[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[j], xa, raw[i][j], 0, 0, 0);
          raw[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[j], xb, raw[i][j], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j) acc[i][j] += sc[j] * raw[i][j];
  };

  // ---- the ring: NS - 2 K-tiles stay in flight across the barrier (gemm_bf16_kernel's loop).
  // The restaged buffer (kt + NS - 1) % NS was last read in iteration kt - 1, whose reads
  // every wave has retired (lgkmcnt(0)) before it reaches this iteration's barrier.
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nk) stage(s, s);
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    const int ahead = min(nk - 1 - kt, NS - 2);     // tiles issued after kt (uniform)
    wait_ahead<INSTR, NS - 2>(ahead);
    lgkmcnt0();
    raw_barrier();
    if (kt + NS - 1 < nk) {
      int nb = cur + NS - 1;
      if (nb >= NS) nb -= NS;
      stage(nb, kt + NS - 1);
    }
    float sc[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) sc[j] = srow[j][kt];
    compute(cur, sc);
    cur = (cur + 1 == NS) ? 0 : cur + 1;
  }
  wait_vmcnt<0>();

  // ---- epilogue: acc[i][j][r] = C[m0 + wm TM + 16 i + fr][n0 + wn TN + 16 j + 4 fq + r]
  const int col0 = n0 + wn * TN;
  if (gridDim.y > 1) {                              // fp32 partial slab of this K slice (format 0)
    float* slab = ws + (long)ks * M * N;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = m0 + a_row[i];
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int col = col0 + 16 * j + 4 * fq;
        if (row < M && col < N) slab_quad_fp32(slab + (long)row * N + col, acc[i][j], 0, true, 4);
      }
    }
    return;
  }
  const bool vec = out_vec<EPI>(C, ldc, N, bias);
  if constexpr (EPI == EPI_SILU) {
    // column blocks j (even) = gate, j + 1 = up of the same 16 features
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = m0 + a_row[i];
#pragma unroll
      for (int j = 0; j < NI; j += 2) {
        const int gcol = col0 + 16 * j;
        if (row < M && gcol < N)
          store_silu_quad(C, ldc, row, (gcol >> 5) * 16 + 4 * fq, acc[i][j], acc[i][j + 1], vec);
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int row = m0 + a_row[i];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int col = col0 + 16 * j + 4 * fq;
      if (row < M && col < N) store_quad<EPI>(C, ldc, row, col, N, acc[i][j], bias, vec);
    }
  }
}

// grid (row tiles x column tiles, splits); dynamic LDS NS x (BM x 256 + BN x 128) B, past
// 64 KiB (the opt-in, once per kernel); then the split-K reduce unless C == nullptr (the slabs
// are left for a fused consumer, fused_reduce.hip)
template <int BM, int BN, int NS, int WM, int WN, int EPI>
static int launch_fp8_tiles(const void* A, int lda, const void* Wq, const void* S, int sld,
                            int ldw, void* C, int ldc, int M, int N, int K, int splits,
                            const void* bias, void* ws, hipStream_t st) {
  constexpr size_t LDS = (size_t)NS * (BM * 256 + BN * 128);
  static_assert(LDS <= 160 * 1024, "the CU's LDS");
  const auto kernel = gemm_fp8_tiles_kernel<BM, BN, NS, WM, WN, EPI>;
  static bool attr_done = false;
  if (!attr_done) {
    const hipError_t e = hipFuncSetAttribute(
        (const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  const long tiles = (long)((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  if (tiles > 0x7fffffffL / splits) return (int)hipErrorInvalidValue;
  kernel<<<dim3((unsigned)tiles, splits), 64 * WM * WN, LDS, st>>>(
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

// tile 72: 128 x 128, 2 x 2 waves, 3 stages of 32 KiB A + 16 KiB W (144 KiB);
// tile 73: 128 x 256, 2 x 4 waves, 2 stages of 32 KiB A + 32 KiB W (128 KiB): two waves a
// SIMD, so one wave's LDS reads and conversions run beside the other's MFMAs
template <int EPI>
static int dispatch_fp8_tiles(int tile_cfg, const void* A, int lda, const void* Wq, const void* S,
                              int sld, int ldw, void* C, int ldc, int M, int N, int K, int splits,
                              const void* bias, void* ws, hipStream_t st) {
  if (tile_cfg == 72)
    return launch_fp8_tiles<128, 128, 3, 2, 2, EPI>(A, lda, Wq, S, sld, ldw, C, ldc, M, N, K,
                                                    splits, bias, ws, st);
  return launch_fp8_tiles<128, 256, 2, 2, 4, EPI>(A, lda, Wq, S, sld, ldw, C, ldc, M, N, K,
                                                  splits, bias, ws, st);
}

// scales: [N / 16, sld] fp32 with sld >= K / 128. Epilogues: bf16, fp32, SiLU(gate) * up
// (N % 32 == 0), bias; splits > 1: fp32 slabs in ws, reduced into C unless C is null (slab
// format 0). The arguments of dli_gemm_fp8_stream; any M >= 1 (the planner decides where).
extern "C" int dli_gemm_fp8_tiles(const void* A, int lda, const void* Wq, const void* scales,
                                  int sld, int ldw, void* C, int ldc, int M, int N, int K,
                                  int epi, int tile_cfg, int splits, const void* bias, void* ws,
                                  hipStream_t st) {
  if (M <= 0 || N <= 0) return 0;
  if (tile_cfg != 72 && tile_cfg != 73) return (int)hipErrorInvalidValue;
  if (N % 16 || K < 128 || K % 128 || ldw % 16 || ldw < K || lda % 8 || lda < K ||
      A == nullptr || Wq == nullptr || scales == nullptr || ((uintptr_t)A | (uintptr_t)Wq) % 16 ||
      sld < K / 128)
    return (int)hipErrorInvalidValue;
  if (splits < 1 || K % splits || (K / splits) % 128 || (splits > 1 && ws == nullptr) ||
      (C == nullptr && splits < 2))
    return (int)hipErrorInvalidValue;
  if ((epi == EPI_SILU && N % 32) || (epi == EPI_BIAS && bias == nullptr))
    return (int)hipErrorInvalidValue;
  switch (epi) {
    case EPI_BF16: return dispatch_fp8_tiles<EPI_BF16>(tile_cfg, A, lda, Wq, scales, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_F32: return dispatch_fp8_tiles<EPI_F32>(tile_cfg, A, lda, Wq, scales, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_SILU: return dispatch_fp8_tiles<EPI_SILU>(tile_cfg, A, lda, Wq, scales, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    case EPI_BIAS: return dispatch_fp8_tiles<EPI_BIAS>(tile_cfg, A, lda, Wq, scales, sld, ldw, C, ldc, M, N, K, splits, bias, ws, st);
    default: return (int)hipErrorInvalidValue;
  }
}
