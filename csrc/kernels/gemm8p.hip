// 8-wave "8-phase ping-pong" MFMA GEMMs (family "8p" of ops/gemm.py's TILE_TABLE): 256x256
// (gemm8p_kernel), 256x224 (gemm8p224_kernel) and 256x128 (gemm8p128_kernel) block tiles, two
// wave groups alternating MFMA and load segments (cdna_hip_programming.md §5 'The 256² 8-phase
// template').
#include "gemm_common.h"

// ---- LDS-DMA staging shared by the three kernels. A piece is 8 tile rows x 128 B, moved by
// one wave instruction: lane L lands at row L / 8, physical chunk L % 8, so it loads logical
// chunk (L % 8) ^ ((r >> 1) & 7) of its row r (clamped into the matrix). A region, the part
// of a K-tile restaged in one phase, is two pieces per wave.
struct Piece {
  int src;                                         // element offset of the lane's source, K-tile 0
  int dst;                                         // LDS byte offset of the piece in a buffer
};
// the piece of first tile row rb of A (is_a) or W; the W image follows a_bytes of A
__device__ __forceinline__ Piece make_piece(bool is_a, int rb, int lane, const BlockCoord& b,
                                            int lda, int N, int ldw, int a_bytes) {
  const int r = rb + (lane >> 3);
  const int c = (lane & 7) ^ ((r >> 1) & 7);
  Piece p;
  if (is_a) p.src = min(b.m0 + r, b.Mg - 1) * lda + b.kb + c * 8;
  else p.src = min(b.n0 + r, N - 1) * ldw + b.kb + c * 8;
  p.dst = (is_a ? 0 : a_bytes) + rb * 128;
  return p;
}
// K-tile kt of one region into the buffer at lds
__device__ __forceinline__ void dma_region(const u16* base, const Piece (&pc)[2], char* lds,
                                           int kt) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
    __builtin_amdgcn_global_load_lds((gbl_void*)(base + pc[i].src + kt * BK),
                                     (lds_void*)(lds + pc[i].dst), 16, 0, 0);
}

// ---------------------------------------------------------------------------------------
// 256x256 "8-phase ping-pong" GEMM (cdna_hip_programming.md §5 'The 256² 8-phase template',
// T3+T4+T5; /opt/skills/guides/MI355X_MICROARCH.md 'Two waves per SIMD' items 1, 7, 9).
//
// 8 waves = 2 groups of 4 (g = wid >> 2 = the wave's 128-row half of the tile; one wave of
// each group per SIMD). Every K-tile (BK = 64) is 4 phases; a phase is a LOAD segment
// (this phase's ds_reads + one quarter of a later K-tile's glds + a counted vmcnt) and a
// MATRIX segment (16 MFMAs, one 64x32 quadrant of the wave's 128x64 output), separated by
// raw s_barriers. Group 1 runs one barrier behind group 0, so on every SIMD one wave is in
// its matrix segment while its partner is in its load segment.
//
//   phase | ds_read_b128 (this K-tile)        | MFMAs          | glds issued
//   0     | A rows 0-63 of the half, B 0-31   | acc[0-3][0-1]  | slot 3 of K-tile T+1
//   1     | B cols 32-63                      | acc[0-3][2-3]  | slot 0 of K-tile T+2
//   2     | A rows 64-127                     | acc[4-7][2-3]  | slot 1 of K-tile T+2
//   3     | -                                 | acc[4-7][0-1]  | slot 2 of K-tile T+2
//
// LDS: 2 buffers x (A 256x64 + W 256x64) bf16 = 128 KiB (1 workgroup / CU), 128-B rows with
// the chunk XOR swizzle of gemm_bf16_kernel. Staging slots per group (2 glds per lane each):
// group 0 stages A rows 0-63 / 64-127 and the even 32-row W chunks, group 1 A rows
// 128-191 / 192-255 and the odd W chunks. With segments numbered s (group 0 loads in even
// s, group 1 in odd s) every slot is restaged >= 2 segments after its last ds_read of the
// K-tile two back (WAR) and retired by its issuer's vmcnt >= 1 barrier before its first
// ds_read (RAW) when every load segment leaves the last 3 segments' glds in flight:
// vmcnt(6) in steady state, fewer when the K loop's tail issues nothing.
template <int EPI>
__global__ void __launch_bounds__(512) gemm8p_kernel(
    const u16* __restrict__ A, int lda, const u16* __restrict__ W, int ldw,
    void* __restrict__ C, int ldc, int M, int N, int K, int k_split_len,
    const u16* __restrict__ bias, float* __restrict__ ws, const int* __restrict__ group_off) {
  constexpr int BM = 256, BN = 256;
  constexpr int A_BYTES = BM * BK * 2, BUF = 2 * A_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const BlockCoord bc = block_coord<BM, BN, 4>(W, ldw, M, N, K, k_split_len, group_off);
  const int row0 = bc.row0, Mg = bc.Mg, m0 = bc.m0, n0 = bc.n0, nk = bc.nk;
  const u16* Wg = bc.Wg;
  if (m0 >= Mg) return;
  const u16* Ab = A + (long)row0 * lda;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wid >> 2, gw = wid & 3;           // group (= M half), wave in group (= N quarter)

  // ---- staging: slot s (0..3) x piece i (0..1)
  Piece pc[4][2];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const bool is_a = (s & 1) == 0;
      const int rb = is_a ? 64 * (2 * g + (s >> 1)) + 32 * i + 8 * gw
                          : 64 * (2 * (s >> 1) + i) + 32 * g + 8 * gw;
      pc[s][i] = make_piece(is_a, rb, lane, bc, lda, N, ldw, A_BYTES);
    }
  auto issue = [&](auto S, int kt) {
    constexpr int s = decltype(S)::value;
    dma_region((s & 1) ? Wg : Ab, pc[s], smem + (kt & 1) * BUF, kt);
  };

  // ---- fragments
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: K-tiles 0 and 1 in full
  if (nk > 0) {
    issue(std::integral_constant<int, 0>{}, 0); issue(std::integral_constant<int, 1>{}, 0);
    issue(std::integral_constant<int, 2>{}, 0); issue(std::integral_constant<int, 3>{}, 0);
  }
  if (nk > 1) {
    issue(std::integral_constant<int, 0>{}, 1); issue(std::integral_constant<int, 1>{}, 1);
    issue(std::integral_constant<int, 2>{}, 1); issue(std::integral_constant<int, 3>{}, 1);
  }
  // (starting once K-tile 0 alone has landed, as gemm8p224_kernel does, was measured and not
  // kept: gate/up 99.1 vs 98.7 us, LM head 456.6 vs 446.2 us at M = 512, profiles/r7/)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (g == 1) {                                    // stagger: group 1 runs one segment behind
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_s_setprio(1);                 // static priority for the younger half
  }

  bf16x8 a0[4][2], a1[4][2], b0[2][2], b1[2][2];
  for (int kt = 0; kt < nk; ++kt) {
    const char* abuf = smem + (kt & 1) * BUF;
    const char* wbuf = abuf + A_BYTES;
    const int arow = g * 128 + fr, wrow = gw * 64 + fr;
    auto phase = [&](auto P) {
      constexpr int p = decltype(P)::value;
      auto reads = [&]() {
        if (p == 0) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) a0[i][kk] = read_frag(abuf, arow + 16 * i, kk, fq);
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) b0[j][kk] = read_frag(wbuf, wrow + 16 * j, kk, fq);
        } else if (p == 1) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) b1[j][kk] = read_frag(wbuf, wrow + 32 + 16 * j, kk, fq);
        } else if (p == 2) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) a1[i][kk] = read_frag(abuf, arow + 64 + 16 * i, kk, fq);
        }
      };
      auto stage = [&]() {
        if (p == 0) {
          if (kt >= 1 && kt + 1 < nk) issue(std::integral_constant<int, 3>{}, kt + 1);
        } else if (kt + 2 < nk) {
          issue(std::integral_constant<int, (p + 3) & 3>{}, kt + 2);
        }
      };
      reads();
      stage();
      // one counted wait per K-tile (the 8-phase template's schedule): at phase 3 of K-tile
      // T every DMA of T+1 is retired; only T+2's slots 0-2 (issued in phases 1-3) stay in
      // flight. Phases 0-2 do not wait at all.
      if (p == 3) {
        if (kt + 2 < nk) wait_vmcnt<6>();
        else wait_vmcnt<0>();
      }
      raw_barrier();
      const bf16x8 (&af)[4][2] = (p < 2) ? a0 : a1;
      const bf16x8 (&bf)[2][2] = (p == 0 || p == 3) ? b0 : b1;
      constexpr int I0 = (p < 2) ? 0 : 4, J0 = (p == 0 || p == 3) ? 0 : 2;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[I0 + i][J0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                bf[j][kk], af[i][kk], acc[I0 + i][J0 + j], 0, 0, 0);
      raw_barrier();
    };
    phase(std::integral_constant<int, 0>{});
    phase(std::integral_constant<int, 1>{});
    phase(std::integral_constant<int, 2>{});
    phase(std::integral_constant<int, 3>{});
  }
  if (g == 0) {                                    // balance group 1's stagger barrier
    __builtin_amdgcn_s_barrier();
  }

  // ---- epilogue (transposed accumulators):
  // acc[I][J][r] = C[m0 + 128g + 16I + fr][n0 + 64gw + 16J + 4fq + r]
  gemm_epilogue<EPI, 8, 4>(acc, m0 + 128 * g, n0 + 64 * gw, bc, C, ldc, M, N, bias, ws, fr, fq);
}

// ---------------------------------------------------------------------------------------
// 256x224 ping-pong GEMM: the 8-phase schedule of gemm8p_kernel for N-tiles of 224 columns,
// so a GEMM whose N is a multiple of 7 x 32 fills the chip where 256-wide tiles leave CUs
// idle: the Llama-3 gate/up projection at M = 512 (N = 28672) is 2 x 128 = 256 tiles on 256
// CUs instead of 224 (one workgroup per CU at 128 KiB of LDS).
//
// Waves: group g = wid >> 2 = the tile's 128-row half (one wave of each group per SIMD,
// group 1 one barrier behind); in a group, wave (wm, wn) = (w4 >> 1, w4 & 1) owns rows
// 128 g + 64 wm .. +63 and columns 112 wn .. +111: 4 x 7 MFMA blocks, as gemm8p's 8 x 4.
// K-tile T (BK = 64) = 4 phases, each a LOAD segment (ds_reads of T, LDS-DMA of T+2) and a
// MATRIX segment (MFMAs):
//   phase | reads                              | MFMAs              | DMA for T+2
//   0     | A rows +0..31 (both kk), B +0..63  | 2 x 4 blocks       | -
//   1     | B +64..111                         | 2 x 3 blocks       | A "h0", B "h0"
//   2     | A rows +32..63                     | 2 x 3 blocks       | B "h1"
//   3     | -                                  | 2 x 4 blocks       | A "h1"
// (A h0 = rows r % 64 < 32, h1 the rest; B h0 = rows 0-63 and 112-175, h1 = rows 64-111,
// 176-223 and 224-255: the next tile's rows, staged so every wave DMAs 2 pieces per region,
// never read.) Every LOAD segment retires its ds_reads (lgkmcnt(0)) before its barrier, so a
// region is restaged in the phase after its last reading phase — after group 1's read too.
// Phase 3 waits (counted vmcnt: T+2's 8 DMAs stay in flight) for every DMA of T+1, retired
// for all readers by the barrier closing the segment. SiLU pairs are 16-column blocks (2p,
// 2p+1); the pair (6, 7) straddles the two waves of a row band and meets through LDS.
template <int EPI>
__global__ void __launch_bounds__(512) gemm8p224_kernel(
    const u16* __restrict__ A, int lda, const u16* __restrict__ W, int ldw,
    void* __restrict__ C, int ldc, int M, int N, int K, int k_split_len,
    const u16* __restrict__ bias, float* __restrict__ ws, const int* __restrict__ group_off) {
  constexpr int BM = 256, BN = 224;
  constexpr int A_BYTES = BM * BK * 2, BUF = 2 * A_BYTES;     // A 256 rows + B image 256 rows
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const BlockCoord bc = block_coord<BM, BN, 4>(W, ldw, M, N, K, k_split_len, group_off);
  const int row0 = bc.row0, Mg = bc.Mg, m0 = bc.m0, n0 = bc.n0, nk = bc.nk;
  const u16* Wg = bc.Wg;
  if (m0 >= Mg) return;
  const u16* Ab = A + (long)row0 * lda;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wid >> 2, w4 = wid & 3, wm = w4 >> 1, wn = w4 & 1;

  // ---- LDS-DMA regions, 16 pieces each (wave wid takes pieces wid and wid + 8): A h0
  // piece q -> rows 64 (q >> 2) + 8 (q & 3), A h1 -> the same + 32; B h0 piece q -> rows 8q
  // (q < 8) or 112 + 8 (q - 8); B h1 piece q -> rows 64 + 8q (q < 6), 176 + 8 (q - 6)
  // (q < 12), 224 + 8 (q - 12).
  auto piece_row = [](int region, int q) {
    switch (region) {
      case 0: return 64 * (q >> 2) + 8 * (q & 3);
      case 1: return 64 * (q >> 2) + 8 * (q & 3) + 32;
      case 2: return q < 8 ? 8 * q : 112 + 8 * (q - 8);
      default: return q < 6 ? 64 + 8 * q : (q < 12 ? 176 + 8 * (q - 6) : 224 + 8 * (q - 12));
    }
  };
  Piece pc[4][2];                                  // [region: A h0, A h1, B h0, B h1][piece]
#pragma unroll
  for (int rg = 0; rg < 4; ++rg)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      pc[rg][i] = make_piece(rg < 2, piece_row(rg, wid + 8 * i), lane, bc, lda, N, ldw, A_BYTES);
  auto dma = [&](auto RG, int kt) {
    constexpr int rg = decltype(RG)::value;
    dma_region(rg < 2 ? Ab : Wg, pc[rg], smem + (kt & 1) * BUF, kt);
  };
  auto dma_all = [&](int kt) {
    dma(std::integral_constant<int, 0>{}, kt); dma(std::integral_constant<int, 1>{}, kt);
    dma(std::integral_constant<int, 2>{}, kt); dma(std::integral_constant<int, 3>{}, kt);
  };

  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc[4][7];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 7; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: K-tiles 0 and 1 whole
  if (nk > 0) dma_all(0);
  if (nk > 1) { dma_all(1); wait_vmcnt<8>(); }
  else wait_vmcnt<0>();
  __syncthreads();
  if (g == 1) {                                    // stagger: group 1 runs one segment behind
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_s_setprio(1);                 // static priority for the younger half
  }
  const int arow = 128 * g + 64 * wm + fr, brow = 112 * wn + fr;
  bf16x8 a0[2][2], a1[2][2], b0[4][2], b1[3][2];
  for (int kt = 0; kt < nk; ++kt) {
    const char* abuf = smem + (kt & 1) * BUF;
    const char* bbuf = abuf + A_BYTES;
    auto phase = [&](auto P) {
      constexpr int p = decltype(P)::value;
      if (p == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) a0[i][kk] = read_frag(abuf, arow + 16 * i, kk, fq);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) b0[j][kk] = read_frag(bbuf, brow + 16 * j, kk, fq);
      } else if (p == 1) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) b1[j][kk] = read_frag(bbuf, brow + 64 + 16 * j, kk, fq);
        if (kt + 2 < nk) { dma(std::integral_constant<int, 0>{}, kt + 2);
                           dma(std::integral_constant<int, 2>{}, kt + 2); }
      } else if (p == 2) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) a1[i][kk] = read_frag(abuf, arow + 32 + 16 * i, kk, fq);
        if (kt + 2 < nk) dma(std::integral_constant<int, 3>{}, kt + 2);
      } else {
        if (kt + 2 < nk) { dma(std::integral_constant<int, 1>{}, kt + 2); wait_vmcnt<8>(); }
        else wait_vmcnt<0>();
      }
      lgkmcnt0();                                  // this segment's reads done
      raw_barrier();
      const bf16x8 (&af)[2][2] = (p < 2) ? a0 : a1;
      constexpr int I0 = (p < 2) ? 0 : 2;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (p == 0 || p == 3) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[I0 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  b0[j][kk], af[i][kk], acc[I0 + i][j], 0, 0, 0);
          } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
              acc[I0 + i][4 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  b1[j][kk], af[i][kk], acc[I0 + i][4 + j], 0, 0, 0);
          }
        }
      raw_barrier();
    };
    phase(std::integral_constant<int, 0>{});
    phase(std::integral_constant<int, 1>{});
    phase(std::integral_constant<int, 2>{});
    phase(std::integral_constant<int, 3>{});
  }
  if (g == 0) __builtin_amdgcn_s_barrier();       // balance group 1's stagger barrier

  // ---- epilogue (transposed accumulators):
  // acc[i][j][r] = C[m0 + 128 g + 64 wm + 16 i + fr][n0 + 112 wn + 16 j + 4 fq + r]
  const int wr0 = m0 + 128 * g + 64 * wm, wc0 = n0 + 112 * wn;
  // the unsplit SiLU*up store stays here (7 blocks per wave: the pairs are not gemm_epilogue's
  // (even, odd) blocks); the slabs and the other epilogues are the shared code
  if constexpr (EPI == EPI_SILU) {
    if (gridDim.y == 1) {
      const bool vec = out_vec<EPI>(C, ldc, N, bias);
      // block 6 of wave wn = 0 (gate) pairs with block 0 of wave wn = 1 (up): through LDS
      __syncthreads();                               // every wave is past its last LDS read
      float* xch = reinterpret_cast<float*>(smem) + (2 * g + wm) * 1024;   // 64 x 16 fp32
      if (wn == 1) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          *reinterpret_cast<f32x4*>(xch + (16 * i + fr) * 16 + 4 * fq) = acc[i][0];
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wr0 + 16 * i + fr;
        if (row >= Mg) continue;
        // own pairs: wave 0 blocks (0,1) (2,3) (4,5) + (6, partner's 0); wave 1 (1,2) (3,4)
        // (5,6) (compile-time block indices in each branch: no runtime-indexed registers)
        if (wn == 0) {
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const int gcol = wc0 + 32 * q;
            if (gcol < N)
              store_silu_quad(C, ldc, row0 + row, (gcol >> 5) * 16 + 4 * fq, acc[i][2 * q],
                              acc[i][2 * q + 1], vec);
          }
          const int gcol = wc0 + 16 * 6;
          if (gcol < N) {
            const f32x4 up = *reinterpret_cast<const f32x4*>(xch + (16 * i + fr) * 16 + 4 * fq);
            store_silu_quad(C, ldc, row0 + row, (gcol >> 5) * 16 + 4 * fq, acc[i][6], up, vec);
          }
        } else {
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const int gcol = wc0 + 16 + 32 * q;
            if (gcol < N)
              store_silu_quad(C, ldc, row0 + row, (gcol >> 5) * 16 + 4 * fq, acc[i][2 * q + 1],
                              acc[i][2 * q + 2], vec);
          }
        }
      }
      return;
    }
  }
  gemm_epilogue<EPI, 4, 7>(acc, wr0, wc0, bc, C, ldc, M, N, bias, ws, fr, fq);
}

// ---------------------------------------------------------------------------------------
// 256x128 ping-pong GEMM: the 8-phase schedule of gemm8p224_kernel for 128-column N-tiles.
// Where 256-column tiles leave most of the chip idle or need deep K splits: the Mixtral
// grouped down projection (N = 4096, one 256-row tile per expert: 8 x 16 = 128 workgroups of
// 256x256 / 152 of 256x224, here 8 x 32 = 256), and the dense N = 4096 projections at
// M = 512 (64 tiles: split-K 4 fills 256 CUs with half the fp32 slab bytes of 32 tiles x 8).
//
// Waves: group g = wid >> 2 = the tile's 128-row half (one wave of each group per SIMD,
// group 1 one barrier behind); wave (wm, wn) = (w4 >> 1, w4 & 1) of a group owns rows
// 128 g + 64 wm .. +63 and columns 64 wn .. +63: 4 x 4 MFMA blocks.
//   phase | reads                              | MFMAs             | DMA for T+2
//   0     | A rows +0..31 (both kk), B +0..31  | rows 0-31, cols 0-31   | -
//   1     | B +32..63                          | rows 0-31, cols 32-63  | A h0
//   2     | A rows +32..63                     | rows 32-63, cols 32-63 | B
//   3     | -                                  | rows 32-63, cols 0-31  | A h1, then a counted
//                                                                         wait for T+1's DMAs
// (A h0 = rows r % 64 < 32, h1 the rest; B = all 128 rows, last read in phase 1.) LDS:
// 2 x (A 256 x 64 + B 128 x 64) bf16 = 96 KiB. SiLU pairs (2p, 2p+1) stay inside a wave.
template <int EPI>
__global__ void __launch_bounds__(512) gemm8p128_kernel(
    const u16* __restrict__ A, int lda, const u16* __restrict__ W, int ldw,
    void* __restrict__ C, int ldc, int M, int N, int K, int k_split_len,
    const u16* __restrict__ bias, float* __restrict__ ws, const int* __restrict__ group_off) {
  constexpr int BM = 256, BN = 128;
  constexpr int A_BYTES = BM * BK * 2, BUF = A_BYTES + BN * BK * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const BlockCoord bc = block_coord<BM, BN, 4>(W, ldw, M, N, K, k_split_len, group_off);
  const int row0 = bc.row0, Mg = bc.Mg, m0 = bc.m0, n0 = bc.n0, nk = bc.nk;
  const u16* Wg = bc.Wg;
  if (m0 >= Mg) return;
  const u16* Ab = A + (long)row0 * lda;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wid >> 2, w4 = wid & 3, wm = w4 >> 1, wn = w4 & 1;

  // ---- LDS-DMA regions, 16 pieces each (wave wid takes pieces wid and wid + 8): A h0
  // piece q -> rows 64 (q >> 2) + 8 (q & 3), A h1 -> the same + 32, B piece q -> rows 8 q.
  auto piece_row = [](int region, int q) {
    switch (region) {
      case 0: return 64 * (q >> 2) + 8 * (q & 3);
      case 1: return 64 * (q >> 2) + 8 * (q & 3) + 32;
      default: return 8 * q;
    }
  };
  Piece pc[3][2];                                  // [region: A h0, A h1, B][piece]
#pragma unroll
  for (int rg = 0; rg < 3; ++rg)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      pc[rg][i] = make_piece(rg < 2, piece_row(rg, wid + 8 * i), lane, bc, lda, N, ldw, A_BYTES);
  auto dma = [&](auto RG, int kt) {
    constexpr int rg = decltype(RG)::value;
    dma_region(rg < 2 ? Ab : Wg, pc[rg], smem + (kt & 1) * BUF, kt);
  };
  auto dma_all = [&](int kt) {
    dma(std::integral_constant<int, 0>{}, kt); dma(std::integral_constant<int, 1>{}, kt);
    dma(std::integral_constant<int, 2>{}, kt);
  };

  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- prologue: K-tiles 0 and 1 whole
  if (nk > 0) dma_all(0);
  if (nk > 1) { dma_all(1); wait_vmcnt<6>(); }
  else wait_vmcnt<0>();
  __syncthreads();
  if (g == 1) {                                    // stagger: group 1 runs one segment behind
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_s_setprio(1);                 // static priority for the younger half
  }
  const int arow = 128 * g + 64 * wm + fr, brow = 64 * wn + fr;
  bf16x8 a0[2][2], a1[2][2], b0[2][2], b1[2][2];
  for (int kt = 0; kt < nk; ++kt) {
    const char* abuf = smem + (kt & 1) * BUF;
    const char* bbuf = abuf + A_BYTES;
    auto phase = [&](auto P) {
      constexpr int p = decltype(P)::value;
      if (p == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) a0[i][kk] = read_frag(abuf, arow + 16 * i, kk, fq);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) b0[j][kk] = read_frag(bbuf, brow + 16 * j, kk, fq);
      } else if (p == 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) b1[j][kk] = read_frag(bbuf, brow + 32 + 16 * j, kk, fq);
        if (kt + 2 < nk) dma(std::integral_constant<int, 0>{}, kt + 2);
      } else if (p == 2) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) a1[i][kk] = read_frag(abuf, arow + 32 + 16 * i, kk, fq);
        if (kt + 2 < nk) dma(std::integral_constant<int, 2>{}, kt + 2);
      } else {
        if (kt + 2 < nk) { dma(std::integral_constant<int, 1>{}, kt + 2); wait_vmcnt<6>(); }
        else wait_vmcnt<0>();
      }
      lgkmcnt0();                                  // this segment's reads done
      raw_barrier();
      const bf16x8 (&af)[2][2] = (p < 2) ? a0 : a1;
      const bf16x8 (&bf)[2][2] = (p == 0 || p == 3) ? b0 : b1;
      constexpr int I0 = (p < 2) ? 0 : 2, J0 = (p == 0 || p == 3) ? 0 : 2;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[I0 + i][J0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                bf[j][kk], af[i][kk], acc[I0 + i][J0 + j], 0, 0, 0);
      raw_barrier();
    };
    phase(std::integral_constant<int, 0>{});
    phase(std::integral_constant<int, 1>{});
    phase(std::integral_constant<int, 2>{});
    phase(std::integral_constant<int, 3>{});
  }
  if (g == 0) __builtin_amdgcn_s_barrier();       // balance group 1's stagger barrier

  // ---- epilogue (transposed accumulators):
  // acc[i][j][r] = C[m0 + 128 g + 64 wm + 16 i + fr][n0 + 64 wn + 16 j + 4 fq + r]
  gemm_epilogue<EPI, 4, 4>(acc, m0 + 128 * g + 64 * wm, n0 + 64 * wn, bc, C, ldc, M, N, bias, ws,
                           fr, fq);
}

// gemm8p_kernel's schedule: grouped tile order, a static priority for waves 4-7 and one
// counted vmcnt per K-tile, each
// measured on MI355X (scripts/bench_gemm8p.py, profiles/r1_gemm8p/, profiles/r2_s2/): grouped
// tile order (+6-14 % on prefill shapes), a static priority for waves 4-7 (+1.5-5 %) over
// per-cluster flips, and one counted vmcnt per K-tile instead of one per phase (+6 % on
// prefill shapes, +6-11 % on the decode gate/up, down and LM head); a deep-prefetch plan
// (per group, an A half and all four W chunks of its parity per K-tile, five load segments
// in flight) and glds-before-ds_read order measured slower / equal, and so (within 1 %,
// profiles/r2_s2/gemm8p_wait/variants.log) did the template's B-before-A read order, an
// lgkmcnt(0) after the barrier and per-cluster priority flips. The code of the rejected
// variants last existed in commit 1acadf7.

// 2 buffers of an A image and a W image (256x224: a 256-row W image)
constexpr size_t LDS_8P = 2 * (size_t)(256 + 256) * BK * 2;
constexpr size_t LDS_8P128 = 2 * (size_t)(256 + 128) * BK * 2;

template <int EPI>
static int dispatch_8p(int tile_cfg, DLI_GEMM_ARGS) {
  switch (tile_cfg) {
    // 256x256 8-phase ping-pong (gemm8p_kernel)
    case 22:
      return launch_gemm<gemm8p_kernel<EPI>, EPI, 256, 256, 512, LDS_8P, 64>(DLI_GEMM_PASS);
    // 256x224 ping-pong (gemm8p224_kernel): N = 28672 gate/up at M = 512 is 256 tiles
    case 26:
      return launch_gemm<gemm8p224_kernel<EPI>, EPI, 256, 224, 512, LDS_8P, 32>(DLI_GEMM_PASS);
    // 256x128 ping-pong (gemm8p128_kernel): Mixtral grouped down (8 x 32 tiles), N = 4096 at
    // M = 512 (64 tiles x split 4)
    case 28:
      return launch_gemm<gemm8p128_kernel<EPI>, EPI, 256, 128, 512, LDS_8P128, 32>(DLI_GEMM_PASS);
    default: return DLI_NOT_MINE;
  }
}

int gemm_8p_dispatch(int epi, int tile_cfg, DLI_GEMM_ARGS) { DLI_EPI_SWITCH_S16(dispatch_8p) }
int gemm_8p_set_slab_store(int mode) { return set_slab_store_tu(mode); }
