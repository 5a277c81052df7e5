// The 4-wave 256x256 MFMA GEMM (gemm4w_kernel: one wave per SIMD, 128x128 wave tiles,
// accumulators pinned in the AGPR file), its launcher (instantiated by gemm4w.hip) and the
// pieces its persistent form shares (gemm4wp.hip). Tile ids: ops/gemm.py TILE_TABLE.
#pragma once
#include "gemm_common.h"

// 16-B buffer load of `base` (a range-checked descriptor over `nbytes`: lanes past it read
// zeros) straight into LDS at the wave-uniform `lds` + 16 * lane; voff per lane, soff uniform
__device__ __forceinline__ void buf_lds16(const void* base, int nbytes, char* lds, int voff,
                                          int soff) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, nbytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void*)lds, 16, voff, soff, 0, 0);
}

// fragment f (0..15) of a 32-deep half of a 128x128 wave tile, in the order the MFMAs consume
// them: A0, B0..B7, A1..A7 (arow / wrow: the lane's first A / W row of the wave tile)
__device__ __forceinline__ void read_frag_4w(int f, bf16x8 (&av)[8], bf16x8 (&bv)[8],
                                             const char* pa, const char* pw, int arow, int wrow,
                                             int kk, int fq) {
  if (f >= 1 && f <= 8) {
    bv[f - 1] = read_frag(pw, wrow + 16 * (f - 1), kk, fq);
  } else {
    const int ia = f == 0 ? 0 : f - 8;
    av[ia] = read_frag(pa, arow + 16 * ia, kk, fq);
  }
}

// accumulators leave the AGPR file by one pinned copy each, ahead of any row / column
// condition (an AGPR value read inside a divergent branch made hipcc move the whole
// accumulator set through VGPRs in the K loop)
__device__ __forceinline__ f32x4 vget(const f32x4& a) {
  f32x4 v;
  asm volatile("" : "=v"(v) : "0"(a));
  return v;
}

// the unsplit epilogue of a 128x128 wave tile of pinned accumulators:
// acc[I][J][r] = C[row0 + wr0 + 16I + fr][wc0 + 16J + 4fq + r], rows wr0 + .. < Mg.
// Not gemm_epilogue: every accumulator must leave the AGPRs through vget, and there is no
// register room for the 16-B stores or the slab probe modes.
template <int EPI>
__device__ __forceinline__ void store_out_4w(const f32x4 (&acc)[8][8], int wr0, int wc0, int row0,
                                             int Mg, void* C, int ldc, int N, const u16* bias,
                                             int fr, int fq) {
  const bool vec = out_vec<EPI>(C, ldc, N, bias);
  if (EPI == EPI_SILU) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = wr0 + 16 * i + fr;
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const f32x4 g = vget(acc[i][j]), u = vget(acc[i][j + 1]);
        const int gcol = wc0 + 16 * j;
        if (row < Mg && gcol < N)
          store_silu_quad(C, ldc, row0 + row, (gcol >> 5) * 16 + 4 * fq, g, u, vec);
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = wr0 + 16 * i + fr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f32x4 v = vget(acc[i][j]);
      const int col = wc0 + 16 * j + 4 * fq;
      if (row < Mg && col < N) store_quad<EPI>(C, ldc, row0 + row, col, N, v, bias, vec);
    }
  }
}

// ---------------------------------------------------------------------------------------
// 256x256 GEMM with ONE wave per SIMD and 128x128 wave tiles ("4-wave"): the structure of
// the library kernels the prefill projections used to fall back to (hipBLASLt's
// MT256x256x64 solution for these shapes is 4 waves, MIWaveTile 16x4, 1 workgroup per CU).
// Against the 8-wave ping-pong (gemm8p_kernel: 128x64 per wave, two waves per SIMD) a
// 128x128 wave tile reads 1/3 fewer LDS bytes per MFMA (32 ds_read_b128 per 128 MFMAs per
// K-tile instead of 24 per 64) and issues half the barrier traffic; on MI355X under DVFS the
// energy per MFMA, not the cycle count, sets the clock the chip holds on random data
// (cdna_hip_programming.md §5.4 rule 28), and LDS read bytes are one of the terms.
//
// Waves (wm, wn) = (wid >> 1, wid & 1) own rows 128 wm .. +127 and columns 128 wn .. +127:
// acc[8][8] 16x16 blocks = 256 accumulator registers. LDS: 2 buffers x (A 256x64 + W 256x64)
// bf16 = 128 KiB, the chunk XOR swizzle of gemm_bf16_kernel, staged by LDS-DMA (each wave
// moves 64 rows of A and 64 rows of W per K-tile: 16 x 1 KiB). K-tile T = two 32-deep halves:
//   half 0: ds_read the kk=1 fragments of T (F1) | 64 MFMAs on F0 (kk=0 of T)
//   lgkmcnt(0) + vmcnt(0) (T+1 landed) + s_barrier     <- the only barrier of the K-tile
//   half 1: LDS-DMA T+2 into T's buffer; ds_read F0 = kk=0 of T+1 | 64 MFMAs on F1
// so the fragments a half multiplies were read during the previous half, and the barrier
// never leaves the matrix pipe without queued work beyond its own skew.
// Tile order: grouped, GM = 4 tile-rows per group (as gemm8p_kernel).
// DEEP (tile 41): 3 W stages instead of 2. TWO_B (tile 45, the default 4-wave tile): the
// two-barrier K-tile, ktile2 below; plain ring only.
// Measured and not kept (round 4, profiles/r4/gemm4w/; their code last existed in commit
// 1acadf7): a K loop starting at K-tile t % 8 per workgroup, GM = 8, all 16 next-half reads
// or all 16 LDS-DMA pieces of a K-tile up front, staging through registers, sc1 loads, the
// two-barrier K-tile with later barrier positions or on the deep ring, column-major MFMA
// order, per-piece voffset addressing.
template <int EPI, bool DEEP, bool TWO_B>
__global__ void __launch_bounds__(256, 1) gemm4w_kernel(
    const u16* __restrict__ A, int lda, const u16* __restrict__ W, int ldw,
    void* __restrict__ C, int ldc, int M, int N, int K, int k_split_len,
    const u16* __restrict__ bias, float* __restrict__ ws, const int* __restrict__ group_off) {
  constexpr int BM = 256, BN = 256;
  constexpr int A_BYTES = BM * BK * 2, BUF = 2 * A_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const BlockCoord bc = block_coord<BM, BN, 4>(W, ldw, M, N, K, k_split_len, group_off);
  const int row0 = bc.row0, Mg = bc.Mg, m0 = bc.m0, n0 = bc.n0, kb = bc.kb, nk = bc.nk;
  const u16* Wg = bc.Wg;
  if (m0 >= Mg) return;
  const u16* Ab = A + (long)row0 * lda;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;

  // ---- staging by buffer LDS-DMA: piece i (0..7) of A / W = rows 64 wid + 8 i + lane / 8 of
  // the tile, swizzled chunk (lane & 7) ^ ((row >> 1) & 7) = (lane & 7) ^ ((lane >> 4) + 4 i)
  // & 7: only the parity of i changes the lane's offset, the rest is the scalar soffset
  // i * 8 rows + K-tile. Rows past the matrix read as zeros (buffer range check) instead of
  // needing a clamped address per row, so a lane keeps 4 offset VGPRs, not 16 pointers.
  // (the descriptors are built inside buf_lds16: a lambda capturing an
  // __amdgpu_buffer_rsrc_t made hipcc drop the kernel's host-side handle)
  const u16* a_base = Ab + (long)m0 * lda;
  const u16* w_base = Wg + (long)n0 * ldw;
  const int a_bytes = min(Mg - m0, BM) * lda * 2, w_bytes = min(N - n0, BN) * ldw * 2;
  const int prow = 64 * wid + (lane >> 3);
  const int ce = (lane & 7) ^ ((lane >> 4) & 7), co = (lane & 7) ^ (((lane >> 4) + 4) & 7);
  const int a_off[2] = {prow * lda * 2 + (kb + ce * 8) * 2, prow * lda * 2 + (kb + co * 8) * 2};
  const int w_off[2] = {prow * ldw * 2 + (kb + ce * 8) * 2, prow * ldw * 2 + (kb + co * 8) * 2};
  // LDS: 2 stages of {A 256x64, W 256x64} (128 KiB); DEEP: 2 A stages and 3 W stages
  // (160 KiB, the whole LDS): the weight panel, which a decode-sized GEMM streams from HBM
  // while A is L2-resident, is fetched one K-tile further ahead (a CU's stream rate is its
  // bytes in flight over the loaded memory latency)
  auto abase = [&](int kt) -> char* {
    return DEEP ? smem + (kt & 1) * A_BYTES : smem + (kt & 1) * BUF;
  };
  auto wbase = [&](int kt, int ws) -> char* {      // ws = kt % 3 (DEEP)
    return DEEP ? smem + 2 * A_BYTES + ws * A_BYTES : smem + (kt & 1) * BUF + A_BYTES;
  };
  // one 1-KiB piece f (0..15: A pieces 0-7 of K-tile ka, W pieces 8-15 of K-tile kw into W
  // slot ws); a negative K-tile skips its pieces
  auto stage_piece = [&](int ka, int kw, int ws, int f) {
    const int i = f & 7;
    if (f < 8) {
      if (ka >= 0)
        buf_lds16(a_base, a_bytes, abase(ka) + (64 * wid + 8 * i) * 128, a_off[i & 1],
                  i * 16 * lda + ka * (BK * 2));
    } else if (kw >= 0) {
      buf_lds16(w_base, w_bytes, wbase(kw, ws) + (64 * wid + 8 * i) * 128, w_off[i & 1],
                i * 16 * ldw + kw * (BK * 2));
    }
  };
  auto stage = [&](int ka, int kw, int ws) {
#pragma unroll
    for (int f = 0; f < 16; ++f) stage_piece(ka, kw, ws, f);
  };

  const int fr = lane & 15, fq = lane >> 4;
  const int arow = wm * 128 + fr, wrow = wn * 128 + fr;

  f32x4 acc[8][8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // one 32-deep half: 64 MFMAs on (acur, bcur) while the next half's 16 fragments are read
  // from (na, nw) into (anext, bnext). The MFMAs are inline asm with the accumulator pinned to
  // the AGPR file ("+a"): with 256 accumulators per lane the compiler's own MFMA selection
  // bounced them between VGPRs and AGPRs (1,000+ v_accvgpr moves per K-tile). hipcc pads no
  // hazard inside an asm statement (cdna_hip_programming.md §5.7): the fragments come from
  // ds_reads, whose completion hipcc waits for by register (lgkmcnt) before each statement;
  // an accumulator is read only as the next MFMA's C (no wait states) until the drain after
  // the loop. ka / kw >= 0: this half also stages those K-tiles, one LDS-DMA piece after
  // every 4th MFMA (16 pieces issued back to back held the matrix pipe for several hundred
  // cycles: an LDS-DMA issue costs ~60 cycles among MFMAs, /opt/skills/guides/MI355X_MICROARCH.md constants).
  auto half = [&](const bf16x8 (&acur)[8], const bf16x8 (&bcur)[8], bf16x8 (&anext)[8],
                  bf16x8 (&bnext)[8], const char* na, const char* nw, int nkk, bool more,
                  int ka, int kw, int ws) __attribute__((always_inline)) {
    const bool dma = ka >= 0 || kw >= 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0"
                     : "+a"(acc[i][j]) : "v"(bcur[j]), "v"(acur[i]));
        const int q = 8 * i + j;
        if (dma && (q & 3) == 1) {
          stage_piece(ka, kw, ws, q >> 2);
          __builtin_amdgcn_sched_barrier(0);
        }
        // one next-half fragment read after every 4th MFMA, pinned in place (the scheduler
        // hoisted all 16 above the first MFMA, whose lgkmcnt then waited on 2 of them), in
        // the order the next half consumes them: A0, B0..B7, A1..A7
        if (more && (q & 3) == 3) {
          read_frag_4w(q >> 2, anext, bnext, na, nw, arow, wrow, nkk, fq);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
  };

  // ---- prologue. Plain: K-tiles 0 and 1 in flight. DEEP: A 0-1 and W 0-2 (issue order A0 W0
  // A1 W1 W2). Then the kk=0 fragments of K-tile 0 in registers.
  if (nk > 0) stage(0, 0, 0);
  if (nk > 1) stage(1, 1, 1);
  if (DEEP && nk > 2) stage(-1, 2, 2);
  if (DEEP && nk > 2) wait_vmcnt<24>();
  else if (nk > 1) wait_vmcnt<16>();
  else wait_vmcnt<0>();
  raw_barrier();
  bf16x8 a0[8], b0[8], a1[8], b1[8];
  if (nk > 0) {
    a0[0] = read_frag(abase(0), arow, 0, fq);
#pragma unroll
    for (int j = 0; j < 8; ++j) b0[j] = read_frag(wbase(0, 0), wrow + 16 * j, 0, fq);
#pragma unroll
    for (int i = 1; i < 8; ++i) a0[i] = read_frag(abase(0), arow + 16 * i, 0, fq);
  }

  // one K-tile of the one-barrier schedule; SA / SW (compile-time, so no branch sits inside
  // an MFMA sequence): restage A (K-tile kt + 2) / W (kt + 2, DEEP: kt + 3) during its second
  // half
  int wsl = 0;                                      // W slot of kt (DEEP: kt % 3)
  auto ktile = [&](auto SA, auto SW, int kt) __attribute__((always_inline)) {
    constexpr bool sa = decltype(SA)::value, sw = decltype(SW)::value;
    const int ws1 = wsl == 2 ? 0 : wsl + 1;
    const char* ab = abase(kt);
    const char* wb = wbase(kt, wsl);
    // half 0: MFMAs on kk=0 of kt, reading kk=1 of kt
    half(a0, b0, a1, b1, ab, wb, 1, true, -1, -1, 0);
    // every wave's reads of these buffers retired; K-tile kt+1 landed for every wave: the
    // only younger DMAs may be DEEP's W of kt+2 (issued last in the previous K-tile)
    lgkmcnt0();                                    // seen by hipcc's counters
    if (DEEP && kt + 2 < nk) wait_vmcnt<8>();
    else wait_vmcnt<0>();
    raw_barrier();
    // half 1: MFMAs on kk=1 of kt, reading kk=0 of kt+1; restage kt's buffers
    half(a1, b1, a0, b0, abase(kt + 1), wbase(kt + 1, ws1), 0, true, sa ? kt + 2 : -1,
         sw ? kt + (DEEP ? 3 : 2) : -1, wsl);
    wsl = ws1;
  };
  // The two-barrier K-tile (the buffer-release point moved forward): one K-tile = 128
  // MFMAs, 64 on F0 (kk=0, read during the previous K-tile) then 64 on F1:
  //   MFMAs 0-15: one F1(kt) fragment read after each        | frees buffer kt early
  //   after MFMA 19: lgkmcnt(0) + s_barrier (B1: every wave has read buffer kt)
  //   MFMAs 20-95: LDS-DMA of K-tile kt+2 into buffer kt, one piece per 5 MFMAs
  //   after MFMA 103: vmcnt(16) (K-tile kt+1 landed; kt+2 may fly) + s_barrier (B2)
  //   MFMAs 104-119: one F0(kt+1) fragment read after each
  // The DMA of kt+2 starts ~45 MFMAs earlier than in the one-barrier schedule and is waited
  // for ~1.5 K-tiles later (hides ~2,400 cycles of HBM latency instead of ~1,000-2,000),
  // and 16 DMAs spread over 80 MFMAs instead of 64. Plain (2-stage) ring only.
  static_assert(!(TWO_B && DEEP), "two-barrier schedule: plain ring only");
  // STG: this K-tile stages K-tile kt+2; more: a K-tile follows (B2 and the F0 reads)
  auto ktile2 = [&](auto STG, bool more, int kt) __attribute__((always_inline)) {
    constexpr bool stg = decltype(STG)::value;
    const char* ab = abase(kt);
    const char* wb = wbase(kt, 0);
    const char* nab = abase(kt + 1);
    const char* nwb = wbase(kt + 1, 0);
    constexpr int QB1 = 19, QB2 = 103;             // B1 / B2 positions
    auto read_fx = [&](int f, bf16x8 (&av)[8], bf16x8 (&bv)[8], const char* pa, const char* pw,
                       int kk) __attribute__((always_inline)) {
      read_frag_4w(f, av, bv, pa, pw, arow, wrow, kk, fq);
    };
    auto step = [&](int q) __attribute__((always_inline)) {
      if (q < 16) {                                // F1(kt)
        read_fx(q, a1, b1, ab, wb, 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (q == QB1) {
        lgkmcnt0();
        raw_barrier();
      }
      if (stg && q > QB1 && q <= QB1 + 80 && (q - QB1 - 1) % 5 == 0) {
        stage_piece(kt + 2, kt + 2, 0, (q - QB1 - 1) / 5);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (q == QB2 && more) {
        wait_vmcnt<stg ? 16 : 0>();
        raw_barrier();
      }
      if (more && q > QB2 && q <= QB2 + 16) {      // F0(kt+1)
        read_fx(q - QB2 - 1, a0, b0, nab, nwb, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0"
                     : "+a"(acc[i][j]) : "v"(b0[j]), "v"(a0[i]));
        step(8 * i + j);
      }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0"
                     : "+a"(acc[i][j]) : "v"(b1[j]), "v"(a1[i]));
        step(64 + 8 * i + j);
      }
  };

  using T_ = std::integral_constant<bool, true>;
  using F_ = std::integral_constant<bool, false>;
  int kt = 0;
  if (TWO_B) {
    for (; kt + 2 < nk; ++kt) ktile2(T_{}, true, kt);
    for (; kt < nk; ++kt) ktile2(F_{}, kt + 1 < nk, kt);
  } else {
    if (DEEP) {
      for (; kt + 3 < nk; ++kt) ktile(T_{}, T_{}, kt);
      if (kt + 2 < nk) { ktile(T_{}, F_{}, kt); ++kt; }
    } else {
      for (; kt + 2 < nk; ++kt) ktile(T_{}, T_{}, kt);
    }
    if (kt + 1 < nk) { ktile(F_{}, F_{}, kt); ++kt; }
    if (nk > 0) {
      half(a0, b0, a1, b1, abase(kt), wbase(kt, wsl), 1, true, -1, -1, 0);
      half(a1, b1, a0, b0, smem, smem, 0, false, -1, -1, 0);
    }
  }
  // MFMA results -> any other reader: the XDL write-back wait states (§5.7 item 2), tied to
  // the last row of accumulators written so that no copy of them is hoisted above the pad
  asm volatile("s_nop 15\n\ts_nop 15"
               : "+a"(acc[7][0]), "+a"(acc[7][1]), "+a"(acc[7][2]), "+a"(acc[7][3]),
                 "+a"(acc[7][4]), "+a"(acc[7][5]), "+a"(acc[7][6]), "+a"(acc[7][7]));
  // ---- epilogue (transposed accumulators):
  // acc[I][J][r] = C[m0 + 128 wm + 16I + fr][n0 + 128 wn + 16J + 4fq + r]
  const int wr0 = m0 + 128 * wm, wc0 = n0 + 128 * wn;
  if (gridDim.y > 1) {
    float* slab = ws + (long)bc.ks * M * N;
    const int sm = g_slab_store;
    const bool vec = (N & 3) == 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int row = wr0 + 16 * i + fr;
      float* srow = slab + (long)(row0 + min(row, Mg - 1)) * N;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 v = vget(acc[i][j]);
        const int col = wc0 + 16 * j + 4 * fq;
        if (row < Mg && col < N) slab_quad_fp32(srow + col, v, sm & 3, vec, N - col);
      }
    }
    return;
  }
  store_out_4w<EPI>(acc, wr0, wc0, row0, Mg, C, ldc, N, bias, fr, fq);
}

template <int EPI, bool DEEP, bool TWO_B>
static int launch_4w(DLI_GEMM_ARGS) {
  return launch_gemm<gemm4w_kernel<EPI, DEEP, TWO_B>, EPI, 256, 256, 256,
                     (DEEP ? 5 : 4) * (size_t)256 * BK * 2, 32>(DLI_GEMM_PASS);
}
