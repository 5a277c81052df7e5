// Generic LDS-tiled MFMA GEMM family (family "tiles" of ops/gemm.py's TILE_TABLE, the one
// list of tile ids; dispatch_tiles below is its C++ side): WM x WN waves, BM x BN x 64 block
// tiles, 2 or 3 LDS stages filled by LDS-DMA. Grouped (MoE) launches run on the dense grid
// (row tiles x column tiles, splits, groups) or, given the align step's tile list, on the
// compact grid over the non-empty row tiles (block_coord, gemm_common.h). Split-K writes fp32 slabs for the fused
// consumers (fused_reduce.hip) or reduces them with splitk_reduce_kernel.
#include "gemm_common.h"

template <int BM, int BN, int EPI, int NS, int WM, int WN, int STAG = 0>
__global__ void __launch_bounds__(64 * WM * WN) gemm_bf16_kernel(
    const u16* __restrict__ A, int lda, const u16* __restrict__ W, int ldw,
    void* __restrict__ C, int ldc, int M, int N, int K, int k_split_len,
    const u16* __restrict__ bias, float* __restrict__ ws, const int* __restrict__ group_off,
    const int* __restrict__ tile_list) {
  constexpr int NW = WM * WN;                      // waves: WM along M x WN along N
  constexpr int TM = BM / WM, TN = BN / WN;        // wave tile
  constexpr int MI = TM / 16, NI = TN / 16;        // 16x16 MFMA blocks per wave
  constexpr int A_BYTES = BM * BK * 2, W_BYTES = BN * BK * 2;
  constexpr int BUF = A_BYTES + W_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  // ---- tile coordinates (n-major tile order; grouped with a tile list: the list's items)
  const BlockCoord bc = block_coord<BM, BN, 1>(W, ldw, M, N, K, k_split_len, group_off,
                                               tile_list);
  const int row0 = bc.row0, Mg = bc.Mg, m0 = bc.m0, n0 = bc.n0, kb = bc.kb, nk = bc.nk;
  const u16* Wg = bc.Wg;
  if (m0 >= Mg) return;                             // grouped: empty tile (block-uniform)

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const u16* Ab = A + (long)row0 * lda;
  // grouped SiLU*up with a row index (dli_gemm_grouped_gather passes it as `bias`, which the
  // SiLU epilogue never reads): permuted row p of the group reads activation row arow[p], so
  // the MoE gate/up projection streams the token rows in place (no gathered copy)
  const int* arow = (EPI == EPI_SILU && group_off != nullptr)
                        ? reinterpret_cast<const int*>(bias) : nullptr;

  // ---- per-lane glds source pointers (row clamped in range; swizzled chunk)
  // one glds wave-instruction stages 8 rows x 128 B; all NW waves share each tile
  constexpr int A_INSTR = BM / (8 * NW), W_INSTR = BN / (8 * NW);
  static_assert(A_INSTR * 8 * NW == BM && W_INSTR * 8 * NW == BN, "tile vs waves");
  const u16* a_src[A_INSTR];
  const u16* w_src[W_INSTR];
#pragma unroll
  for (int i = 0; i < A_INSTR; ++i) {
    const int r = (i * NW + wid) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    const int gr = min(m0 + r, Mg - 1);
    a_src[i] = (arow != nullptr ? A + (long)arow[row0 + gr] * lda : Ab + (long)gr * lda) + kb +
               c * 8;
  }
#pragma unroll
  for (int i = 0; i < W_INSTR; ++i) {
    const int r = (i * NW + wid) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((r >> 1) & 7);
    const int gr = min(n0 + r, N - 1);
    w_src[i] = Wg + (long)gr * ldw + kb + c * 8;
  }
  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * BUF;
#pragma unroll
    for (int i = 0; i < A_INSTR; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void*)(a_src[i] + kt * BK),
                                       (lds_void*)(base + (i * NW + wid) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < W_INSTR; ++i)
      __builtin_amdgcn_global_load_lds((gbl_void*)(w_src[i] + kt * BK),
                                       (lds_void*)(base + A_BYTES + (i * NW + wid) * 1024), 16,
                                       0, 0);
  };

  f32x4 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per-lane fragment read offsets (bytes, within a buffer), chunk XOR applied per k-step
  const int fr = lane & 15, fq = lane >> 4;
  int a_row[MI], w_row[NI];
#pragma unroll
  for (int i = 0; i < MI; ++i) a_row[i] = wm * TM + i * 16 + fr;
#pragma unroll
  for (int j = 0; j < NI; ++j) w_row[j] = wn * TN + j * 16 + fr;

  // every fragment of K half kk of the K-tile in buffer buf
  auto read_frags = [&](int buf, int kk, bf16x8 (&af)[MI], bf16x8 (&bfr)[NI]) {
    const char* abuf = smem + buf * BUF;
    const char* wbuf = abuf + A_BYTES;
#pragma unroll
    for (int i = 0; i < MI; ++i) af[i] = read_frag(abuf, a_row[i], kk, fq);
#pragma unroll
    for (int j = 0; j < NI; ++j) bfr[j] = read_frag(wbuf, w_row[j], kk, fq);
  };
  auto mfmas = [&](const bf16x8 (&af)[MI], const bf16x8 (&bfr)[NI]) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
      for (int j = 0; j < NI; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
  };
  auto compute = [&](int buf) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[MI], bfr[NI];
      read_frags(buf, kk, af, bfr);
      mfmas(af, bfr);
    }
  };

  if constexpr (STAG != 0) {
    // Staggered two-group schedule for the 2 x 4-wave, 3-stage tiles (MI355X_MICROARCH.md
    // 'Two waves per SIMD' item 9; the stagger of gemm8p_kernel). The lockstep loop below
    // sends all eight waves into their ds_read burst, their MFMAs and the barrier together,
    // so no MFMA issues under the reads. Here group g = wid >> 2 (= wm, the wave's 64-row
    // half; waves w and w + 4 share a SIMD) splits every K-step into a LOAD and a MATRIX
    // segment closed by raw s_barriers, and group 1 runs one segment behind group 0: on
    // every SIMD one wave is in MATRIX while its partner is in LOAD.
    //
    //   segment s | group 0                  | group 1
    //   2T        | LOAD(T)                  | MATRIX(T-1)
    //   2T + 1    | MATRIX(T)                | LOAD(T)
    //
    //   LOAD(T):   ds_read_b128 of every fragment of K-tile T (both kk halves) from buffer
    //              T % 3; the wave's share of the LDS-DMA of K-tile T+2 into buffer
    //              (T+2) % 3; vmcnt(INSTR) (K-tile T+1 retired, T+2 stays in flight; vmcnt(0)
    //              in the tail, where nothing was issued); lgkmcnt(0); barrier
    //   MATRIX(T): the K-tile's MI x NI x 2 MFMAs (kk 0 then 1: the lockstep order per
    //              accumulator, so the results are bit-identical); barrier
    //
    //   buffer (T+2) % 3 = (T-1) % 3: last ds_read in LOAD(T-1) = segments 2T-2 (group 0) and
    //     2T-1 (group 1), each with lgkmcnt(0) before its closing barrier; restaged in
    //     segments 2T (group 0) and 2T+1 (group 1): one segment after the last read (WAR).
    //   K-tile T+1: issued in LOAD(T-1) (or the prologue), retired by group 0's vmcnt in
    //     segment 2T and by group 1's in segment 2T+1, each before the segment's closing
    //     barrier; first read in segment 2T+2 (group 0), after the barrier that closes 2T+1 —
    //     one barrier more than one group alone would need (RAW).
    //   prologue: K-tiles 0 and 1 issued, vmcnt(INSTR) retires K-tile 0 (vmcnt(0) if nk = 1),
    //     barrier; group 1 then waits one more barrier (segment 0), group 0 one after the
    //     loop, so every wave passes 2 nk + 2 barriers.
    static_assert(WM == 2 && WN == 4 && NS == 3, "staggered schedule: 2 x 4 waves, 3 stages");
    constexpr int INSTR = A_INSTR + W_INSTR;
    const int g = __builtin_amdgcn_readfirstlane(wid) >> 2;
    if (nk > 0) stage(0, 0);
    if (nk > 1) { stage(1, 1); wait_vmcnt<INSTR>(); }
    else wait_vmcnt<0>();
    raw_barrier();
    if (g == 1) {                                    // stagger: group 1 runs one segment behind
      raw_barrier();
      __builtin_amdgcn_s_setprio(1);                 // static priority for the younger half
    }
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
      // ---- LOAD
      bf16x8 af[2][MI], bfr[2][NI];
      read_frags(cur, 0, af[0], bfr[0]);
      read_frags(cur, 1, af[1], bfr[1]);
      if (kt + 2 < nk) {
        int nb = cur + 2;
        if (nb >= NS) nb -= NS;
        stage(nb, kt + 2);
        wait_vmcnt<INSTR>();
      } else {
        wait_vmcnt<0>();
      }
      lgkmcnt0();                                    // this segment's reads done
      raw_barrier();
      // ---- MATRIX
      mfmas(af[0], bfr[0]);
      mfmas(af[1], bfr[1]);
      raw_barrier();
      cur = (cur + 1 == NS) ? 0 : cur + 1;
    }
    if (g == 0) raw_barrier();                       // balance group 1's stagger barrier
  } else if (NS == 2) {
    // 2 LDS buffers: the next tile's DMA overlaps this tile's MFMAs; drained every K-step
    if (nk > 0) stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
      compute(cur);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  } else {
    // NS >= 3 LDS buffers, NS - 2 tiles kept in flight ACROSS the barrier
    // (cdna_hip_programming.md §5 'Pipelining across barriers'): a counted vmcnt retires
    // tile kt only (the tiles issued after it stay in flight), then a raw s_barrier (a
    // __syncthreads() would emit vmcnt(0) and drain the DMA); the restaged buffer
    // (kt + NS - 1) % NS was last read in iteration kt - 1, which every wave has finished.
    // Deeper rings (NS 4-6 on the 128x64 / 128x96 / 128x128 / 128x192 decode tiles) were
    // measured and not kept: equal or slower at M = 512 (profiles/r3/deep_ring/).
    constexpr int INSTR = A_INSTR + W_INSTR;
#pragma unroll
    for (int s = 0; s < NS - 1; ++s)
      if (s < nk) stage(s, s);
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
      const int ahead = min(nk - 1 - kt, NS - 2);     // tiles issued after kt (uniform)
      wait_ahead<INSTR, NS - 2>(ahead);
      lgkmcnt0();
      __builtin_amdgcn_s_barrier();
      if (kt + NS - 1 < nk) {
        int nb = cur + NS - 1;
        if (nb >= NS) nb -= NS;
        stage(nb, kt + NS - 1);
      }
      compute(cur);
      cur = (cur + 1 == NS) ? 0 : cur + 1;
    }
    wait_vmcnt<0>();
  }

  // ---- epilogue (transposed accumulators):
  // acc[i][j][r] = C[m0 + wm*TM + 16i + fr][n0 + wn*TN + 16j + 4fq + r]
  // The text of gemm_epilogue (gemm_common.h), kept inline: through the shared function hipcc
  // allocated this kernel's registers differently (up to +12 / -16 VGPRs over 117
  // instantiations, profiles/r8/README.md)
  const bool split = gridDim.y > 1;
  if (split) {
    float* slab = ws + (long)bc.ks * M * N;
    const int sm = g_slab_store;
    const bool vec = (N & 3) == 0;
    const int col0 = n0 + wn * TN;
    if (EPI == EPI_SLAB16) {
      const bool wide = slab_wide(N, ws);
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = m0 + wm * TM + 16 * i + fr;
        slab_row16<NI>(slab + (long)(row0 + row) * N + col0, acc[i], row < Mg, N - col0, ws, vec,
                       wide, fq);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = m0 + wm * TM + 16 * i + fr;
      if (row >= Mg) continue;
      float* srow = slab + (long)(row0 + row) * N;
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int col = col0 + 16 * j + 4 * fq;
        if (col >= N) continue;
        slab_quad(srow + col, acc[i][j], sm, vec, N - col, ws);
      }
    }
    return;
  }
  const bool vec = out_vec<EPI>(C, ldc, N, bias);
  const bool wide = out_wide<EPI>(C, ldc, N, bias);
  if (EPI == EPI_SILU) {
    // column blocks j (even) = gate, j+1 = up of the same 16 features
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = m0 + wm * TM + 16 * i + fr;
      if (row >= Mg) continue;
#pragma unroll
      for (int j = 0; j < NI; j += 2) {
        const int gcol = n0 + wn * TN + 16 * j;         // first gate row of the pair
        if (gcol < N)
          store_silu_quad(C, ldc, row0 + row, (gcol >> 5) * 16 + 4 * fq, acc[i][j],
                          acc[i][j + 1], vec);
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int row = m0 + wm * TM + 16 * i + fr;
    store_row<EPI, NI>(C, ldc, row0 + row, n0 + wn * TN, N, acc[i], bias, row < Mg, vec, wide,
                       fq);
  }
}

template <int BM, int BN, int EPI, int NS, int WM = 2, int WN = 2, int STAG = 0>
static int launch_cfg(DLI_GEMM_ARGS) {
  // SiLU*up pairs gate/up blocks inside a wave's column range: a multiple of 32 columns
  return launch_gemm<gemm_bf16_kernel<BM, BN, EPI, NS, WM, WN, STAG>, EPI, BM, BN, 64 * WM * WN,
                     NS * (size_t)(BM + BN) * BK * 2, (BN / WN) % 32 ? 0 : 32, true>(
      DLI_GEMM_PASS);
}

template <int EPI>
static int dispatch_tiles(int tile_cfg, DLI_GEMM_ARGS) {
  switch (tile_cfg) {
#define DLI_CFG(id, bm, bn, ns) \
    case id: return launch_cfg<bm, bn, EPI, ns>(DLI_GEMM_PASS);
    DLI_CFG(0, 64, 64, 2) DLI_CFG(1, 64, 128, 2) DLI_CFG(2, 128, 128, 2) DLI_CFG(3, 128, 256, 2)
    DLI_CFG(4, 256, 128, 2)
    DLI_CFG(5, 64, 64, 3) DLI_CFG(6, 64, 128, 3) DLI_CFG(7, 128, 128, 3) DLI_CFG(8, 128, 256, 3)
    DLI_CFG(9, 256, 128, 3)
    DLI_CFG(10, 192, 128, 2) DLI_CFG(11, 192, 128, 3) DLI_CFG(12, 160, 128, 2)
#define DLI_CFG8(id, bm, bn, ns, wm, wn) \
    case id: return launch_cfg<bm, bn, EPI, ns, wm, wn>(DLI_GEMM_PASS);
    // 8 waves (512 threads): 256-wide tiles halve the L2 re-reads of A/W at M >= 256
    DLI_CFG8(13, 256, 256, 2, 2, 4) DLI_CFG8(14, 256, 128, 2, 4, 2) DLI_CFG8(15, 128, 256, 2, 2, 4)
    DLI_CFG8(16, 256, 128, 3, 4, 2) DLI_CFG8(17, 128, 256, 3, 2, 4)
    // grid-filling shapes for N = 6144 / 4096 at M = 512 (4 x 64 = 256 workgroups)
    DLI_CFG(18, 128, 96, 2) DLI_CFG(19, 128, 96, 3) DLI_CFG(20, 128, 64, 2) DLI_CFG(21, 128, 64, 3)
    // 192-wide tiles: N = 6144 (fused QKV) = 32 column tiles, so M = 512 fills 256 CUs with
    // 4 x 32 x split 2 (128-row) or 2 x 32 x split 4 (256-row) workgroups of 8 waves
    DLI_CFG8(23, 128, 192, 3, 2, 4) DLI_CFG8(24, 128, 192, 2, 2, 4) DLI_CFG8(25, 256, 192, 2, 4, 2)
    // tiles 23 / 17 on the staggered two-group schedule (STAG): same tile, ring and bits
    case 60: return launch_cfg<128, 192, EPI, 3, 2, 4, 1>(DLI_GEMM_PASS);
    case 61: return launch_cfg<128, 256, EPI, 3, 2, 4, 1>(DLI_GEMM_PASS);
#undef DLI_CFG8
#undef DLI_CFG
    default: return DLI_NOT_MINE;
  }
}

int gemm_tiles_dispatch(int epi, int tile_cfg, DLI_GEMM_ARGS) { DLI_EPI_SWITCH_S16(dispatch_tiles) }
int gemm_tiles_set_slab_store(int mode) { return set_slab_store_tu(mode); }
