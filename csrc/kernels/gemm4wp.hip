// Persistent form of the 4-wave two-barrier 256x256 GEMM (tile 55; tile 45 = gemm4w_kernel
// <EPI, false, true> is its one-tile-per-workgroup form). VERDICT r4 item 4: the prefill
// projections pay, per 256x256 tile, a prologue (the first two K-tiles' LDS-DMA latency with
// the matrix pipe idle) and an epilogue (the 128-256 KB store tail) that a workgroup-per-tile
// grid cannot hide. Here one workgroup per CU walks tiles v = blockIdx.x, + gridDim.x, ...
// (the same virtual ids, XCD remap and GM-4 grouped order as tile 45, so the tiles in flight
// at any time are the ones a wave of tile 45's grid would run), and the two DMA windows of a
// tile's LAST two K-tiles — idle in tile 45 — stage K-tiles 0 and 1 of the workgroup's next
// tile. The epilogue's stores then drain while those DMAs fly, and the next tile starts with
// both of its first K-tiles in LDS.
//
// Restrictions (the launcher returns hipErrorInvalidValue and the planner never picks it
// otherwise): no split-K, no grouped (MoE) mode, K a multiple of 128 (an even K-tile count:
// the next tile's K-tiles 0 / 1 land in buffers 0 / 1, which the current tile's last two
// K-tiles have just released).
#include "gemm4w.h"

template <int EPI>
__global__ void __launch_bounds__(256, 1) gemm4wp_kernel(
    const u16* __restrict__ A, int lda, const u16* __restrict__ W, int ldw,
    void* __restrict__ C, int ldc, int M, int N, int K, const u16* __restrict__ bias) {
  constexpr int BM = 256, BN = 256, GM = 4;
  constexpr int A_BYTES = BM * BK * 2, BUF = 2 * A_BYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tiles_m = (M + BM - 1) / BM;
  const int tiles_n = (N + BN - 1) / BN;
  const int nwg = tiles_m * tiles_n;
  const int nk = K / BK;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid >> 1, wn = wid & 1;

  // virtual tile id -> (m0, n0): tile 45's XCD remap + GM-4 grouped order
  auto coords = [&](int v, int& m0, int& n0) {
    tile_origin<BM, BN, GM>(xcd_remap(v, nwg), tiles_m, tiles_n, m0, n0);
  };

  // ---- staging: piece f (0..15) of K-tile kg of the tile whose operand panels start at
  // sa / sw (sab / swb bytes in range: rows past the matrix read as zeros) into buffer buf
  const int prow = 64 * wid + (lane >> 3);
  const int ce = (lane & 7) ^ ((lane >> 4) & 7), co = (lane & 7) ^ (((lane >> 4) + 4) & 7);
  const int a_off[2] = {prow * lda * 2 + ce * 16, prow * lda * 2 + co * 16};
  const int w_off[2] = {prow * ldw * 2 + ce * 16, prow * ldw * 2 + co * 16};
  const u16* sa = A;
  const u16* sw = W;
  int sab = 0, swb = 0;
  auto set_stage = [&](int m0, int n0) {
    sa = A + (long)m0 * lda;
    sw = W + (long)n0 * ldw;
    sab = min(M - m0, BM) * lda * 2;
    swb = min(N - n0, BN) * ldw * 2;
  };
  auto stage_piece = [&](int kg, int buf, int f) {
    const int i = f & 7;
    char* dst = smem + buf * BUF + (f < 8 ? 0 : A_BYTES) + (64 * wid + 8 * i) * 128;
    if (f < 8)
      buf_lds16(sa, sab, dst, a_off[i & 1], i * 16 * lda + kg * (BK * 2));
    else
      buf_lds16(sw, swb, dst, w_off[i & 1], i * 16 * ldw + kg * (BK * 2));
  };

  const int fr = lane & 15, fq = lane >> 4;
  const int arow = wm * 128 + fr, wrow = wn * 128 + fr;
  auto abuf = [&](int kt) -> const char* { return smem + (kt & 1) * BUF; };
  auto wbuf = [&](int kt) -> const char* { return smem + (kt & 1) * BUF + A_BYTES; };

  f32x4 acc[8][8];
  bf16x8 a0[8], b0[8], a1[8], b1[8];
  auto read_f0 = [&](int kt) {       // kk = 0 fragments of K-tile kt (order A0, B0..B7, A1..)
    a0[0] = read_frag(abuf(kt), arow, 0, fq);
#pragma unroll
    for (int j = 0; j < 8; ++j) b0[j] = read_frag(wbuf(kt), wrow + 16 * j, 0, fq);
#pragma unroll
    for (int i = 1; i < 8; ++i) a0[i] = read_frag(abuf(kt), arow + 16 * i, 0, fq);
  };
  auto read_fx = [&](int f, bf16x8 (&av)[8], bf16x8 (&bv)[8], const char* pa, const char* pw,
                     int kk) __attribute__((always_inline)) {
    read_frag_4w(f, av, bv, pa, pw, arow, wrow, kk, fq);
  };

  // one K-tile of the two-barrier schedule (gemm4w.h ktile2): MFMAs 0-15 read F1(kt), B1
  // after MFMA 19, the DMA window (16 pieces over MFMAs 20-95) stages K-tile kg of the
  // staging panels into kt's buffer, B2 after MFMA 103 (vmcnt: the pieces just issued may
  // fly), MFMAs 104-119 read F0(kt+1). STG: this K-tile stages; MORE: a K-tile of the same
  // tile follows (B2 and the F0 reads).
  auto ktile = [&](auto STG, bool more, int kt, int kg) __attribute__((always_inline)) {
    constexpr bool stg = decltype(STG)::value;
    const char* ab = abuf(kt);
    const char* wb = wbuf(kt);
    const char* nab = abuf(kt + 1);
    const char* nwb = wbuf(kt + 1);
    constexpr int QB1 = 19, QB2 = 103;
    auto step = [&](int q) __attribute__((always_inline)) {
      if (q < 16) {
        read_fx(q, a1, b1, ab, wb, 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (q == QB1) {
        lgkmcnt0();
        raw_barrier();
      }
      if (stg && q > QB1 && q <= QB1 + 80 && (q - QB1 - 1) % 5 == 0) {
        stage_piece(kg, kt & 1, (q - QB1 - 1) / 5);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (q == QB2 && more) {
        wait_vmcnt<stg ? 16 : 0>();
        raw_barrier();
      }
      if (more && q > QB2 && q <= QB2 + 16) {
        read_fx(q - QB2 - 1, a0, b0, nab, nwb, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0"
                     : "+a"(acc[u][v]) : "v"(b0[v]), "v"(a0[u]));
        step(8 * u + v);
      }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0"
                     : "+a"(acc[u][v]) : "v"(b1[v]), "v"(a1[u]));
        step(64 + 8 * u + v);
      }
  };
  using T_ = std::integral_constant<bool, true>;
  int v = blockIdx.x;
  if (v >= nwg) return;                              // wave-uniform: every wave exits
  int m0, n0;
  coords(v, m0, n0);
  set_stage(m0, n0);
  // prologue of the first tile: K-tiles 0 and 1 in flight, then F0 of K-tile 0
  stage_piece(0, 0, 0);
#pragma unroll
  for (int f = 1; f < 16; ++f) stage_piece(0, 0, f);
#pragma unroll
  for (int f = 0; f < 16; ++f) stage_piece(1, 1, f);
  wait_vmcnt<16>();
  raw_barrier();

  while (true) {                                     // every wave runs the same tiles
    const int vn = v + (int)gridDim.x;
    const bool has_next = vn < nwg;
    int mn = 0, nn = 0;
    if (has_next) coords(vn, mn, nn);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the zeroed accumulators are read by inline-asm MFMAs, which hipcc pads no hazard for:
    // pin every write ahead of a few wait states (gemm4w.h: nothing copies them in the loop)
#pragma unroll
    for (int i = 0; i < 8; ++i)
      asm volatile("s_nop 3"
                   : "+a"(acc[i][0]), "+a"(acc[i][1]), "+a"(acc[i][2]), "+a"(acc[i][3]),
                     "+a"(acc[i][4]), "+a"(acc[i][5]), "+a"(acc[i][6]), "+a"(acc[i][7]));
    read_f0(0);
    int kt = 0;
    for (; kt + 2 < nk; ++kt) ktile(T_{}, true, kt, kt + 2);
    // the last two K-tiles stage the next tile's K-tiles 0 and 1 (buffers 0 / 1: nk even).
    // Without a next tile they stage through an empty buffer range (no memory traffic, the
    // range check returns zeros): one code path — a branch here doubled the unrolled tail
    // and hipcc spilled the fragments (1 KB/lane of scratch)
    set_stage(mn, nn);
    sab = has_next ? sab : 0;
    swb = has_next ? swb : 0;
    ktile(T_{}, true, kt, 0);
    ktile(T_{}, false, kt + 1, 1);
    // MFMA results -> the epilogue's copies: XDL write-back wait states (gemm4w.h)
    asm volatile("s_nop 15\n\ts_nop 15"
                 : "+a"(acc[7][0]), "+a"(acc[7][1]), "+a"(acc[7][2]), "+a"(acc[7][3]),
                   "+a"(acc[7][4]), "+a"(acc[7][5]), "+a"(acc[7][6]), "+a"(acc[7][7]));
    // ---- epilogue of tile (m0, n0), transposed accumulators:
    // acc[I][J][r] = C[m0 + 128 wm + 16I + fr][n0 + 128 wn + 16J + 4fq + r]
    const int wr0 = m0 + 128 * wm, wc0 = n0 + 128 * wn;
    store_out_4w<EPI>(acc, wr0, wc0, 0, M, C, ldc, N, bias, fr, fq);
    // the next tile's K-tiles 0 and 1 (issued in the last two K-tiles) landed for every wave
    // (also before exiting: no LDS-DMA outlives the workgroup)
    wait_vmcnt<0>();
    if (!has_next) break;
    raw_barrier();
    v = vn;
    m0 = mn;
    n0 = nn;
  }
}

template <int EPI>
static int launch_4wp(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M,
                      int N, int K, int splits, const void* bias, const int* group_off,
                      hipStream_t st) {
  if (splits != 1 || group_off != nullptr || K % (2 * BK) || C == nullptr ||
      (EPI == EPI_SILU && N % 32))
    return (int)hipErrorInvalidValue;
  constexpr size_t lds = 4 * (size_t)256 * BK * 2;
  static int cus = 0;
  if (!cus) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (cus <= 0) cus = 256;
    const hipError_t e = hipFuncSetAttribute((const void*)gemm4wp_kernel<EPI>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { cus = 0; return (int)e; }
  }
  const int tiles = ((M + 255) / 256) * ((N + 255) / 256);
  // one workgroup per CU (128 KiB of LDS each); a multiple of 8 keeps every workgroup's
  // virtual tile ids on one XCD residue class, as tile 45's grid places them
  int grid = tiles < cus ? tiles : (cus / 8) * 8;
  if (grid < 1) grid = 1;
  gemm4wp_kernel<EPI><<<grid, 256, lds, st>>>((const u16*)A, lda, (const u16*)W, ldw, C, ldc,
                                              M, N, K, (const u16*)bias);
  DLI_RETURN_LAUNCH();
}

template <int EPI>
static int dispatch_4wp(int tile_cfg, DLI_GEMM_ARGS) {
  (void)ws;
  (void)groups;
  if (tile_cfg != 55) return DLI_NOT_MINE;
  return launch_4wp<EPI>(A, lda, W, ldw, C, ldc, M, N, K, splits, bias, go, st);
}

int gemm_4wp_dispatch(int epi, int tile_cfg, DLI_GEMM_ARGS) { DLI_EPI_SWITCH(dispatch_4wp) }
