// Shared pieces of the bf16 MFMA GEMM families (gemm_tiles.hip, gemm8p.hip, gemm4w.hip,
// gemv.hip; dispatched by gemm.hip's dli_gemm): epilogue stores, split-K slab stores, the
// waitcnt / barrier / fragment helpers, the block -> tile mapping, the shared epilogue, the
// split-K reduce kernel and the launcher.
// Every kernel computes C[M,N] = A[M,K] . W[N,K]^T with the W fragment as MFMA operand A
// (transposed accumulators, see below). Static / inline only: each family is its own
// translation unit.
#pragma once
#include "common.h"
#include <type_traits>


#define BK 64

enum { EPI_BF16 = 0, EPI_F32 = 1, EPI_SILU = 2, EPI_BIAS_GELU = 3, EPI_BIAS = 4,
       // slab-only split-K call (C == nullptr, splits > 1) whose partials are stored as fp16
       // scaled by 1/16 instead of fp32 (half the bytes the GEMM writes and its consumer
       // reads; the scale keeps |partial| up to ~1e6 in range). Tiles and 8-phase families.
       EPI_SLAB16 = 5 };

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

__device__ __forceinline__ float silu_f(float x) { return x / (1.f + __expf(-x)); }
// tanh-approximate GELU, branch-free: 0.5 (1 + tanh(y)) = sigmoid(2 y). tanhf's range
// branches made a 256-accumulator epilogue too large to unroll, and the rolled loop indexed
// the accumulators dynamically: hipcc demoted them to scratch and copied them out of the
// AGPRs inside the K loop, where no hazard padding follows an inline-asm MFMA
__device__ __forceinline__ float gelu_f(float x) {
  const float y2 = 1.5957691216057308f * (x + 0.044715f * x * x * x);
  return x / (1.f + __expf(-y2));
}

template <int EPI>
__device__ __forceinline__ void store_pair_or_one(void* C, int ldc, int row, int col, float v,
                                                  const u16* bias) {
  if (EPI == EPI_F32) {
    ((float*)C)[(long)row * ldc + col] = v;
  } else {
    if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) v += bf2f(bias[col]);
    if (EPI == EPI_BIAS_GELU) v = gelu_f(v);
    ((u16*)C)[(long)row * ldc + col] = f2bf(v);
  }
}

// fp32 split-K partial stores: 0 plain (the line stays dirty in the XCD's L2 and is written
// back at the kernel boundary, /opt/skills/guides/MI355X_MICROARCH.md price row 'boundary'), 1 nontemporal,
// 2 sc1 (write-through: the bytes leave L2 while the GEMM still computes), 3 sc0 sc1.
// One copy per translation unit (device code is not relocatable across files, -fno-gpu-rdc):
// every GEMM family sets its own through set_slab_store_tu(), dli_gemm_set_slab_store sets all.
static __device__ int g_slab_store = 0;
static inline int set_slab_store_tu(int mode) {
  int old = 0;
  (void)hipMemcpyFromSymbol(&old, HIP_SYMBOL(g_slab_store), sizeof(int));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_slab_store), &mode, sizeof(int));
  return old;
}
__device__ __forceinline__ void slab_store(float* p, float v, int mode) {
  if (mode == 1) {
    __builtin_nontemporal_store(v, p);
  } else if (mode == 2) {
    asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
  } else if (mode == 3) {
    asm volatile("global_store_dword %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
  } else {
    *p = v;
  }
}

// ---- transposed accumulators. Every MFMA kernel in this file passes the W fragment as MFMA
// operand A and the activation fragment as operand B, i.e. it computes C^T = W . A^T. A
// 16x16 output block then lands as: lane (fq = lane / 16, fr = lane % 16) holds
// C[16 i + fr][16 j + 4 fq + r] for r = 0..3 — four CONSECUTIVE columns of one row — so an
// epilogue writes one 16-B (fp32 slab / logits) or 8-B (bf16) vector per block instead of
// four 4-B / 2-B scalars. The epilogue store tail of a short-K split GEMM is issue-bound
// (cdna_hip_programming.md T21: halving the store instructions at equal bytes halved it);
// the fragments read from LDS, the MFMA count and the slab layout are unchanged.
__device__ __forceinline__ void slab_store4(float* p, f32x4 v, int mode) {
  if (mode == 1) {
    __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p));
  } else if (mode == 2) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
  } else if (mode == 3) {
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1" ::"v"(p), "v"(v) : "memory");
  } else {
    *reinterpret_cast<f32x4*>(p) = v;
  }
}

// the fp32 partial quad (store modes 0-3); the 4-wave family calls it directly (its
// accumulator-pinned epilogue has no register room for the probe modes)
__device__ __forceinline__ void slab_quad_fp32(float* p, f32x4 v, int mode, bool vec, int left) {
  if (vec) {
    slab_store4(p, v, mode);
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < left) slab_store(p + r, v[r], mode);
  }
}

// fp16 (x 1/16) partial quad of the EPI_SLAB16 slab image: p = &fp32-indexed slab[row][col]
// (the element index into a [splits][M][N] image based at ws), one 8-B store
__device__ __forceinline__ void slab_quad16(float* p, f32x4 v, bool vec, int left,
                                            const float* ws) {
  u16* q = (u16*)ws + (p - ws);
  if (vec) {
    uint2 pk;
    pk.x = pack2h(v[0] * SLAB16_SCALE, v[1] * SLAB16_SCALE);
    pk.y = pack2h(v[2] * SLAB16_SCALE, v[3] * SLAB16_SCALE);
    *reinterpret_cast<uint2*>(q) = pk;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < left) q[r] = (u16)(pack2h(v[r] * SLAB16_SCALE, 0.f) & 0xffffu);
  }
}

// one split-K partial quad: p = &slab[row][col]; vec = (N % 4 == 0), so col + 3 < N.
// Probe modes (dli_gemm_set_slab_store): 4 = bf16 partials at the same element index of a
// bf16 [splits][M][N] image based at ws, 5 = no store (timing only: the consumer reads junk)
__device__ __forceinline__ void slab_quad(float* p, f32x4 v, int mode, bool vec, int left,
                                          const float* ws) {
  if (mode == 5) return;
  if (mode == 4) {
    u16* q = (u16*)ws + (p - ws);
    if (vec) {
      uint2 pk;
      pk.x = pack2bf(v[0], v[1]);
      pk.y = pack2bf(v[2], v[3]);
      *reinterpret_cast<uint2*>(q) = pk;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (r < left) q[r] = f2bf(v[r]);
    }
    return;
  }
  slab_quad_fp32(p, v, mode, vec, left);
}

// a quad packed to bf16 with the bias / GELU of the epilogue applied; inb: the quad's columns
// exist (the bias is not read past N)
template <int EPI>
__device__ __forceinline__ uint2 pack_quad(f32x4 v, const u16* bias, int col, bool inb) {
  float o[4] = {v[0], v[1], v[2], v[3]};
  if (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU) {
    uint2 b = uint2{0u, 0u};
    if (inb) b = *reinterpret_cast<const uint2*>(bias + col);
    o[0] += __uint_as_float(b.x << 16); o[1] += __uint_as_float(b.x & 0xffff0000u);
    o[2] += __uint_as_float(b.y << 16); o[3] += __uint_as_float(b.y & 0xffff0000u);
  }
  if (EPI == EPI_BIAS_GELU) {
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = gelu_f(o[r]);
  }
  uint2 pk;
  pk.x = pack2bf(o[0], o[1]);
  pk.y = pack2bf(o[2], o[3]);
  return pk;
}

// four consecutive output columns [col, col + 4) of one row; vec = (N % 4 == 0 && ldc % 4
// == 0): one 16-B (fp32) / 8-B (bf16) store, else per-column stores for the row's tail
template <int EPI>
__device__ __forceinline__ void store_quad(void* C, int ldc, int row, int col, int N, f32x4 v,
                                           const u16* bias, bool vec) {
  if (!vec) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (col + r < N) store_pair_or_one<EPI>(C, ldc, row, col + r, v[r], bias);
    return;
  }
  if (EPI == EPI_F32) {
    *reinterpret_cast<f32x4*>((float*)C + (long)row * ldc + col) = v;
    return;
  }
  *reinterpret_cast<uint2*>((u16*)C + (long)row * ldc + col) = pack_quad<EPI>(v, bias, col, true);
}

// the vector epilogue needs every row start and column quad aligned: N and ldc multiples
// of 4, C (and the bias) 16-B (fp32) / 8-B (bf16) aligned (C may be a column view)
template <int EPI>
__device__ __forceinline__ bool out_vec(const void* C, int ldc, int N, const u16* bias) {
  const uintptr_t mis = ((uintptr_t)C | (uintptr_t)bias) & (EPI == EPI_F32 ? 15 : 7);
  return ((N | ldc) & 3) == 0 && mis == 0;
}

// SiLU(gate) * up of one gate block g and its up block u (same lane, same row): the four
// features [f, f + 4) of the 16-row-interleaved gate/up layout
__device__ __forceinline__ void store_silu_quad(void* C, int ldc, int row, int f, f32x4 g,
                                                f32x4 u, bool vec) {
  float o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = silu_f(g[r]) * u[r];
  u16* p = (u16*)C + (long)row * ldc + f;
  if (vec) {
    uint2 pk;
    pk.x = pack2bf(o[0], o[1]);
    pk.y = pack2bf(o[2], o[3]);
    *reinterpret_cast<uint2*>(p) = pk;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) p[r] = f2bf(o[r]);
  }
}

// ---- 16-B epilogue stores for 2-byte outputs. A lane's packed quad of a 16-column block is
// 8 B (uint2); lane (fr, fq) holds columns 4 fq .. 4 fq + 3 of its row, so a row receives a
// block's 32 bytes from four lanes and the store tail issues one 8-B store per block. For two
// ADJACENT blocks (j, j + 1), v_permlane16_swap_b32 vdst, src swaps the odd 16-lane rows of
// vdst (lanes 16-31, 48-63) with the even rows of src (lanes 0-15, 32-47); with vdst = block
// j's dword and src = block j + 1's dword, once per dword, the lanes then hold
//   fq 0: block j   columns 0-7      fq 1: block j+1 columns 0-7
//   fq 2: block j   columns 8-15     fq 3: block j+1 columns 8-15
// i.e. 8 contiguous columns each: one 16-B store per lane replaces two 8-B stores (half the
// store instructions at equal bytes, 64 contiguous bytes per row; the store tail is
// issue-bound, cdna_hip_programming.md T21). The values are unchanged, only the lane that
// stores them. The swap is a cross-lane operation: EVERY lane of the wave must execute it, so
// the row / column predicates apply to the store alone. An odd block left over, rows or N
// without 16-B alignment and the fp32 outputs keep the 8-B / per-column stores. So does the
// SiLU*up epilogue: pairing two gate/up results into one 16-B store ran the M = 512 gate/up
// GEMM on the 256x256 8-phase tile 2.9 % slower (profiles/r7/README.md).
__device__ __forceinline__ uint4 widen_pair(uint2 a, uint2 b) {
  const auto x = __builtin_amdgcn_permlane16_swap(a.x, b.x, false, false);
  const auto y = __builtin_amdgcn_permlane16_swap(a.y, b.y, false, false);
  return uint4{x[0], y[0], x[1], y[1]};
}
// first of the lane's 8 columns after widen_pair, relative to block j's first column
__device__ __forceinline__ int wide_col(int fq) { return 16 * (fq & 1) + 8 * (fq >> 1); }

// 16-B stores need every row start and 8-column run aligned
__device__ __forceinline__ bool slab_wide(int N, const float* ws) {
  return (N & 7) == 0 && ((uintptr_t)ws & 15) == 0;
}
template <int EPI>
__device__ __forceinline__ bool out_wide(const void* C, int ldc, int N, const u16* bias) {
  if (EPI == EPI_F32 || EPI == EPI_SLAB16 || EPI == EPI_SILU) return false;
  return ((N | ldc) & 7) == 0 && ((uintptr_t)C & 15) == 0 && ((uintptr_t)bias & 7) == 0;
}

// one lane's row of NB adjacent 16-column blocks of the fp16 slab image: p = &slab[row][first
// column of block 0] (fp32-indexed, as slab_quad16), left = N - that column, ok = row in range
template <int NB>
__device__ __forceinline__ void slab_row16(float* p, const f32x4 (&v)[NB], bool ok, int left,
                                           const float* ws, bool vec, bool wide, int fq) {
  if (wide) {
    u16* q = (u16*)ws + (p - ws);
#pragma unroll
    for (int j = 0; j + 1 < NB; j += 2) {
      uint2 a, b;
      a.x = pack2h(v[j][0] * SLAB16_SCALE, v[j][1] * SLAB16_SCALE);
      a.y = pack2h(v[j][2] * SLAB16_SCALE, v[j][3] * SLAB16_SCALE);
      b.x = pack2h(v[j + 1][0] * SLAB16_SCALE, v[j + 1][1] * SLAB16_SCALE);
      b.y = pack2h(v[j + 1][2] * SLAB16_SCALE, v[j + 1][3] * SLAB16_SCALE);
      const uint4 w = widen_pair(a, b);
      const int c = 16 * j + wide_col(fq);
      if (ok && c < left) *reinterpret_cast<uint4*>(q + c) = w;
    }
    if (NB & 1) {
      const int c = 16 * (NB - 1) + 4 * fq;
      if (ok && c < left) slab_quad16(p + c, v[NB - 1], vec, left - c, ws);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int c = 16 * j + 4 * fq;
    if (ok && c < left) slab_quad16(p + c, v[j], vec, left - c, ws);
  }
}

// one lane's row of NB adjacent 16-column blocks of the output: col0 = first column of block 0
template <int EPI, int NB>
__device__ __forceinline__ void store_row(void* C, int ldc, int row, int col0, int N,
                                          const f32x4 (&v)[NB], const u16* bias, bool ok,
                                          bool vec, bool wide, int fq) {
  if (wide) {
    u16* prow = (u16*)C + (long)row * ldc;
#pragma unroll
    for (int j = 0; j + 1 < NB; j += 2) {
      const int ca = col0 + 16 * j + 4 * fq;
      const uint2 a = pack_quad<EPI>(v[j], bias, ca, ca < N);
      const uint2 b = pack_quad<EPI>(v[j + 1], bias, ca + 16, ca + 16 < N);
      const uint4 w = widen_pair(a, b);
      const int c = col0 + 16 * j + wide_col(fq);
      if (ok && c < N) *reinterpret_cast<uint4*>(prow + c) = w;
    }
    if (NB & 1) {
      const int c = col0 + 16 * (NB - 1) + 4 * fq;
      if (ok && c < N) store_quad<EPI>(C, ldc, row, c, N, v[NB - 1], bias, vec);
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int c = col0 + 16 * j + 4 * fq;
    if (ok && c < N) store_quad<EPI>(C, ldc, row, c, N, v[j], bias, vec);
  }
}

// s_waitcnt vmcnt(N) with expcnt/lgkmcnt left at their maxima (gfx9 encoding)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// s_waitcnt vmcnt(INSTR * ahead) for a wave-uniform ahead in [0, MAXA]: retire everything
// but the `ahead` youngest tiles of INSTR LDS-DMA instructions each
template <int INSTR, int MAXA>
__device__ __forceinline__ void wait_ahead(int ahead) {
  static_assert(MAXA <= 4 && INSTR * MAXA < 64, "vmcnt range");
  if constexpr (MAXA >= 4) { if (ahead >= 4) { wait_vmcnt<INSTR * 4>(); return; } }
  if constexpr (MAXA >= 3) { if (ahead == 3) { wait_vmcnt<INSTR * 3>(); return; } }
  if constexpr (MAXA >= 2) { if (ahead == 2) { wait_vmcnt<INSTR * 2>(); return; } }
  if constexpr (MAXA >= 1) { if (ahead == 1) { wait_vmcnt<INSTR>(); return; } }
  wait_vmcnt<0>();
}

// s_waitcnt lgkmcnt(0) with vmcnt / expcnt left at their maxima: the wave's ds_reads done
__device__ __forceinline__ void lgkmcnt0() { __builtin_amdgcn_s_waitcnt(0xC07F); }

// a raw s_barrier (a __syncthreads() would emit vmcnt(0) and drain the LDS-DMA in flight)
// that neither the compiler's memory operations nor its scheduler move across
__device__ __forceinline__ void raw_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::: "memory");
}

// one MFMA operand fragment (8 bf16 of K half kk, K quarter fq = lane / 16) of tile row `row`
// from an LDS part of 128-B rows whose 16-B chunk c is stored at chunk c ^ ((row >> 1) & 7)
__device__ __forceinline__ bf16x8 read_frag(const char* part, int row, int kk, int fq) {
  const int c = kk * 4 + fq;
  return *reinterpret_cast<const bf16x8*>(part + row * 128 + ((c ^ ((row >> 1) & 7)) << 4));
}

// Block -> (output tile, K split). Without split-K: the XCD remap over tiles (n-major order,
// so an XCD's tiles share W panels). With split-K, (split, tile) is one split-major index
// remapped over the whole grid, so an XCD's blocks work on ONE K slice: its L2 fetches that
// slice of A once instead of every XCD fetching all of A (rocprofv3 TCC_EA0_RDREQ_*: the
// down projection at M=512, split 8, read 224 MB per call for 132 MB of operands).
// The hardware places linear block id L = y * gridDim.x + x on XCD L % 8.
__device__ __forceinline__ void split_tile(int nwg, bool grouped, int& tile, int& ks) {
  if (grouped || gridDim.y == 1) {
    tile = xcd_remap(blockIdx.x, nwg);
    ks = blockIdx.y;
    return;
  }
  const int total = nwg * (int)gridDim.y;
  const int lg = xcd_remap((int)(blockIdx.y * gridDim.x + blockIdx.x), total);
  ks = lg / nwg;
  tile = lg - ks * nwg;
}

// tile index -> tile origin. GM = 1: n-major order (consecutive tiles share one W panel).
// GM > 1: grouped order, an XCD's ~32 consecutive tiles cover GM tile-rows x 32/GM
// tile-columns, so its CUs share both A and W panels in its L2
template <int BM, int BN, int GM>
__device__ __forceinline__ void tile_origin(int tile, int tiles_m, int tiles_n, int& m0, int& n0) {
  if (GM > 1) {
    const int per_group = GM * tiles_n;
    const int first_m = (tile / per_group) * GM;
    const int gsz = min(tiles_m - first_m, GM);
    const int in_g = tile % per_group;
    m0 = (first_m + in_g % gsz) * BM;
    n0 = (in_g / gsz) * BN;
  } else {
    m0 = (tile % tiles_m) * BM;
    n0 = (tile / tiles_m) * BN;
  }
}

// What a workgroup works on: rows [row0 + m0, ..) of A / C within a group of Mg rows (grouped
// mode: grid.z = group, rows [off[g], off[g+1]), weights W + g N ldw; else the whole matrix,
// M = max rows of any group), columns from n0, K-tiles [kb / BK, kb / BK + nk) of split ks.
// A block with m0 >= Mg has nothing to do (block-uniform).
// tile_list (grouped mode only, nullable): the compact grid (tiles x column tiles, splits, 1)
// over the list moe_align_kernel wrote for this BM — pair 0 = (item count, BM), pair 1 + i =
// (group, first row within the group) of item i. Workgroup t = blockIdx.x takes column tile
// t % tiles_n of item t / tiles_n; at or past the count it has nothing to do. No XCD remap:
// the items with work are the first of the grid, and the hardware's round-robin placement
// (block L on XCD L % 8) spreads them over all eight XCDs, where the remap packs consecutive
// tiles onto one (T = 1, 8 items: every working workgroup on XCD 0, the gate/up GEMM 52.6 us
// against 32.6 us on the dense grid). The grid is sized by the host bound
// ceil(rows / BM) + groups on the item count, not by M x groups. The tile a workgroup computes
// is the one the dense grid's (m0, n0, blockIdx.z = group) workgroup computes.
struct BlockCoord {
  int row0, Mg, m0, n0, kb, nk, ks;
  const u16* Wg;
};
template <int BM, int BN, int GM>
__device__ __forceinline__ BlockCoord block_coord(const u16* W, int ldw, int M, int N, int K,
                                                  int k_split_len, const int* group_off,
                                                  const int* tile_list = nullptr) {
  BlockCoord b;
  b.row0 = 0;
  b.Mg = M;
  b.Wg = W;
  if (tile_list != nullptr) {
    const int tiles_n = (N + BN - 1) / BN;
    const int tile = blockIdx.x;
    const int item = tile / tiles_n;
    b.ks = blockIdx.y;
    b.kb = b.ks * k_split_len;
    b.nk = min(k_split_len, K - b.kb) / BK;
    b.n0 = (tile - item * tiles_n) * BN;
    b.m0 = 0;
    b.Mg = 0;                                          // past the list: nothing to do
    if (item < tile_list[0]) {
      const int g = tile_list[2 + 2 * item];
      b.m0 = tile_list[3 + 2 * item];
      b.row0 = group_off[g];
      b.Mg = group_off[g + 1] - b.row0;
      b.Wg = W + (long)g * N * ldw;
    }
    return b;
  }
  if (group_off != nullptr) {
    b.row0 = group_off[blockIdx.z];
    b.Mg = group_off[blockIdx.z + 1] - b.row0;
    b.Wg = W + (long)blockIdx.z * N * ldw;
  }
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  int tile;
  split_tile(tiles_m * tiles_n, group_off != nullptr, tile, b.ks);
  tile_origin<BM, BN, GM>(tile, tiles_m, tiles_n, b.m0, b.n0);
  b.kb = b.ks * k_split_len;
  b.nk = min(k_split_len, K - b.kb) / BK;
  return b;
}

// The epilogue of a wave holding MI x NI transposed accumulator blocks:
// acc[i][j][r] = C[wr0 + 16 i + fr][wc0 + 16 j + 4 fq + r] (wr0 within the group's rows).
// Split-K (grid.y > 1): the fp32 slab of split b.ks, or its fp16 image (EPI_SLAB16). Else the
// fused store: SiLU(gate) * up over the block pairs (j, j + 1), j even, or a row of blocks with
// bias / GELU. With NI odd the wave's pairs are not (even, odd) blocks: such a kernel stores
// its SiLU result itself (gemm8p224_kernel) and nothing is stored here. Used by the 8-phase
// kernels. gemm_bf16_kernel keeps the same text inline (hipcc allocated its registers
// differently through this function) and the 4-wave kernels an epilogue of their own (pinned
// accumulator copies, gemm4w.h).
template <int EPI, int MI, int NI>
__device__ __forceinline__ void gemm_epilogue(const f32x4 (&acc)[MI][NI], int wr0, int wc0,
                                              const BlockCoord& b, void* C, int ldc, int M, int N,
                                              const u16* bias, float* ws, int fr, int fq) {
  if (gridDim.y > 1) {
    float* slab = ws + (long)b.ks * M * N;
    const int sm = g_slab_store;
    const bool vec = (N & 3) == 0;
    if (EPI == EPI_SLAB16) {
      const bool wide = slab_wide(N, ws);
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wr0 + 16 * i + fr;
        slab_row16<NI>(slab + (long)(b.row0 + row) * N + wc0, acc[i], row < b.Mg, N - wc0, ws,
                       vec, wide, fq);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int row = wr0 + 16 * i + fr;
      if (row >= b.Mg) continue;
      float* srow = slab + (long)(b.row0 + row) * N;
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const int col = wc0 + 16 * j + 4 * fq;
        if (col >= N) continue;
        slab_quad(srow + col, acc[i][j], sm, vec, N - col, ws);
      }
    }
    return;
  }
  const bool vec = out_vec<EPI>(C, ldc, N, bias);
  const bool wide = out_wide<EPI>(C, ldc, N, bias);
  if constexpr (EPI == EPI_SILU) {
    if constexpr (NI % 2 == 0) {
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wr0 + 16 * i + fr;
        if (row >= b.Mg) continue;
#pragma unroll
        for (int j = 0; j < NI; j += 2) {
          const int gcol = wc0 + 16 * j;             // first gate column of the pair
          if (gcol < N)
            store_silu_quad(C, ldc, b.row0 + row, (gcol >> 5) * 16 + 4 * fq, acc[i][j],
                            acc[i][j + 1], vec);
        }
      }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < MI; ++i) {
    const int row = wr0 + 16 * i + fr;
    store_row<EPI, NI>(C, ldc, b.row0 + row, wc0, N, acc[i], bias, row < b.Mg, vec, wide, fq);
  }
}

// split-K reduction + epilogue: one thread per output element group of 4 columns
template <int EPI>
static __global__ void __launch_bounds__(256) splitk_reduce_kernel(void* __restrict__ C, int ldc,
                                                            const float* __restrict__ ws, int M,
                                                            int N, int splits,
                                                            const u16* __restrict__ bias) {
  const int outN = (EPI == EPI_SILU) ? N / 2 : N;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)M * outN) return;
  const int row = (int)(gid / outN), col = (int)(gid % outN);
  if (EPI == EPI_SILU) {
    const int grp = col >> 4, in = col & 15;
    const long gi = (long)row * N + grp * 32 + in, ui = gi + 16;
    float g = 0.f, u = 0.f;
    for (int s = 0; s < splits; ++s) { g += ws[(long)s * M * N + gi]; u += ws[(long)s * M * N + ui]; }
    ((u16*)C)[(long)row * ldc + col] = f2bf(silu_f(g) * u);
  } else {
    float v = 0.f;
    for (int s = 0; s < splits; ++s) v += ws[(long)s * M * N + (long)row * N + col];
    store_pair_or_one<EPI>(C, ldc, row, col, v, bias);
  }
}


// the dispatch signature every family shares: (tile_cfg) -> that family's launcher, or
// DLI_NOT_MINE when the tile id belongs to another family
// tl / tl_max: the grouped tile list and the host bound on its item count (block_coord);
// null / 0 everywhere but the generic tile family's list form
#define DLI_GEMM_ARGS const void *A, int lda, const void *W, int ldw, void *C, int ldc, int M, \
                      int N, int K, int splits, const void *bias, void *ws, const int *go,  \
                      int groups, const int *tl, int tl_max, hipStream_t st
#define DLI_GEMM_PASS A, lda, W, ldw, C, ldc, M, N, K, splits, bias, ws, go, groups, tl, tl_max, st
constexpr int DLI_NOT_MINE = -0x4d494e45;

// The launcher of every kernel with the (A, lda, W, ldw, C, ldc, M, N, K, k_split_len, bias,
// ws, group_off) signature: BM x BN tiles on grid (tiles, splits, groups), LDS bytes of
// dynamic LDS (> 64 KiB needs the opt-in, once per kernel), then the split-K reduce unless
// C == nullptr (the partial slabs are left for a fused consumer, fused_reduce.hip). SILU_N:
// the SiLU*up epilogue needs N to be a multiple of it; 0 = this tile has no SiLU epilogue
// (a wave's column range does not hold whole gate/up pairs). LIST: the kernel takes the tile
// list as its last argument (grid (tl_max x column tiles, splits, 1) when one is given); the
// other families refuse one.
template <auto KERNEL, int EPI, int BM, int BN, int THREADS, size_t LDS, int SILU_N,
          bool LIST = false>
static int launch_gemm(DLI_GEMM_ARGS) {
  if (EPI == EPI_SILU && (SILU_N == 0 || N % (SILU_N ? SILU_N : 1)))
    return (int)hipErrorInvalidValue;
  if (tl != nullptr && (!LIST || go == nullptr || tl_max < (M + BM - 1) / BM + groups))
    return (int)hipErrorInvalidValue;
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  int ksl = K / splits;
  ksl = (ksl / BK) * BK;
  if (ksl * splits != K) return (int)hipErrorInvalidValue;
  static bool attr_done = false;
  if (!attr_done) {
    const hipError_t e = hipFuncSetAttribute((const void*)KERNEL,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  if constexpr (LIST) {
    const dim3 grid = tl != nullptr ? dim3(tl_max * ((N + BN - 1) / BN), splits, 1)
                                    : dim3(tiles, splits, groups);
    KERNEL<<<grid, THREADS, LDS, st>>>((const u16*)A, lda, (const u16*)W, ldw, C, ldc, M, N, K,
                                       ksl, (const u16*)bias, (float*)ws, go, tl);
  } else {
    KERNEL<<<dim3(tiles, splits, groups), THREADS, LDS, st>>>(
        (const u16*)A, lda, (const u16*)W, ldw, C, ldc, M, N, K, ksl, (const u16*)bias,
        (float*)ws, go);
  }
  if (splits > 1 && C != nullptr) {
    const int outN = (EPI == EPI_SILU) ? N / 2 : N;
    const long total = (long)M * outN;
    splitk_reduce_kernel<EPI><<<(int)((total + 255) / 256), 256, 0, st>>>(
        C, ldc, (const float*)ws, M, N, splits, (const u16*)bias);
  }
  DLI_RETURN_LAUNCH();
}

int gemm_tiles_dispatch(int epi, int tile_cfg, DLI_GEMM_ARGS);
int gemm_8p_dispatch(int epi, int tile_cfg, DLI_GEMM_ARGS);
int gemm_4w_dispatch(int epi, int tile_cfg, DLI_GEMM_ARGS);
int gemm_4wp_dispatch(int epi, int tile_cfg, DLI_GEMM_ARGS);
int gemm_gemv_dispatch(int epi, int tile_cfg, DLI_GEMM_ARGS);
int gemm_tiles_set_slab_store(int mode);
int gemm_8p_set_slab_store(int mode);
int gemm_4w_set_slab_store(int mode);

// EPI -> template argument, for a family's dispatch<EPI>(tile_cfg, ...); the families with
// an fp16 slab store (tiles, 8-phase) take DLI_EPI_SWITCH_S16
#define DLI_EPI_SWITCH_S16(FN)                                                     \
  if (epi == EPI_SLAB16) {                                                         \
    if (C != nullptr || splits < 2) return (int)hipErrorInvalidValue;              \
    return FN<EPI_SLAB16>(tile_cfg, DLI_GEMM_PASS);                                \
  }                                                                                \
  DLI_EPI_SWITCH(FN)

#define DLI_EPI_SWITCH(FN)                                                         \
  switch (epi) {                                                                   \
    case EPI_BF16: return FN<EPI_BF16>(tile_cfg, DLI_GEMM_PASS);                   \
    case EPI_F32: return FN<EPI_F32>(tile_cfg, DLI_GEMM_PASS);                     \
    case EPI_SILU: return FN<EPI_SILU>(tile_cfg, DLI_GEMM_PASS);                   \
    case EPI_BIAS_GELU: return FN<EPI_BIAS_GELU>(tile_cfg, DLI_GEMM_PASS);         \
    case EPI_BIAS: return FN<EPI_BIAS>(tile_cfg, DLI_GEMM_PASS);                   \
    default: return (int)hipErrorInvalidValue;                                     \
  }
