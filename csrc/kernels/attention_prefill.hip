// Causal variable-length (packed) GQA prefill attention on MFMA — SURVEY.md §2.4 K7.
//
// Reads q/k/v straight out of the fused QKV activation (row stride = (Hq+2Hkv)*hd) after
// the in-place RoPE, so no separate K/V copies exist. A workgroup = 4 waves = 64 query rows
// of one query head (16 per wave); the workgroup streams 64-key tiles of K and V through
// LDS ONCE for all 4 waves (each wave used to fetch its own K rows from global memory: 4x
// the K/V traffic, O(L^2) bytes per head for long prompts):
//   stage      tile t+1 is loaded into registers while tile t is computed, then written
//              to LDS between two barriers (K and V rows padded to hd*2+32 B:
//              conflict-free ds_read_b128 of the A operand and transposing reads of V)
//   S^T[key, q] = K . Q^T        mfma_f32_16x16x32_bf16, K rows as the A operand
//   softmax along keys           exp2 domain, online (flash) rescaling per tile
//   O[q, d] += P[q, key] . V     P re-used from the accumulator registers (permuted key
//                                order); V read as the B operand with the CDNA4 transposing
//                                ds_read_b64_tr_b16 (cdna_hip_programming.md T10)
// Causality: a wave skips the math of tiles entirely above its rows (it still helps stage
// them); the workgroup stops at its last row's bound.
// Chunked prefill (PAGED): the chunk's K/V have already been written to the paged cache
// (rope_cache), so keys come from the cache through the block table: a chunk of len queries
// at positions [ctx - len, ctx) attends over all ctx cached keys of its sequence (earlier
// chunks, a recomputed prefix) with the causal bound shifted by ctx - len.
// Sliding window (window > 0): query q sees the keys q - window < j <= q, `window` keys with
// its own. A workgroup starts at the 64-key tile that holds the first key of its first row,
// a wave skips the tiles wholly below its own first row's window as it skips those above its
// rows, and the tiles a window edge crosses are masked per (query, key). A row's own key is
// always visible, so no row has an empty window.
// Grid: (ceil(max_len / (16 wph)), num_seqs, Hq * wph / 4). wph = waves per query head: 4
// (64 rows per workgroup) in general; for batches of short prompts (max_len <= 32 / 16) a
// workgroup packs 2 / 4 query heads of one GQA group (2 / 1 waves each): the K/V tiles it
// stages serve every packed head, and no wave idles past a 32-token prompt (the bench's
// 512 x 32-token prefill ran 16,384 half-idle workgroups).
#include "common.h"
#include <limits.h>

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;
typedef short s16x8 __attribute__((ext_vector_type(8)));
#define PF_WAVES 4
#define PF_QROWS 16
#define PF_KT 64

// KV = fp8 (PAGED only): the cache holds one e4m3fn byte per element (common.h). A thread loads
// half the bytes (16 B = 16 dims per chunk) and dequantises them to bf16 in the register stage,
// on their way into the same LDS image; scale_log2 then carries k_scale and the final 1 / l
// factor v_scale, which travels as a trailing argument that is empty for a bf16 cache.
template <bool FP8>
struct PrefillKvScale {
  float v_scale;
};
template <>
struct PrefillKvScale<false> {};

template <int HD, bool PAGED, typename KV = u16>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) prefill_attn_kernel(
    u16* __restrict__ out, int out_stride, const u16* __restrict__ qkv, int row_stride,
    const int* __restrict__ cu_seqlens, int hq, int hkv, float scale_log2,
    const int* __restrict__ ctx_lens, const KV* __restrict__ k_cache,
    const KV* __restrict__ v_cache, const int* __restrict__ block_tables, int bt_stride,
    int block_size, int wph, int window, const PrefillKvScale<sizeof(KV) == 1> kvs) {
  constexpr bool FP8 = sizeof(KV) == 1;
  static_assert(!FP8 || PAGED, "only the paged cache is FP8");
  constexpr int KK = HD / 32, DB = HD / 16;
  // K row in LDS (u16): 288 B for hd 128 (72 dwords; 40 for hd 64). With the
  // ds_read_b128 lane groups of gfx950 ({0-3,12-15,20-27}, ... MI355X_MICROARCH.md §LDS)
  // the former 272-B rows put two lanes of every group on one 16-B slot: 2-way, measured
  // as 51 % SQ_LDS_BANK_CONFLICT (profiles/r6/s31); a 72-dword row is conflict-free.
  constexpr int KROW = HD + 16;
  constexpr int VROW = HD + 16;                    // V row in LDS (u16): hd*2 + 32 B
  constexpr int CH = HD / 8;                       // 16-B chunks per row
  constexpr int PER = PF_KT * CH / 256;            // chunks per thread per tile (K or V)
  constexpr int NLD = FP8 ? PER / 2 : PER;         // 16-B loads per thread per tile (K or V)
  __shared__ __attribute__((aligned(16))) u16 ktile[PF_KT * KROW];
  __shared__ __attribute__((aligned(16))) u16 vtile[PF_KT * VROW];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int seq = blockIdx.y, h = blockIdx.z * (PF_WAVES / wph) + wid / wph;
  const int col = lane & 15, grp = lane >> 4;
  const int s0 = cu_seqlens[seq], len = cu_seqlens[seq + 1] - s0;
  const int nkeys = PAGED ? ctx_lens[seq] : len;                 // keys visible to the chunk
  const int qoff = nkeys - len;                                  // position of query row 0
  const int wg_q0 = blockIdx.x * wph * PF_QROWS;
  if (wg_q0 >= len) return;                                      // workgroup-uniform exit
  const int q0 = wg_q0 + (wid % wph) * PF_QROWS;                 // this wave's first row
  const bool active = q0 < len;
  const int G = hq / hkv, kvh = h / G;
  const u16* qbase = qkv + (long)h * HD;
  const u16* kbase = qkv + (long)(hq + kvh) * HD;
  const u16* vbase = qkv + (long)(hq + hkv + kvh) * HD;
  const int* btab = PAGED ? block_tables + (long)seq * bt_stride : nullptr;
  const long head_off = (long)kvh * block_size * HD;             // (blk, head) panel offset

  bf16x8 qf[KK];
  {
    const int qr = min(q0 + col, len - 1);
    const u16* qp = qbase + (long)(s0 + qr) * row_stride;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      uint4 v = *reinterpret_cast<const uint4*>(qp + kk * 32 + grp * 8);
      qf[kk] = *reinterpret_cast<bf16x8*>(&v);
    }
  }
  const int my_q = qoff + q0 + col;        // position of the query row of this lane's column
  float m_run = -INFINITY, l_part = 0.f;
  f32x4 o_acc[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) o_acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int kend_wg = min(nkeys, qoff + wg_q0 + wph * PF_QROWS);       // last row's bound
  const int kend_w = min(nkeys, qoff + q0 + PF_QROWS);                 // this wave's bound
  // window: keys > (query position) - wspan; off = a span no key reaches
  const int wspan = window > 0 ? window : INT_MAX;
  const int kbeg_w = max(0, qoff + q0 - wspan + 1);                    // this wave's first key
  const int kbeg_wg = max(0, qoff + wg_q0 - wspan + 1) / PF_KT * PF_KT;   // first tile staged

  // the next K/V tile in flight in registers: named values, not arrays — uint4 kreg[PER]
  // indexed in a loop was promoted to LDS by the compiler (a second staging copy through
  // LDS, its bank conflicts counted with the tile's: profiles/r6/README.md §12)
  static_assert(PER == 2 || PER == 4, "tile staging assumes 2 or 4 chunks per thread");
  uint4 kr0, kr1, kr2, kr3, vr0, vr1, vr2, vr3;
  auto load1 = [&](int j, int k0, uint4& kr, uint4& vr) {
    const int i = tid + 256 * j;
    const int r = i / CH, c = i % CH;
    const int tok = min(k0 + r, nkeys - 1);
    if constexpr (FP8) {                           // chunk i of the tile's 64 x CH / 2
      const int r8 = i / (CH / 2), c8 = i % (CH / 2);
      const int tok8 = min(k0 + r8, nkeys - 1);
      const long e = (long)btab[tok8 / block_size] * hkv * block_size * HD + head_off +
                     (long)(tok8 % block_size) * HD + c8 * 16;
      kr = *reinterpret_cast<const uint4*>(k_cache + e);
      vr = *reinterpret_cast<const uint4*>(v_cache + e);
    } else if (PAGED) {
      const long e = (long)btab[tok / block_size] * hkv * block_size * HD + head_off +
                     (long)(tok % block_size) * HD + c * 8;
      kr = *reinterpret_cast<const uint4*>(k_cache + e);
      vr = *reinterpret_cast<const uint4*>(v_cache + e);
    } else {
      const long row = s0 + tok;
      kr = *reinterpret_cast<const uint4*>(kbase + row * row_stride + c * 8);
      vr = *reinterpret_cast<const uint4*>(vbase + row * row_stride + c * 8);
    }
  };
  auto load_tile = [&](int k0) {
    load1(0, k0, kr0, vr0);
    if constexpr (NLD >= 2) load1(1, k0, kr1, vr1);
    if constexpr (NLD == 4) {
      load1(2, k0, kr2, vr2);
      load1(3, k0, kr3, vr3);
    }
  };
  auto store1 = [&](int j, const uint4& kr, const uint4& vr) {
    const int i = tid + 256 * j;
    const int r = i / CH, c = i % CH;
    if constexpr (FP8) {
      const int r8 = i / (CH / 2), c8 = i % (CH / 2);
      uint4 lo, hi;
      fp8x16_to_bf16(kr, lo, hi);
      *reinterpret_cast<uint4*>(ktile + r8 * KROW + c8 * 16) = lo;
      *reinterpret_cast<uint4*>(ktile + r8 * KROW + c8 * 16 + 8) = hi;
      fp8x16_to_bf16(vr, lo, hi);
      *reinterpret_cast<uint4*>(vtile + r8 * VROW + c8 * 16) = lo;
      *reinterpret_cast<uint4*>(vtile + r8 * VROW + c8 * 16 + 8) = hi;
    } else {
      *reinterpret_cast<uint4*>(ktile + r * KROW + c * 8) = kr;
      *reinterpret_cast<uint4*>(vtile + r * VROW + c * 8) = vr;
    }
  };
  load_tile(kbeg_wg);
  const int qrow = (lane >> 2) & 3, pcol = lane & 3;
  for (int k0 = kbeg_wg; k0 < kend_wg; k0 += PF_KT) {
    __syncthreads();                                             // previous tile fully read
    store1(0, kr0, vr0);
    if constexpr (NLD >= 2) store1(1, kr1, vr1);
    if constexpr (NLD == 4) {
      store1(2, kr2, vr2);
      store1(3, kr3, vr3);
    }
    __syncthreads();                                             // tile visible to all waves
    if (k0 + PF_KT < kend_wg) load_tile(k0 + PF_KT);             // in flight during compute
    // tile above this wave's rows, or wholly below their window
    if (!active || k0 >= kend_w || k0 + PF_KT <= kbeg_w) continue;
    // ---- S^T = K . Q^T over four 16-key subtiles
    f32x4 s_acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const u16* kp = ktile + (16 * s + col) * KROW;
      s_acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        s_acc[s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            *reinterpret_cast<const bf16x8*>(kp + kk * 32 + grp * 8), qf[kk], s_acc[s], 0, 0, 0);
    }
    float p[16], tmax = -INFINITY;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + 16 * s + 4 * grp + r;
        const float v = (key <= my_q && key < nkeys && key > my_q - wspan)
                            ? s_acc[s][r] * scale_log2 : -INFINITY;
        p[s * 4 + r] = v;
        tmax = fmaxf(tmax, v);
      }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
    const float m_new = fmaxf(m_run, tmax);
    // rows past the sequence end may see no valid key: keep them finite
    const float m_use = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = exp2f(m_run - m_use);
    m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) { p[j] = exp2f(p[j] - m_use); psum += p[j]; }
    l_part = l_part * alpha + psum;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = __shfl(alpha, 4 * grp + r, 64);
#pragma unroll
      for (int i = 0; i < DB; ++i) o_acc[i][r] *= a;
    }
    // ---- O += P . V, two 32-key halves; B operand rows: keys 32h + 4grp + q and
    // 32h + 16 + 4grp + q (the p[] key order), cols 16i + 4p via tr16 reads
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      bf16x8 pa;
#pragma unroll
      for (int j = 0; j < 8; ++j) pa[j] = (__bf16)p[8 * hh + j];
#pragma unroll
      for (int i = 0; i < DB; ++i) {
        const u16* a0 = vtile + (32 * hh + 4 * grp + qrow) * VROW + 16 * i + 4 * pcol;
        const u16* a1 = vtile + (32 * hh + 16 + 4 * grp + qrow) * VROW + 16 * i + 4 * pcol;
        s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(a0));
        s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (__attribute__((address_space(3))) s16x4*)(a1));
        s16x8 w = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o_acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, *reinterpret_cast<bf16x8*>(&w),
                                                          o_acc[i], 0, 0, 0);
      }
    }
  }
  if (!active) return;
  float l_tot = l_part + __shfl_xor(l_part, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
  if constexpr (FP8) inv *= kvs.v_scale;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float iv = __shfl(inv, 4 * grp + r, 64);
    const int qr = q0 + 4 * grp + r;
    if (qr < len) {
      u16* op = out + (long)(s0 + qr) * out_stride + (long)h * HD;
#pragma unroll
      for (int i = 0; i < DB; ++i) op[16 * i + col] = f2bf(o_acc[i][r] * iv);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Long sequences: 8 waves x 32 query rows = 256 rows per workgroup, v_mfma_f32_32x32x16_bf16,
// "swapped" products so that no value moves between lanes except one max exchange per tile:
//   S^T[key, q] = K . Q^T        A = K rows from LDS (ds_read_b128), B = Q^T from registers;
//                                each lane owns ONE query (its column) and 32 of the tile's
//                                64 keys (its rows), so the row max / sum are lane-local
//   O^T[d, q] += V^T . P^T       the S^T accumulator converted to bf16 IS the B operand
//                                (cdna_hip_programming.md §3 'accumulator as operand': k-step s
//                                = registers 8s..8s+7, keys 16s + 8(j>>2) + 4h + (j&3)); V^T
//                                comes from ds_read_b64_tr_b16 reads of those key rows
// so the online-softmax rescale of O^T is lane-local too. K/V tiles of 64 keys are staged
// ONCE per workgroup (8 waves share them: half the LDS reads per FLOP of the 16-row kernel)
// through registers into a double-buffered LDS image with the 256-B-row XOR swizzle that
// keeps both the row reads and the transposed reads conflict-free (§5.5 T10 image (b)); the
// next tile's global loads are in flight during the current tile (one barrier per tile).
// Causal: key tiles stop at the workgroup's last row; a wave skips tiles entirely above its
// rows and masks only tiles that cross its diagonal. Row blocks run longest-first.
#define PL_WAVES 8
#define PL_QROWS 32
#define PL_ROWS (PL_WAVES * PL_QROWS)
#define PL_KT 64
// shortest max_seqlen that takes the 256-row kernel; below, the 64-row kernel wastes fewer
// idle waves (settable for A/B runs and tests: dli_prefill_set_min_len)
static int g_pl_min_len = 256;
static int g_pf_pack = 1;                          // head packing for short prompts (A/B)

// Tile image: 8-row x 32-column subtiles of 512 B (cdna_hip_programming.md §5.5 T10, image
// (a)): conflict-free for the 32x32x16 row reads (ds_read_b128) AND the transposed reads
// (ds_read_b64_tr_b16), and every read's address is one of 2 lane bases + an immediate.
__device__ __forceinline__ int pl_off(int row, int ch) {      // byte offset of 16-B chunk
  return 2048 * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}
__device__ __forceinline__ float pl_max3(float a, float b, float c) {  // no canonicalise
  float r;
  asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
#define PL_RESCALE_THR 8.f      // log2 units: a running max is raised only by more than this

template <int HD, bool PAGED>
__global__ void __launch_bounds__(512) prefill_attn32_kernel(
    u16* __restrict__ out, int out_stride, const u16* __restrict__ qkv, int row_stride,
    const int* __restrict__ cu_seqlens, int hq, int hkv, float scale_log2,
    const int* __restrict__ ctx_lens, const u16* __restrict__ k_cache,
    const u16* __restrict__ v_cache, const int* __restrict__ block_tables, int bt_stride,
    int block_size, int window) {
  static_assert(HD == 128, "long-sequence kernel: head_dim 128");
  constexpr int KC = HD / 16;                      // K-steps of the QK^T product
  constexpr int DBK = HD / 32;                     // 32-wide d blocks of O^T
  constexpr int TILE_B = PL_KT * HD * 2;           // bytes per K (or V) tile image
  constexpr int NBUF = 3;
  __shared__ __attribute__((aligned(16))) char lds[NBUF][2][TILE_B];   // [buf][K/V]
  const int seq = blockIdx.y, h = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qc = lane & 31, hi = lane >> 5;
  const int s0 = cu_seqlens[seq], len = cu_seqlens[seq + 1] - s0;
  const int nblk = (len + PL_ROWS - 1) / PL_ROWS;
  const int blk = (int)(gridDim.x - 1 - blockIdx.x);            // longest blocks first
  if (blk >= nblk) return;                                       // workgroup-uniform
  const int nkeys = PAGED ? ctx_lens[seq] : len;
  const int qoff = nkeys - len;
  const int wg_q0 = blk * PL_ROWS;
  const int q0 = wg_q0 + wid * PL_QROWS;                         // this wave's first row
  const bool active = q0 < len;
  const int G = hq / hkv, kvh = h / G;
  const u16* kbase = qkv + (long)(hq + kvh) * HD;
  const u16* vbase = qkv + (long)(hq + hkv + kvh) * HD;
  const int* btab = PAGED ? block_tables + (long)seq * bt_stride : nullptr;
  const long head_off = (long)kvh * block_size * HD;

  // Q^T operand: lane (query qc, half hi) holds Q[q][16c + 8hi .. +7]
  bf16x8 qf[KC];
  {
    const int qr = min(q0 + qc, len - 1);
    const u16* qp = qkv + (long)(s0 + qr) * row_stride + (long)h * HD + 8 * hi;
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      uint4 v = *reinterpret_cast<const uint4*>(qp + 16 * c);
      qf[c] = *reinterpret_cast<bf16x8*>(&v);
    }
  }
  const int qpos = qoff + q0 + qc;                 // position of this lane's query
  const int wq_lo = qoff + q0, wq_hi = qoff + min(q0 + PL_QROWS, len) - 1;
  const int kend_wg = min(nkeys, qoff + min(wg_q0 + PL_ROWS, len));
  const int ntiles = (kend_wg + PL_KT - 1) / PL_KT;
  // window: keys > (query position) - wspan; off = a span no key reaches. The workgroup's
  // first tile holds the first key of its first row; a wave's first key is that of its own
  const int wspan = window > 0 ? window : INT_MAX;
  const int tfirst = max(0, qoff + wg_q0 - wspan + 1) / PL_KT;
  const int kbeg_w = max(0, wq_lo - wspan + 1);

  f32x16 o[DBK];
#pragma unroll
  for (int i = 0; i < DBK; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m_run = -INFINITY, l_part = 0.f;

  // global -> LDS by LDS-DMA (global_load_lds_dwordx4, no staging registers): an operand's
  // tile image is 16 pieces of 1 KiB (= subtiles 2hp, 2hp+1 of 8-row group rg); wave w
  // stages pieces w and w + 8 of K and of V. The DMA writes lane-linearly (lane L at byte
  // 16L of the piece), so each lane loads the logical chunk that lands there.
  auto stage = [&](int buf, int k0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int piece = wid + 8 * j;
      const int rg = piece >> 1, hp = piece & 1;
      const int r = 8 * rg + ((lane & 31) >> 2);
      const int c = 4 * (2 * hp + (lane >> 5)) + ((lane & 3) ^ ((r >> 2) & 3));
      const int tok = min(k0 + r, nkeys - 1);
      const u16 *ks, *vs;
      if (PAGED) {
        const long e = (long)btab[tok / block_size] * hkv * block_size * HD + head_off +
                       (long)(tok % block_size) * HD + c * 8;
        ks = k_cache + e;
        vs = v_cache + e;
      } else {
        const long row = (long)(s0 + tok) * row_stride + c * 8;
        ks = kbase + row;
        vs = vbase + row;
      }
      __builtin_amdgcn_global_load_lds((gbl_void*)ks, (lds_void*)&lds[buf][0][piece * 1024],
                                       16, 0, 0);
      __builtin_amdgcn_global_load_lds((gbl_void*)vs, (lds_void*)&lds[buf][1][piece * 1024],
                                       16, 0, 0);
    }
  };

  stage(0, tfirst * PL_KT);
  if (ntiles - tfirst > 1) {
    stage(1, (tfirst + 1) * PL_KT);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");             // tile 0 landed
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  // LDS read bases (image (a)): K row reads of row 32 sub + qc, chunk 2c + hi; transposed V
  // reads by 16-lane group g16, lane (q4, p4) of the group: rows 16 ks + 4 hi + q4 (+8)
  const int g16 = lane >> 4, q4 = (lane >> 2) & 3, p4 = lane & 3;
  int kbase_off[2], vbase_off[2];
#pragma unroll
  for (int par = 0; par < 2; ++par)
    kbase_off[par] = 2048 * (qc >> 3) + 64 * (qc & 7) + 16 * ((2 * par + hi) ^ ((qc >> 2) & 3));
  {
    const int cl = 2 * (g16 & 1) + (p4 >> 1);
    vbase_off[0] = 64 * (4 * hi + q4) + 16 * (cl ^ hi) + 8 * (p4 & 1);
    vbase_off[1] = 2048 + 64 * (4 * hi + q4) + 16 * (cl ^ (hi ^ 2)) + 8 * (p4 & 1);
  }
  // One barrier per tile: tile t+2 is DMA'd into the buffer tile t-1 used while tile t is
  // computed; the counted vmcnt + barrier closing iteration t retire tile t+1. (A variant
  // running the two 4-wave groups one half-tile apart measured 2x slower: the per-segment
  // branches split the loop body and the compiler no longer interleaves the softmax VALU
  // work with the MFMAs.)
  f32x16 sacc[2];
  int cur = 0;
  for (int t = tfirst; t < ntiles; ++t) {
    const int k0 = t * PL_KT;
    if (t + 2 < ntiles) stage(cur == 0 ? 2 : cur - 1, k0 + 2 * PL_KT);
    if (active && k0 <= wq_hi && k0 + PL_KT > kbeg_w) {
      const char* kt = lds[cur][0];
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[sub][r] = 0.f;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          // = pl_off(32 sub + qc, 2c + hi): lane base by c parity + immediate
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(
              kt + kbase_off[c & 1] + 8192 * sub + 512 * (c >> 1));
          sacc[sub] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[c], sacc[sub], 0, 0, 0);
        }
      }
      // mask (only tiles crossing this wave's diagonal, the key end or a window's lower edge)
      if (k0 + PL_KT - 1 > wq_lo || k0 + PL_KT > nkeys || k0 <= wq_hi - wspan) {
#pragma unroll
        for (int sub = 0; sub < 2; ++sub)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = k0 + 32 * sub + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (key > qpos || key >= nkeys || key <= qpos - wspan) sacc[sub][r] = -INFINITY;
          }
      }
      float mloc = pl_max3(sacc[0][0], sacc[0][1], sacc[0][2]);
#pragma unroll
      for (int r = 3; r < 15; r += 2) mloc = pl_max3(mloc, sacc[0][r], sacc[0][r + 1]);
      mloc = pl_max3(mloc, sacc[0][15], sacc[1][0]);
#pragma unroll
      for (int r = 1; r < 15; r += 2) mloc = pl_max3(mloc, sacc[1][r], sacc[1][r + 1]);
      mloc = pl_max3(mloc, sacc[1][15], sacc[1][15]);
      mloc = pl_max3(mloc, __shfl_xor(mloc, 32, 64), mloc);
      // deferred rescale (§5.5 T13): the running max moves only when the tile's max exceeds
      // it by more than 2^PL_RESCALE_THR, so P <= 2^8 and O^T is rescaled on few tiles
      float alpha = 1.f;
      if ((mloc - m_run) * scale_log2 > PL_RESCALE_THR) {
        alpha = m_run == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((m_run - mloc) * scale_log2);
        m_run = mloc;
      }
      const float mc = (m_run == -INFINITY ? 0.f : m_run) * scale_log2;
      float psum = 0.f;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = __builtin_amdgcn_exp2f(fmaf(sacc[sub][r], scale_log2, -mc));
          sacc[sub][r] = e;
          psum += e;
        }
      l_part = l_part * alpha + psum;
      if (__ballot(alpha != 1.f)) {
#pragma unroll
        for (int i = 0; i < DBK; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
      }
      // O^T += V^T . P^T over 4 k-steps of 16 keys
      const char* vt = lds[cur][1];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int sub = ks >> 1, s = ks & 1;
        bf16x8 pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) pb[j] = (__bf16)sacc[sub][8 * s + j];
#pragma unroll
        for (int db = 0; db < DBK; ++db) {
          // rows 16 ks + 4hi + q4 (and +8), chunk 4db + 2(g16&1) + (p4>>1), half p4&1:
          // pl_off + 8(p4&1) = vbase_off[0 or 1] + 4096 ks + 512 db
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(vt + vbase_off[0] + 4096 * ks + 512 * db));
          const s16x4 up = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(vt + vbase_off[1] + 4096 * ks + 512 * db));
          const s16x8 w = {lo[0], lo[1], lo[2], lo[3], up[0], up[1], up[2], up[3]};
          o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&w),
                                                         pb, o[db], 0, 0, 0);
        }
      }
    }
    if (t + 2 < ntiles) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xC07F);                          // lgkmcnt(0): own reads done
    __builtin_amdgcn_s_barrier();
    cur = (cur == 2) ? 0 : cur + 1;
  }
  if (!active) return;
  const float l_tot = l_part + __shfl_xor(l_part, 32, 64);
  const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
  const int qr = q0 + qc;
  if (qr < len) {
    u16* op = out + (long)(s0 + qr) * out_stride + (long)h * HD;
#pragma unroll
    for (int db = 0; db < DBK; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        U16x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v.v[r] = f2bf(o[db][4 * g + r] * inv);
        *reinterpret_cast<U16x4*>(op + 32 * db + 8 * g + 4 * hi) = v;
      }
  }
}

// KV = fp8: scale_log2 carries k_scale too, and every chunk length takes the 64-row kernel
// (head-packed for short chunks): the 256-row kernel's tiles go global -> LDS by LDS-DMA,
// with no register stage to convert in.
template <bool PAGED, typename KV = u16>
static int launch_prefill(void* out, int out_stride, const void* qkv, int row_stride,
                          const int* cu_seqlens, int num_seqs, int max_seqlen, int hq, int hkv,
                          int hd, float scale, const int* ctx_lens, const void* k_cache,
                          const void* v_cache, const int* block_tables, int bt_stride,
                          int block_size, int window, hipStream_t st, float k_scale = 1.f,
                          [[maybe_unused]] float v_scale = 1.f) {
  constexpr bool FP8 = sizeof(KV) == 1;
  if (num_seqs <= 0 || max_seqlen <= 0) return 0;
  if (window < 0) window = 0;
  if (hq % hkv || (hd != 64 && hd != 128)) return (int)hipErrorInvalidValue;
  const float sl2 = scale * 1.4426950408889634f * k_scale;       // (x 1 for a bf16 cache)
  if constexpr (!FP8) {
    if (hd == 128 && max_seqlen >= g_pl_min_len) {   // long sequences: 256-row workgroups
      dim3 grid32((max_seqlen + PL_ROWS - 1) / PL_ROWS, num_seqs, hq);
      prefill_attn32_kernel<128, PAGED><<<grid32, 512, 0, st>>>(
          (u16*)out, out_stride, (const u16*)qkv, row_stride, cu_seqlens, hq, hkv, sl2, ctx_lens,
          (const u16*)k_cache, (const u16*)v_cache, block_tables, bt_stride, block_size, window);
      DLI_RETURN_LAUNCH();
    }
  }
  // waves per query head: pack 2 / 4 heads of one GQA group into a workgroup for short
  // prompts (the packed heads share their kv head, so G must be a multiple of the pack)
  const int G = hq / hkv;
  int wph = PF_WAVES;
  if (g_pf_pack && max_seqlen <= PF_QROWS && G % 4 == 0) wph = 1;
  else if (g_pf_pack && max_seqlen <= 2 * PF_QROWS && G % 2 == 0) wph = 2;
  const int rows_per_wg = wph * PF_QROWS;
  dim3 grid((max_seqlen + rows_per_wg - 1) / rows_per_wg, num_seqs, hq * wph / PF_WAVES);
  PrefillKvScale<FP8> kvs;
  if constexpr (FP8) kvs.v_scale = v_scale;
  if (hd == 128)
    prefill_attn_kernel<128, PAGED, KV><<<grid, 256, 0, st>>>(
        (u16*)out, out_stride, (const u16*)qkv, row_stride, cu_seqlens, hq, hkv, sl2, ctx_lens,
        (const KV*)k_cache, (const KV*)v_cache, block_tables, bt_stride, block_size, wph,
        window, kvs);
  else
    prefill_attn_kernel<64, PAGED, KV><<<grid, 256, 0, st>>>(
        (u16*)out, out_stride, (const u16*)qkv, row_stride, cu_seqlens, hq, hkv, sl2, ctx_lens,
        (const KV*)k_cache, (const KV*)v_cache, block_tables, bt_stride, block_size, wph,
        window, kvs);
  DLI_RETURN_LAUNCH();
}

// window > 0: sliding-window attention (query q sees keys q - window < j <= q)
extern "C" int dli_prefill_attention(void* out, int out_stride, const void* qkv, int row_stride,
                                     const int* cu_seqlens, int num_seqs, int max_seqlen, int hq,
                                     int hkv, int hd, float scale, int window, hipStream_t st) {
  return launch_prefill<false>(out, out_stride, qkv, row_stride, cu_seqlens, num_seqs,
                               max_seqlen, hq, hkv, hd, scale, nullptr, nullptr, nullptr,
                               nullptr, 0, 16, window, st);
}

// Chunked prefill: q from qkv rows [cu[s], cu[s+1]); keys 0..ctx_lens[s]-1 of sequence s
// from the paged caches [num_blocks, hkv, block_size, hd] through block_tables[s, :].
// kv_fp8: the caches hold e4m3fn bytes with the scales k_scale, v_scale (> 0); else bf16, 1.
extern "C" int dli_prefill_attention_paged(void* out, int out_stride, const void* qkv,
                                           int row_stride, const int* cu_seqlens,
                                           const int* ctx_lens, const void* k_cache,
                                           const void* v_cache, const int* block_tables,
                                           int bt_stride, int num_seqs, int max_seqlen, int hq,
                                           int hkv, int hd, int block_size, float scale,
                                           int window, int kv_fp8, float k_scale, float v_scale,
                                           hipStream_t st) {
  if (block_size <= 0 || !kv_scales_ok(kv_fp8, k_scale, v_scale))
    return (int)hipErrorInvalidValue;
  if (!kv_fp8)
    return launch_prefill<true>(out, out_stride, qkv, row_stride, cu_seqlens, num_seqs,
                                max_seqlen, hq, hkv, hd, scale, ctx_lens, k_cache, v_cache,
                                block_tables, bt_stride, block_size, window, st);
  return launch_prefill<true, fp8>(out, out_stride, qkv, row_stride, cu_seqlens, num_seqs,
                                   max_seqlen, hq, hkv, hd, scale, ctx_lens, k_cache, v_cache,
                                   block_tables, bt_stride, block_size, window, st, k_scale,
                                   v_scale);
}

// 0 / 1: head packing of the short-prompt kernel off / on; returns the previous setting
extern "C" int dli_prefill_set_pack(int on) {
  const int old = g_pf_pack;
  g_pf_pack = on ? 1 : 0;
  return old;
}

extern "C" int dli_prefill_set_min_len(int n) {
  const int old = g_pl_min_len;
  if (n > 0) g_pl_min_len = n;
  return old;
}
