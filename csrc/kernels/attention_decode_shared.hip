// Shared-prefix ("cascade") paged decode attention: bf16 cache, head dim 128, full attention.
//
// The kernels of attention_decode.hip give every (sequence, kv head) item its own walk of its
// own block table, so a system prompt that 512 rows of a decode batch share is streamed 512
// times per layer. Here the KV blocks that many rows share are attended once per TILE of
// sequences, each row's private suffix as before, and the two merge through the split
// workspace of decode_reduce_launch. Three kernels:
//
//   shared_plan_kernel    once per decode step, one workgroup: from block_tables and
//                         context_lens alone, the group of rows that share their first block
//                         with the most other rows, and the P leading blocks all of them
//                         share (the newest token never inside). Device in, device out, so a
//                         captured graph replans on every replay.
//   shared_prefix_kernel  a workgroup per (tile of member sequences, kv head, chunk of the
//                         shared run). A tile stacks NS = 64 / G sequences x G query heads as
//                         64 MFMA columns, one 16-column block per wave; with G = 4 no column
//                         is padding, where the per-item kernels pad 4 heads to 16. The
//                         workgroup stages each 32-token K and V tile of its chunk into LDS
//                         ONCE (double-buffered through registers: the loads of tile t + 1
//                         are in flight while tile t computes, one barrier per tile) and all
//                         four waves compute from that copy, so the run's bytes are read
//                         B / NS times instead of B times:
//                           S^T[tok, col] = K . Q^T   (K rows from LDS as the A operand)
//                           online softmax per column, exp2 domain
//                           O += P . V               (S^T accumulator as the A operand, V by
//                                                     ds_read_b64_tr_b16)
//                         The chunk length follows the run (P bs / chunks, >= 128 tokens) so
//                         a grid fixed at capture time still spreads whatever run a replay
//                         finds over all its chunks.
//   shared_suffix_kernel  a wave per (sequence, kv head): decode_attn_loop over
//                         [lo[b], ctx[b]) as the last split.
//
// Workspace: the (m, l, O) format of dli_decode_attention_workspace_bytes with chunks + 1
// splits. Every slot is written on every launch: a member row's prefix slots by the prefix
// kernel (neutral l = 0, m = -inf, O = 0 where its chunk starts past the run), every other
// row's prefix slots (lo[b] = 0: not a member, or no run) by that row's suffix wave, which
// also writes the suffix slot of every row.
#include "attention_decode.h"

#define SHP_COLS 64            // query columns of a sequence tile: DEC_WAVES x 16
#define SHP_MAX_CHUNKS 16
#define SHP_MIN_CHUNK 128      // tokens
#define SHP_PLAN_THREADS 1024
#define SHP_PLAN_MAX_B 2048

// header = (P bs tokens, member count); members = the member rows ascending, then -1;
// lo[b] = P bs for members, 0 for the rest.
//   live    = rows with context_lens[b] > 0: the rows that pad a captured batch to its bucket
//             (context 0, a table of zeros) take no part, whatever block id 0 is to the others
//   leader  = the live row whose column-0 block id is the most frequent among the live rows,
//             ties to the lowest row
//   members = live rows whose column 0 equals the leader's
//   P       = the largest p with columns 0..p-1 of every member equal to the leader's and
//             p bs <= context_lens[b] - 1 for every member; 0 with fewer than 2 members
__global__ void __launch_bounds__(SHP_PLAN_THREADS) shared_plan_kernel(
    int* __restrict__ header, int* __restrict__ members, int* __restrict__ lo,
    const int* __restrict__ block_tables, int bt_stride, int width,
    const int* __restrict__ context_lens, int B, int block_size) {
  __shared__ int col0[SHP_PLAN_MAX_B];        // -1: not a live row (block ids are >= 0)
  __shared__ unsigned char mem[SHP_PLAN_MAX_B];
  __shared__ int s_best, s_lim, s_p;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int b = tid; b < B; b += nt)
    col0[b] = context_lens[b] > 0 ? block_tables[(long)b * bt_stride] : -1;
  if (tid == 0) { s_best = -1; s_lim = width; s_p = INT_MAX; }
  __syncthreads();
  for (int b = tid; b < B; b += nt) {
    if (col0[b] < 0) continue;
    int cnt = 0;
    for (int j = 0; j < B; ++j) cnt += col0[j] == col0[b];
    atomicMax(&s_best, cnt * SHP_PLAN_MAX_B + (SHP_PLAN_MAX_B - 1 - b));
  }
  __syncthreads();
  const bool any = s_best >= 0;               // false: no live row, no leader
  const int leader = any ? SHP_PLAN_MAX_B - 1 - s_best % SHP_PLAN_MAX_B : 0;
  const int nmem = any ? s_best / SHP_PLAN_MAX_B : 0;
  const int lead0 = col0[leader];
  for (int b = tid; b < B; b += nt) {
    const bool m = any && col0[b] == lead0;
    mem[b] = m;
    if (m) atomicMin(&s_lim, (context_lens[b] - 1) / block_size);
  }
  __syncthreads();
  const int lim = s_lim;                      // no member's run can be longer
  const int* lrow = block_tables + (long)leader * bt_stride;
  for (int idx = tid; idx < B * lim; idx += nt) {
    const int b = idx / lim, c = idx - b * lim;
    if (mem[b] && block_tables[(long)b * bt_stride + c] != lrow[c]) atomicMin(&s_p, c);
  }
  __syncthreads();
  const int pbs = nmem < 2 ? 0 : min(lim, s_p) * block_size;
  for (int b = tid; b < B; b += nt) {
    lo[b] = mem[b] ? pbs : 0;
    if (mem[b]) {
      int pos = 0;
      for (int j = 0; j < b; ++j) pos += mem[j];
      members[pos] = b;
    }
    if (b >= nmem) members[b] = -1;
  }
  if (tid == 0) { header[0] = pbs; header[1] = nmem; }
}

__global__ void __launch_bounds__(64 * DEC_WAVES, 4) shared_prefix_kernel(
    const u16* __restrict__ q, int q_stride, const u16* __restrict__ k_cache,
    const u16* __restrict__ v_cache, const int* __restrict__ block_tables, int bt_stride,
    const int* __restrict__ header, const int* __restrict__ members, int hq, int hkv,
    int block_size, float scale_log2, int num_splits, float* __restrict__ ws_o,
    float* __restrict__ ws_ml) {
  constexpr int HD = 128, KK = HD / 32, DB = HD / 16;
  constexpr int KROW = HD + 8;    // padded LDS row of the K tile, in u16: row r starts 4 banks
                                  // after row r - 1, so the 16 rows a lane group reads with
                                  // 16-B loads cover the 64 banks once
  constexpr int VROW = HD + 16;   // the V tile of decode_attn_loop
  __shared__ __attribute__((aligned(16))) u16 ks[2][DEC_TILE * KROW];
  __shared__ __attribute__((aligned(16))) u16 vs[2][DEC_TILE * VROW];
  const int pbs = header[0], nmem = header[1];
  const int G = hq / hkv, NS = SHP_COLS / G;
  const int tile = blockIdx.x, kvh = blockIdx.y, chunk = blockIdx.z;
  if (pbs <= 0 || tile * NS >= nmem) return;                   // workgroup-uniform
  int ct = (pbs + (int)gridDim.z - 1) / (int)gridDim.z;
  ct = max(SHP_MIN_CHUNK, (ct + DEC_TILE - 1) / DEC_TILE * DEC_TILE);
  const int s_begin = min(pbs, chunk * ct), s_end = min(pbs, s_begin + ct);
  const int ntile = (s_end - s_begin + DEC_TILE - 1) / DEC_TILE;

  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = lane & 15, grp = lane >> 4;
  // this lane's query column: sequence seq of the tile, head `head` of the GQA group
  const int c = 16 * wv + col, seq = c / G, head = c - seq * G;
  const int mi = tile * NS + seq;
  const int b = seq < NS && mi < nmem ? members[mi] : -1;
  bf16x8 qf[KK];
  {
    const u16* qp = q + (long)max(b, 0) * q_stride + (long)(kvh * G + head) * HD;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      uint4 v = b >= 0 ? *reinterpret_cast<const uint4*>(qp + kk * 32 + grp * 8)
                       : make_uint4(0, 0, 0, 0);
      qf[kk] = *reinterpret_cast<bf16x8*>(&v);
    }
  }
  // staging: thread -> 16-B chunk cc of rows r0 and r0 + 16 of the K and of the V tile; the
  // run's block ids are those of any member's row
  const int* btr = block_tables + (long)members[0] * bt_stride;
  const int r0 = threadIdx.x >> 4, cc = threadIdx.x & 15;
  const long kv_head_stride = (long)block_size * HD;
  // (four named registers: as arrays behind a lambda hipcc kept them in scratch)
  uint4 k0, k1, v0, v1;
  auto row_at = [&](int t0, int j) {
    const int tok = min(t0 + r0 + 16 * j, s_end - 1);          // clamp: inside the run
    const int blk = btr[tok / block_size], off = tok % block_size;
    return ((long)blk * hkv + kvh) * kv_head_stride + (long)off * HD + cc * 8;
  };
#define SHP_ISSUE(t0)                                                                  \
  {                                                                                    \
    const long at0 = row_at(t0, 0), at1 = row_at(t0, 1);                               \
    k0 = *reinterpret_cast<const uint4*>(k_cache + at0);                               \
    k1 = *reinterpret_cast<const uint4*>(k_cache + at1);                               \
    v0 = *reinterpret_cast<const uint4*>(v_cache + at0);                               \
    v1 = *reinterpret_cast<const uint4*>(v_cache + at1);                               \
  }
#define SHP_STAGE(buf)                                                                 \
  {                                                                                    \
    *reinterpret_cast<uint4*>(&ks[buf][r0 * KROW + cc * 8]) = k0;                      \
    *reinterpret_cast<uint4*>(&ks[buf][(r0 + 16) * KROW + cc * 8]) = k1;               \
    *reinterpret_cast<uint4*>(&vs[buf][r0 * VROW + cc * 8]) = v0;                      \
    *reinterpret_cast<uint4*>(&vs[buf][(r0 + 16) * VROW + cc * 8]) = v1;               \
  }

  float m_run = -INFINITY, l_part = 0.f;
  f32x4 o_acc[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) o_acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (ntile > 0) {
    SHP_ISSUE(s_begin);
    SHP_STAGE(0);
  }
  __syncthreads();
  const int qrow = (lane >> 2) & 3, pcol = lane & 3;
  for (int t = 0; t < ntile; ++t) {
    const int t0 = s_begin + DEC_TILE * t, buf = t & 1;
    const bool more = t + 1 < ntile;
    if (more) SHP_ISSUE(t0 + DEC_TILE);
    uint4 kreg[2][KK];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        kreg[s][kk] = *reinterpret_cast<const uint4*>(
            &ks[buf][(16 * s + col) * KROW + kk * 32 + grp * 8]);
    f32x4 s_acc[2];
    decode_scores<HD>(kreg, qf, s_acc);
    float p[8];
    decode_softmax_update<HD, false>(s_acc, t0, s_end, grp, scale_log2, m_run, l_part, o_acc, p);
    const bf16x8 pa = decode_pack_p(p);
    const u16* vt = vs[buf];
    // B operand as in decode_attn_loop: rows 4grp + qrow and 16 + 4grp + qrow, columns
    // 16i + 4pcol .. +3, transposed by the read
#pragma unroll
    for (int i = 0; i < DB; ++i) {
      const u16* a0 = vt + (4 * grp + qrow) * VROW + 16 * i + 4 * pcol;
      const u16* a1 = vt + (16 + 4 * grp + qrow) * VROW + 16 * i + 4 * pcol;
      s16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(a0));
      s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (__attribute__((address_space(3))) s16x4*)(a1));
      s16x8 w = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
      o_acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, *reinterpret_cast<bf16x8*>(&w),
                                                        o_acc[i], 0, 0, 0);
    }
    // the other buffer was last read in round t - 1, which every wave left at its barrier
    if (more) SHP_STAGE(buf ^ 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
  }
#undef SHP_ISSUE
#undef SHP_STAGE

  // rows 4grp + r of O are the wave's columns 4grp + r: each its own sequence and head
  const float l_tot = decode_l_total(l_part);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int h = 4 * grp + r;
    const float lr = __shfl(l_tot, h, 64);
    const float mr = __shfl(m_run, h, 64);
    const int br = __shfl(b, h, 64), hr = __shfl(head, h, 64);
    if (br < 0) continue;
    const float inv = lr > 0.f ? 1.f / lr : 0.f;
    const long base = ((long)br * hq + kvh * G + hr) * num_splits + chunk;
    float* wo = ws_o + base * HD;
#pragma unroll
    for (int i = 0; i < DB; ++i) wo[16 * i + col] = o_acc[i][r] * inv;
    if (col == 0) {
      ws_ml[base * 2] = lr > 0.f ? mr : -INFINITY;
      ws_ml[base * 2 + 1] = lr;
    }
  }
}

__global__ void __launch_bounds__(64 * DEC_WAVES, 4) shared_suffix_kernel(
    const u16* __restrict__ q, int q_stride, const u16* __restrict__ k_cache,
    const u16* __restrict__ v_cache, const int* __restrict__ block_tables, int bt_stride,
    const int* __restrict__ context_lens, const int* __restrict__ lo, int B, int hq, int hkv,
    int block_size, float scale_log2, int num_splits, float* __restrict__ ws_o,
    float* __restrict__ ws_ml) {
  constexpr int HD = 128, KK = HD / 32, VROW = HD + 16;
  __shared__ __attribute__((aligned(16))) u16 vtile_all[DEC_WAVES][DEC_TILE * VROW];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int item = blockIdx.x * DEC_WAVES + wv;
  if (item >= B * hkv) return;                                 // wave-uniform exit
  const int kvh = item % hkv, b = item / hkv;
  const int G = hq / hkv;
  const int ctx = max(context_lens[b], 0);
  const int s_begin = __builtin_amdgcn_readfirstlane(min(lo[b], ctx));
  bf16x8 qf[KK];
  load_q_frags<HD>(q, q_stride, b, kvh, G, lane, qf);
  const int bt0 = decode_bt_window(block_tables, bt_stride, b, s_begin, ctx, block_size, lane);
  f32x4 o_acc[HD / 16];
  float m_run, l_part;
  decode_attn_loop<HD>(qf, vtile_all[wv], lane, b, kvh, s_begin, ctx, k_cache, v_cache,
                       block_tables, bt_stride, hkv, block_size, scale_log2, bt0, o_acc, m_run,
                       l_part);
  decode_finalize<HD>(o_acc, m_run, l_part, lane, b, kvh, num_splits - 1, G, hq, num_splits,
                      nullptr, ws_o, ws_ml);
  if (s_begin > 0) return;
  // no shared run for this row: its prefix slots, which no prefix workgroup writes, go neutral
  const int nch = num_splits - 1;
  for (int h = 0; h < G; ++h) {
    const long base = ((long)b * hq + kvh * G + h) * num_splits;
    float4* wo = reinterpret_cast<float4*>(ws_o + base * HD);
    for (int e = lane; e < nch * (HD / 4); e += 64) wo[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = lane; s < nch; s += 64) {
      ws_ml[(base + s) * 2] = -INFINITY;
      ws_ml[(base + s) * 2 + 1] = 0.f;
    }
  }
}

// chunks of the shared run: 0 = automatic, else forced (the probe's sweep). Process-wide and
// read by both the workspace size and the launch: set it before either, never while a captured
// graph that holds these kernels is live (its grid and workspace layout were fixed at capture).
static int g_shared_chunks = 0;
extern "C" int dli_decode_shared_set_chunks(int v) {
  const int old = g_shared_chunks;
  g_shared_chunks = v;
  return old;
}

// Chunks so that tiles x kv heads x chunks workgroups reach 4 per CU (1024), each chunk of
// the longest run (max_context) at least SHP_MIN_CHUNK tokens, at most SHP_MAX_CHUNKS
static int shared_num_chunks(int B, int hq, int hkv, int max_context) {
  if (g_shared_chunks > 0)
    return g_shared_chunks < SHP_MAX_CHUNKS ? g_shared_chunks : SHP_MAX_CHUNKS;
  const int NS = SHP_COLS / (hq / hkv);
  const long items = (long)((B + NS - 1) / NS) * hkv;
  int nch = 1;
  while (items * nch < 1024 && nch < SHP_MAX_CHUNKS && max_context >= 2 * nch * SHP_MIN_CHUNK)
    nch *= 2;
  return nch;
}

static bool shared_shape_ok(int hq, int hkv, int hd, int block_size) {
  return hd == 128 && hkv > 0 && hq % hkv == 0 && hq / hkv <= 16 && block_size > 0 &&
         block_size % 16 == 0;
}

extern "C" long dli_decode_attention_shared_workspace_bytes(int B, int hq, int hkv, int hd,
                                                            int max_context) {
  if (B <= 0 || !shared_shape_ok(hq, hkv, hd, 16)) return 0;
  const int splits = shared_num_chunks(B, hq, hkv, max_context) + 1;
  return (long)B * hq * splits * (hd + 2) * (long)sizeof(float);
}

// header [2], members [B], lo [B] (int32, device) from block_tables [B, width] (row stride
// bt_stride) and context_lens [B]
extern "C" int dli_decode_shared_plan(int* header, int* members, int* lo,
                                      const int* block_tables, int bt_stride, int width,
                                      const int* context_lens, int B, int block_size,
                                      hipStream_t st) {
  if (B <= 0) return 0;
  if (B > SHP_PLAN_MAX_B || width < 1 || block_size < 1) return (int)hipErrorInvalidValue;
  shared_plan_kernel<<<1, SHP_PLAN_THREADS, 0, st>>>(header, members, lo, block_tables,
                                                     bt_stride, width, context_lens, B,
                                                     block_size);
  DLI_RETURN_LAUNCH();
}

// dli_decode_attention for a bf16 cache, head dim 128 and full attention with the plan of
// dli_decode_shared_plan; workspace: dli_decode_attention_shared_workspace_bytes
extern "C" int dli_decode_attention_shared(void* out, const void* q, int q_stride,
                                           const void* k_cache, const void* v_cache,
                                           const int* block_tables, int bt_stride,
                                           const int* context_lens, const int* header,
                                           const int* members, const int* lo, int B, int hq,
                                           int hkv, int hd, int block_size, float scale,
                                           int max_context, void* workspace, hipStream_t st) {
  if (B <= 0) return 0;
  if (!shared_shape_ok(hq, hkv, hd, block_size) || workspace == nullptr)
    return (int)hipErrorInvalidValue;
  const int nch = shared_num_chunks(B, hq, hkv, max_context), splits = nch + 1;
  const int NS = SHP_COLS / (hq / hkv);
  const float scale_log2 = scale * 1.4426950408889634f;
  float* ws_o = (float*)workspace;
  float* ws_ml = ws_o + (long)B * hq * splits * hd;
  dim3 gp((B + NS - 1) / NS, hkv, nch);
  shared_prefix_kernel<<<gp, 64 * DEC_WAVES, 0, st>>>(
      (const u16*)q, q_stride, (const u16*)k_cache, (const u16*)v_cache, block_tables,
      bt_stride, header, members, hq, hkv, block_size, scale_log2, splits, ws_o, ws_ml);
  const long items = (long)B * hkv;
  shared_suffix_kernel<<<(int)((items + DEC_WAVES - 1) / DEC_WAVES), 64 * DEC_WAVES, 0, st>>>(
      (const u16*)q, q_stride, (const u16*)k_cache, (const u16*)v_cache, block_tables,
      bt_stride, context_lens, lo, B, hq, hkv, block_size, scale_log2, splits, ws_o, ws_ml);
  return decode_reduce_launch(out, ws_o, ws_ml, B, hq, hd, splits, st);
}
