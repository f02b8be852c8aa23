// filter_search.hip — list scan and coarse quantizer on the matrix cores: MFMA ranking (bf16 x 3 split
// arithmetic by default, f32 MFMA with VI_FILTER_BF16=0), and the pipeline that runs a search through it.  The exact-order
// re-evaluation of the few vectors that can be results is the select phase (select.hip).
//
// The exact-order VALU scan (search_kernels.hip) spends 3 vector ops per (query, vector, dim) and is
// bound by f32 VALU issue.  When many queries of a batch probe the same list, (queries x vectors x
// dims) is GEMM shaped: the matrix cores can RANK the candidates, and only the handful that can
// reach the top-k need the reference's exact arithmetic (src/utils.rs:28-30).
//
//   1. rank      per work item (list segment of <= segb blocks, group of <= 128 queries):
//                m(q,v) = ||v||^2 - 2 q.v on the matrix cores (A = 64 vectors staged in LDS, B = the group's
//                queries in registers, accumulator initialised with ||v||^2): v_mfma_f32_32x32x16_bf16 on
//                operands split hi + lo (hi.hi + hi.lo + lo.hi, mfma_bf16.hpp), or v_mfma_f32_32x32x2_f32.
//                A lane owns one query and 32 of the 64 rows of every block: the 16 accumulator registers of each
//                of the two 32-row tiles, a SUB-BLOCK of 16 rows.  All that is kept of a sub-block is its minimum
//                (8 v_min3_f32): two blocks' four minima form a 16-byte PAIR RECORD, and the four smallest minima
//                of the segment, T0 <= T1 <= T2 <= T3 (a v_med3_f32 network, no positions), a GROUP RECORD — no
//                thresholds, no atomics, no candidate lists, no index bits stolen from the values, nothing that can
//                overflow.  (Round 1 kept the four smallest rows of every 32 with their indices in the low mantissa
//                bits: 226 vector instructions and 16 B per block and lane against 28 and 8 B now.)
//   2. select    one wave per query turns its records into the exact top-k (select.hip, where the margin that makes
//                the rank values sufficient is derived).
//
// The coarse quantizer (ivf_index.rs:205-220) is the same computation with the centroid table as one
// list probed by every query and K = n_probe.
//
// Host side: the dispatcher (search.hip) hands the pipelines their SearchBatch; which rank kernel it takes is decided first (RankPlan).
// ("filter" in this file's name, its kernels and the VI_FILTER variables is the engine's first name; in host code it means a SlotFilter.)
// The grouping between the coarse step and the rank, and the kernels that build the rank work items, are grouping.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device_index.hpp"
#include "device_math.hpp"
#include "grouping.hpp"
#include "mfma_bf16.hpp"
#include "rank_stream.hpp"
#include "scan.hpp"
#include "search_internal.hpp"
#include "select.hpp"
#include "slot_filter.hpp"
#include "wave_sort.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;
constexpr double kApproxRatio = 0.04;  // rank_approx_mode: margin unit / list spread up to which the hi planes alone rank

// ------------------------------------------------------------------------------------------
// record bookkeeping: where the records of (query, probe) start
// ------------------------------------------------------------------------------------------
// rel[q*P+r] = group records of the query's probes before rank r ; qtot[q] = group records of the query
__global__ void pair_groups_kernel(const uint32_t *probes, const uint32_t *list_len, uint32_t nq, uint32_t P,
                                   uint32_t segb0, uint32_t *rel, uint32_t *qtot) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  uint32_t run = 0;
  for (uint32_t r = 0; r < P; ++r) {
    const uint32_t l = probes[(size_t)q * P + r];
    rel[(size_t)q * P + r] = run;
    if (l != kNoPos) {
      uint32_t sb;
      run += 2u * list_segments(list_len[l], segb0, &sb);
    }
  }
  qtot[q] = run;
}

__global__ void iota_kernel(uint32_t *p, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = i;
}

// ------------------------------------------------------------------------------------------
// rank kernel
// ------------------------------------------------------------------------------------------
struct FilterArgs {
  const float4 *blocks;  // f32 blocks, or the bf16 hi/lo image of the same size (BF16 kernels)
  const float *xnorm;
  uint32_t dq, dim;
  const float *Q;
  const uint32_t *first_block, *list_len, *item_start, *seg_start, *pairs;
  uint32_t nlists, P, segb0;
  const uint32_t *qoff, *rel;  // group-record offsets (lists) ...
  uint32_t rec_stride;         // ... or a fixed number of records per slot when qoff is null (coarse table)
  const uint32_t *tile_start;  // pair records: first record tile (2 * GQ records) of each list
  const uint4 *items;          // list phase: the work items' descriptors (item_desc_kernel), or null: derived here
  float4 *gval;                // group records: the four smallest sub-block minima of a (pair, segment, lane half)
  uint32_t *gmeta;             // ... and where the record belongs: probe rank | segment << 6 | lane half << 13
  float4 *brec;                // pair records: the sub-block minima of two blocks
  const uint4 *qimg;  // bf16 ranking: -2 q of the batch split hi / lo once per search (split_queries_kernel)
  uint32_t direct;  // coarse table only: records = the minima of the 8-row sub-blocks of every block, no group records
  uint32_t xmode;  // experiment knob (VI_FILTER_XMODE): 1 = do not restage tiles, 2 = no ranking epilogue
};

// Workgroup = 4 waves = up to 128 queries (4 column tiles of 32) probing ONE list segment.  Every
// 64-vector block of the segment is copied once per workgroup into LDS by LDS-DMA (global_load_lds_dwordx4:
// no staging registers, no ds_write) and consumed by all four waves.  The LDS image is the block verbatim —
// [quad][vector] float4, so a lane's A fragment (quad 2g+h of vector j) is a conflict-free ds_read_b128 —
// followed by the block's 64 squared norms.  With NBUF = 2 the next block lands in the other buffer while
// this one is multiplied (one barrier per block); with NBUF = 1 the load is exposed and hidden by the other
// workgroups of the CU (3 per CU instead of 2).
// registers r0 .. r0+7 of an accumulator tile (an 8-row sub-block): the smallest value with its row in the 3 low
// mantissa bits (|packed - m| < 2^-20 |m|) and the second smallest — 3 instructions per element
__device__ __forceinline__ float2 tile_min8_idx(const f32x16 &a, int r0) {
  float b1 = INFINITY, b2 = INFINITY;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float p = __uint_as_float((__float_as_uint(a[r0 + e]) & ~7u) | (uint32_t)e);
    b2 = __builtin_amdgcn_fmed3f(b1, b2, p);
    b1 = min3_raw(b1, p, p);
  }
  return make_float2(b1, b2);
}
// one block image -> LDS: all of it, or (RANK 2) only its hi planes: pieces (chunk c, plane 0, half h) = 4c + h
template <int NG, int RANK, int NBUF, int WAVES>
__device__ __forceinline__ void tile_dma_rank(float *tile, const float4 *src, const float *xn, int wave, int lane) {
  if constexpr (RANK != 2) {
    if constexpr (NBUF >= 2) tile_dma_image_asm<NG, WAVES>(tile, src, xn, wave, lane);  // the loop places its own waits
    else tile_dma_image<NG, WAVES>(tile, src, xn, wave, lane);
  } else {
#pragma unroll
    for (int i0 = 0; i0 < NG; i0 += WAVES) {
      const int i = i0 + wave;
      if (i < NG) {
        const int piece = 4 * (i >> 1) + (i & 1);  // hi piece i = 2c + h lands compactly at i
        glds16_asm(src + piece * 64 + lane, tile + i * 256);
      }
    }
    if (wave == 0) glds4_asm(xn + lane, tile + NG * 256);  // (asm: the double-buffered loop places its own waits)
  }
}

__global__ void split_queries_kernel(const float *Q, uint32_t nq, uint32_t dim, uint32_t nc, uint4 *out, unsigned long long *any_lo,
                                     uint32_t *zero, uint32_t zero_words, const float *mu, uint2 *out8, unsigned long long *not_i8,
                                     uint64_t *counts);

// NG = dq/2 exactly: a block holds 2*NG quads (dims padded to 16); dim % 4 == 0.  TABLE only names the instance
// that ranks the centroid table (coarse step), so that profiles tell it from the list scan.
// RANK 0: f32 MFMA (eight per 16 dims).  RANK 1: three bf16 MFMAs per 16 dims (hi.hi + hi.lo + lo.hi).
// RANK 2: the stored values are bf16-exact (every lo plane is zero: 8-bit descriptors such as SIFT) — only the hi
// planes are staged (half the bytes) and lo.hi is dropped; hi.lo is dropped too for a wave whose 32 queries are
// bf16-exact (wave-uniform test), which leaves ONE MFMA per 16 dims with the result still exact to f32 rounding.
// GQ = queries per work item: 128 (4 waves) when lists are probed by many queries of the batch, 32 (one wave per
// workgroup, up to 9 workgroups per CU) when a list is probed by a handful — large balanced indexes, where a
// 128-query group would leave three of its four waves idle behind the same tile stream.
template <int NG, int NBUF, bool TABLE, int RANK, int GQ>
__global__ void __launch_bounds__(GQ * 2, GQ == 32 ? (RANK == 2 ? 2 : 1) : ((NBUF == 1 || RANK == 2) ? 3 : 2))
    filter_kernel(FilterArgs a) {  // (second bound = waves per SIMD the register allocation must allow)
  constexpr int WAVES = GQ / 32;
  constexpr int kImage = (RANK == 2 ? NG : 2 * NG) * 256;  // floats of the staged image (RANK 2: hi planes only)
  constexpr int kTileFloats = kImage + 64;                 // + the block's 64 norms
  __shared__ __attribute__((aligned(16))) float s_tiles[NBUF][kTileFloats];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const uint32_t item = blockIdx.x;  // grid == number of items
  uint32_t pair0, nqi, fb, b0, b1, seg, rec0, chunk = 0, nblk = 0;
  if (!TABLE && a.items) {
    const uint4 d0 = a.items[2 * (size_t)item], d1 = a.items[2 * (size_t)item + 1];
    pair0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d0.x); nqi = (uint32_t)__builtin_amdgcn_readfirstlane((int)d0.y);
    fb = (uint32_t)__builtin_amdgcn_readfirstlane((int)d0.z); b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d0.w);
    b1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d1.x); seg = (uint32_t)__builtin_amdgcn_readfirstlane((int)d1.y);
    rec0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d1.z);
  } else {
    uint32_t lo = 0, hi = a.nlists;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.item_start[mid] <= item) lo = mid; else hi = mid;
    }
    const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    const uint32_t s0 = a.seg_start[l], cnt = a.seg_start[l + 1] - s0;
    const uint32_t len = a.list_len[l];
    uint32_t segb;
    const uint32_t nseg = list_segments(len, a.segb0, &segb);
    const uint32_t local = item - a.item_start[l];
    chunk = local / nseg;
    seg = local - chunk * nseg;
    const uint32_t j0 = chunk * GQ;
    pair0 = s0 + j0;
    nqi = min((uint32_t)GQ, cnt - j0);
    fb = a.first_block[l];
    nblk = (len + kWave - 1) / kWave;
    b0 = seg * segb;
    b1 = min(nblk, b0 + segb);
    // tile_start counts the record tiles of the lists before this one: chunks x segments x seg_records
    rec0 = a.tile_start[l] + (chunk * nseg + seg) * seg_records(segb);
  }

  // the first tile is requested before the queries are fetched: both latencies run together
  tile_dma_rank<NG, RANK, NBUF, WAVES>(s_tiles[0], a.blocks + ((size_t)(fb + b0) * a.dq) * kWave, a.xnorm + (size_t)(fb + b0) * kWave, wave, lane);

  // ---- this lane's query: both lane halves hold query j of the wave's tile ----
  // the tile a wave owns rotates with the item so that partially filled groups do not always idle the same SIMD
  const uint32_t wtile = ((uint32_t)wave + item) % (uint32_t)WAVES;
  const uint32_t jq_grp = 32u * wtile + (uint32_t)j;
  const bool qlive = jq_grp < nqi;
  const bool wave_live = 32u * wtile < nqi;  // wave-uniform
  const uint32_t slot = qlive ? a.pairs[pair0 + jq_grp] : 0u;
  const uint32_t qid = slot / a.P;
  const float *qrow = a.Q + (size_t)qid * a.dim;
  float4 qf[NG];  // f32: -2q, dims 8g+4h.. ; BF16: qf[2c] = hi, qf[2c+1] = lo halves (bit patterns) of -2q, dims 16c+8h..
  constexpr bool BF16 = RANK != 0;
  bool q_lo_zero = false;  // RANK 2: every query of this wave splits with lo = 0
  if (!BF16) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const uint32_t e = 8 * g + 4 * h;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (qlive && e < a.dim) v = *reinterpret_cast<const float4 *>(qrow + e);
      qf[g] = make_float4(-2.f * v.x, -2.f * v.y, -2.f * v.z, -2.f * v.w);
    }
  } else {
    // the batch's queries were split once (every query sits in n_probe work items): 16-byte pieces, no arithmetic here
    const uint4 *qi = a.qimg + (size_t)qid * (NG / 2) * 4 + h;  // [plane][chunk][half]
#pragma unroll
    for (int c = 0; c < NG / 2; ++c) {
      uint4 hi = make_uint4(0u, 0u, 0u, 0u), lo = hi;
      if (qlive) { hi = qi[c * 2]; lo = qi[NG + c * 2]; }
      qf[2 * c] = __builtin_bit_cast(float4, hi);
      qf[2 * c + 1] = __builtin_bit_cast(float4, lo);
    }
  }
  if constexpr (RANK == 2) {
    uint32_t any = 0;
#pragma unroll
    for (int c = 0; c < NG / 2; ++c) {
      const uint4 lo = __builtin_bit_cast(uint4, qf[2 * c + 1]);
      any |= lo.x | lo.y | lo.z | lo.w;
    }
    q_lo_zero = __ballot((any & 0x7FFF7FFFu) != 0u) == 0ull;  // (-0 halves are zero too)
  }

  float T0 = INFINITY, T1 = INFINITY, T2 = INFINITY, T3 = INFINITY;  // four smallest sub-block minima of the segment
  float4 w = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);    // the pair record being filled
  // pair records are item-major — [record tile = (query group, segment, pair of blocks)][lane half][query of the
  // group] — so that a wave's 32 queries store 512 contiguous bytes (record counts are checked < 2^32 on the host);
  const uint32_t bi = rec0 * (2u * GQ) + (uint32_t)GQ * (uint32_t)h + jq_grp;

  // LDS-DMA instructions this wave issues per tile (RANK 2: its share of the NG hi pieces; wave 0 also the norms)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pieces have landed ...
  __syncthreads();                                   // ... and so have everyone else's
  for (uint32_t blk = b0; blk < b1; ++blk) {
    const bool more = (blk + 1 < b1) && !(a.xmode & 1u);
    uint32_t nstores = 0;  // record stores this lane issued in this iteration
    const float *s_tile = s_tiles[NBUF == 2 ? ((blk - b0) & 1u) : 0];
    // next block: lands in the other buffer during this block's MFMAs (every wave left that buffer at the
    // barrier that ended the previous iteration)
    if (NBUF == 2 && more)
      tile_dma_rank<NG, RANK, NBUF, WAVES>(s_tiles[((blk - b0) & 1u) ^ 1u], a.blocks + ((size_t)(fb + blk + 1) * a.dq) * kWave,
                   a.xnorm + (size_t)(fb + blk + 1) * kWave, wave, lane);
    if (wave_live) {
      // both row tiles (vectors 0..31 and 32..63) advance together: two independent accumulator chains
      f32x16 acc0, acc1;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {  // rows 8*q4 + 4*h + (0..3) live in regs 4*q4 .. 4*q4+3
        const float4 n0 = *reinterpret_cast<const float4 *>(s_tile + kImage + 8 * q4 + 4 * h);
        const float4 n1 = *reinterpret_cast<const float4 *>(s_tile + kImage + 32 + 8 * q4 + 4 * h);
        acc0[4 * q4 + 0] = n0.x; acc0[4 * q4 + 1] = n0.y; acc0[4 * q4 + 2] = n0.z; acc0[4 * q4 + 3] = n0.w;
        acc1[4 * q4 + 0] = n1.x; acc1[4 * q4 + 1] = n1.y; acc1[4 * q4 + 2] = n1.z; acc1[4 * q4 + 3] = n1.w;
      }
      if constexpr (!BF16) {
        // A fragments are read one K group ahead of the MFMAs that consume them (the compiler would otherwise
        // issue each pair of ds_read_b128 right before its 8 MFMAs and stall on the LDS latency every time)
        float4 a0 = *reinterpret_cast<const float4 *>(s_tile + h * 256 + 4 * j);
        float4 a1 = *reinterpret_cast<const float4 *>(s_tile + h * 256 + 4 * (32 + j));
#pragma unroll
        for (int g = 0; g < NG; ++g) {
          float4 n0 = a0, n1 = a1;
          if (g + 1 < NG) {
            n0 = *reinterpret_cast<const float4 *>(s_tile + (2 * (g + 1) + h) * 256 + 4 * j);
            n1 = *reinterpret_cast<const float4 *>(s_tile + (2 * (g + 1) + h) * 256 + 4 * (32 + j));
          }
          __builtin_amdgcn_sched_barrier(0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, qf[g].x, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, qf[g].x, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, qf[g].y, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, qf[g].y, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, qf[g].z, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, qf[g].z, acc1, 0, 0, 0);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, qf[g].w, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, qf[g].w, acc1, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          a0 = n0;
          a1 = n1;
        }
      } else {
        // image: [chunk][plane][half][vector] x 16 B; fragment (plane p, tile t) of chunk c for lane (j,h) =
        // float4 index ((c*2 + p)*2 + h)*64 + 32t + j
        auto frag = [&](int c, int p, int t) {  // RANK 2 stages the hi pieces compactly: piece 2c + h
          const int piece = RANK == 2 ? 2 * c + h : (c * 2 + p) * 2 + h;
          return __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4 *>(s_tile + (piece * 64 + 32 * t + j) * 4));
        };
        if constexpr (RANK == 1) {
          // hi fragments of chunk c+1 are requested while the lo MFMAs of chunk c run, lo fragments of chunk c
          // while its hi MFMAs run: 16 fragment registers, every read has MFMAs to hide behind
          bf16x8 h0 = frag(0, 0, 0), h1 = frag(0, 0, 1);
#pragma unroll
          for (int c = 0; c < NG / 2; ++c) {
            const bf16x8 bh = __builtin_bit_cast(bf16x8, qf[2 * c]), bl = __builtin_bit_cast(bf16x8, qf[2 * c + 1]);
            const bf16x8 l0 = frag(c, 1, 0), l1 = frag(c, 1, 1);
            __builtin_amdgcn_sched_barrier(0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, bh, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, bh, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, bl, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, bl, acc1, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (c + 1 < NG / 2) { h0 = frag(c + 1, 0, 0); h1 = frag(c + 1, 0, 1); }
            __builtin_amdgcn_sched_barrier(0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(l0, bh, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(l1, bh, acc1, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
          }
        } else {
          // stored values are bf16-exact: hi planes only
          bf16x8 h0 = frag(0, 0, 0), h1 = frag(0, 0, 1);
#pragma unroll
          for (int c = 0; c < NG / 2; ++c) {
            const bf16x8 bh = __builtin_bit_cast(bf16x8, qf[2 * c]), bl = __builtin_bit_cast(bf16x8, qf[2 * c + 1]);
            __builtin_amdgcn_sched_barrier(0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, bh, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, bh, acc1, 0, 0, 0);
            if (!q_lo_zero) {  // wave-uniform
              acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, bl, acc0, 0, 0, 0);
              acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, bl, acc1, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (c + 1 < NG / 2) { h0 = frag(c + 1, 0, 0); h1 = frag(c + 1, 0, 1); }  // requested behind the MFMAs
          }
        }
      }
      if (TABLE && a.direct) {
        // the coarse table (<= 256 blocks): per block and lane the four 8-row sub-blocks' (minimum with its row, second
        // minimum) go out as they are — two 16-byte records; the select reads all of a query's records at once
        // (coarse_select_direct_kernel) and re-evaluates ONE row per candidate sub-block unless the second minimum
        // can matter too
        nstores = qlive ? 2u : 0u;
        if (qlive) {
          const float2 s00 = tile_min8_idx(acc0, 0), s01 = tile_min8_idx(acc0, 8), s10 = tile_min8_idx(acc1, 0), s11 = tile_min8_idx(acc1, 8);
          // query-major: the select reads a query's records as 1 KB runs (these stores pay for it: 32 queries x 32 bytes each)
          float4 *dst = a.brec + ((size_t)chunk * GQ + jq_grp) * (4u * nblk) + 4u * blk + (uint32_t)h;
          dst[0] = make_float4(s00.x, s00.y, s01.x, s01.y);
          dst[2] = make_float4(s10.x, s10.y, s11.x, s11.y);
        }
      } else if (!(a.xmode & 2u)) {
        // all that is kept of the two 16-row sub-blocks: their minima
        const float m0 = tile_min(acc0), m1 = tile_min(acc1);
        VI_TOP4(m0) VI_TOP4(m1)
        if (((blk - b0) & 1u) == 0u) { w.x = m0; w.y = m1; w.z = INFINITY; w.w = INFINITY; }
        else { w.z = m0; w.w = m1; }
        if (((blk - b0) & 1u) != 0u || blk + 1 == b1) {  // the pair is complete (wave-uniform)
          nstores = (qlive && !(a.xmode & 8u)) ? 1u : 0u;
          if (nstores) a.brec[(size_t)bi + (2u * GQ) * ((blk - b0) >> 1)] = w;
        }
      }
    }
    if (NBUF == 1) {
      __syncthreads();  // every wave is done reading the tile
      if (more)
        tile_dma_rank<NG, RANK, NBUF, WAVES>(s_tiles[0], a.blocks + ((size_t)(fb + blk + 1) * a.dq) * kWave,
                     a.xnorm + (size_t)(fb + blk + 1) * kWave, wave, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();  // next tile visible
    } else {
      // The next tile's LDS-DMA was issued before this block's MFMAs; the only younger vector-memory operation
      // are this wave's record stores of this block, if it made any (vmcnt counts loads, stores and LDS-DMA together, in issue order).
      // Waiting for all but that store keeps the store's latency off the critical path; __syncthreads() would
      // insert vmcnt(0), hence the raw barrier (LDS reads of this tile are complete: lgkmcnt(0)).
      // (a store instruction is issued iff some lane of the wave stores: the ballots are the wave-uniform form of that)
      const uint32_t st_ops = __ballot(nstores == 2u) != 0ull ? 2u : (__ballot(nstores == 1u) != 0ull ? 1u : 0u);
      if (st_ops == 2u) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else if (st_ops == 1u) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // next tile visible; this tile free to be overwritten
    }
  }
  if (qlive && !(TABLE && a.direct)) {
    const size_t gi = (a.qoff ? (size_t)a.qoff[qid] + a.rel[slot] : (size_t)slot * a.rec_stride) + 2u * seg + (uint32_t)h;
    a.gval[gi] = make_float4(T0, T1, T2, T3);
    a.gmeta[gi] = (slot - qid * a.P) | (seg << 6) | ((uint32_t)h << 13);  // where the record belongs
  }
}

// ------------------------------------------------------------------------------------------
// rank kernel for wide vectors (128 < D <= 1536)
// ------------------------------------------------------------------------------------------
// Above 128 dimensions the queries of a group no longer fit in registers for a whole work item, so the ranking becomes
// a GEMM proper: per workgroup a C tile of 4 blocks (256 vectors) x 128 queries stays in the accumulators (128 VGPRs
// per wave) while BOTH operands stream through LDS in K steps of 32 dimensions — 32 KB of the blocks' bf16 hi/lo image
// and 16 KB of the queries' (gathered by LDS-DMA with per-lane row addresses from a query-major image of the batch,
// split once per search), double buffered: 97 KB of LDS, one workgroup per CU, 24 MFMAs per wave and 16-dim chunk.
// What a C tile leaves behind is what filter_kernel leaves: sub-block minima in pair records and the segment's four
// smallest in a group record, so the select is the same kernel.
constexpr int kWideBlocks = 4;
constexpr int kWideChunks = 2;
constexpr int kWideBufFloats = (kWideBlocks + 2) * kWideChunks * 4 * 256;  // A: 4 blocks, B: 2 query blocks; x chunks x 4 pieces x 1 KB
constexpr int kWideLdsFloats = 2 * kWideBufFloats + kWideBlocks * 64;      // two buffers + the norms of the C tile's blocks (97 KB)

struct WideArgs {
  const uint4 *img;      // bf16 hi/lo image of the lists: per block nc chunks x [plane][half] x 64 columns x 16 B
  const float *xnorm;    // squared norms in image-column order
  const uint4 *qimg;     // query-major image of the batch: [query][nc][plane][half] x 16 B of -2 q split hi / lo
  uint32_t nc;           // 16-dim chunks per vector
  const uint32_t *first_block, *list_len, *item_start, *seg_start, *pairs, *item_list;
  uint32_t P, segb0;
  const uint32_t *qoff, *rel, *tile_start;
  float4 *gval;
  uint32_t *gmeta;
  float4 *brec;
};

// -2 q split hi / lo, query-major, hi plane first: piece (plane p, chunk c, half h) of query q at q * 4 nc + p * 2 nc + 2 c + h
// (a batch of bf16-exact queries is ranked from its hi planes alone: they are whole cache lines of their own)
// *any_lo is raised when some query has a non-zero lo plane (a batch of bf16-exact queries is ranked without them)
// (`zero`: a buffer the next kernels count into — the coarse step's per-list histogram — cleared here instead of by a memset launch)
// mu (or null): the centre of the ranking images (DeviceIndex::centre) — the image is then that of -2 fl(q - mu)
// out8 (or null: the lists have no int8 image): the int8 image of the batch for rank_stream_i8_kernel, q - 127 (0 past
// dim), 32 ceil(dim / 32) bytes per query in dimension order; *not_i8 is raised when some value is not an integer in
// 0..254 (the batch is then ranked with bf16)
// counts: ws.stats — the grouping's counts (words [0, kStatListCounts) and kStatTiles128) are cleared here, for a grouping
// whose every workgroup adds to them (list_totals_kernel with GroupScanArgs: no kernel of that chain can clear them first)
__global__ void split_queries_kernel(const float *Q, uint32_t nq, uint32_t dim, uint32_t nc, uint4 *out, unsigned long long *any_lo,
                                     uint32_t *zero, uint32_t zero_words, const float *mu, uint2 *out8, unsigned long long *not_i8,
                                     uint64_t *counts) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (query, chunk, half)
  for (uint64_t i = t; i < zero_words; i += (uint64_t)gridDim.x * blockDim.x) zero[i] = 0u;
  if (t < kStatListCounts + 1) counts[t < kStatListCounts ? t : kStatTiles128] = 0;
  if (t >= (uint64_t)nq * nc * 2) return;
  const uint32_t h = (uint32_t)(t & 1u);
  const uint64_t qc = t >> 1;
  const uint32_t c = (uint32_t)(qc % nc);
  const uint64_t q = qc / nc;
  const uint32_t e = 16 * c + 8 * h;
  const float *row = Q + q * dim;
  float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
  if (e < dim) v0 = *reinterpret_cast<const float4 *>(row + e);        // dim % 4 == 0
  if (e + 4 < dim) v1 = *reinterpret_cast<const float4 *>(row + e + 4);
  if (out8) {
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    uint32_t w[2] = {0u, 0u};
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (e + (uint32_t)i < dim) {
        ok = ok && x[i] >= 0.0f && x[i] <= 254.0f && x[i] == floorf(x[i]);
        w[i >> 2] |= (((uint32_t)(int)x[i] - 127u) & 0xFFu) << (8 * (i & 3));
      }
    }
    if (!ok) w[0] = w[1] = 0u;
    const uint64_t row8 = q * (uint64_t)(nc + (nc & 1u)) * 2u;  // uint2 words per query: 32 ceil(dim / 32) bytes
    out8[row8 + e / 8] = make_uint2(w[0], w[1]);
    if ((nc & 1u) && c == nc - 1) out8[row8 + e / 8 + 2] = make_uint2(0u, 0u);  // the zero half of the last 32-dimension chunk
    if (__ballot(!ok) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(not_i8, 1ull);
  }
  if (mu) {
    if (e < dim) { const float4 m = *reinterpret_cast<const float4 *>(mu + e); v0.x -= m.x; v0.y -= m.y; v0.z -= m.z; v0.w -= m.w; }
    if (e + 4 < dim) { const float4 m = *reinterpret_cast<const float4 *>(mu + e + 4); v1.x -= m.x; v1.y -= m.y; v1.z -= m.z; v1.w -= m.w; }
  }
  uint4 hi, lo;
  split8(v0, v1, -2.0f, hi, lo);
  out[q * 4 * nc + 2 * c + h] = hi;
  out[q * 4 * nc + 2 * nc + 2 * c + h] = lo;
  if (__ballot(((lo.x | lo.y | lo.z | lo.w) & 0x7FFF7FFFu) != 0u) != 0ull && (threadIdx.x & 63u) == 0u)  // (-0 halves are zero too)
    atomicOr(any_lo, 1ull);
}

__global__ void __launch_bounds__(256, 1) rank_wide_kernel(WideArgs a) {
  extern __shared__ __attribute__((aligned(16))) float s_wide[];
  float *s_norm = s_wide + 2 * kWideBufFloats;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const uint32_t item = blockIdx.x;
  const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)a.item_list[item]);
  const uint32_t s0 = a.seg_start[l], cnt = a.seg_start[l + 1] - s0;
  const uint32_t len = a.list_len[l];
  uint32_t segb;
  const uint32_t nseg = list_segments(len, a.segb0, &segb);
  const uint32_t local = item - a.item_start[l];
  const uint32_t chunk = local / nseg, seg = local - chunk * nseg;
  const uint32_t j0 = chunk * kGroupQ;
  const uint32_t nqi = min((uint32_t)kGroupQ, cnt - j0);
  const uint32_t fb = a.first_block[l];
  const uint32_t nblk = (len + kWave - 1) / kWave;
  const uint32_t b0 = seg * segb, b1 = min(nblk, b0 + segb);
  const uint32_t nc = a.nc, nslab = (nc + kWideChunks - 1) / kWideChunks;

  // this lane's query (both lane halves hold query j of the wave's tile), and the two queries it gathers for the B tiles
  const uint32_t wtile = ((uint32_t)wave + item) & 3u;
  const uint32_t jq_grp = 32u * wtile + (uint32_t)j;
  const bool qlive = jq_grp < nqi;
  const bool wave_live = 32u * wtile < nqi;
  const uint32_t slot = qlive ? a.pairs[s0 + j0 + jq_grp] : 0u;
  const uint32_t qid = slot / a.P;
  uint32_t gq[2];  // query of column `lane` of query block 0 / 1
#pragma unroll
  for (int qb = 0; qb < 2; ++qb) {
    const uint32_t col = 64u * qb + (uint32_t)lane;
    gq[qb] = col < nqi ? a.pairs[s0 + j0 + col] / a.P : 0u;
  }

  float T0 = INFINITY, T1 = INFINITY, T2 = INFINITY, T3 = INFINITY;
  const uint32_t bi = (a.tile_start[l] + (chunk * nseg + seg) * seg_records(segb)) * (2u * kGroupQ) + (uint32_t)kGroupQ * (uint32_t)h + jq_grp;

  // one K step (slab s of the C tile at blk0) into buffer `buf`: 32 A pieces + 16 B pieces of 1 KB, 12 per wave
  auto stage = [&](uint32_t blk0, uint32_t s, float *buf) {
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      const int pi = wave + 4 * i;
      if (pi < 32) {
        const uint32_t blk = (uint32_t)pi >> 3, c = ((uint32_t)pi >> 2) & 1u, piece = (uint32_t)pi & 3u;
        const uint32_t cc = s * kWideChunks + c;
        if (blk0 + blk < b1 && cc < nc)
          glds16_asm(a.img + (((size_t)(fb + blk0 + blk) * nc + cc) * 4 + piece) * kWave + lane, buf + pi * 256);
      } else {
        const uint32_t r = (uint32_t)pi - 32u, qb = r >> 3, c = (r >> 2) & 1u, piece = r & 3u;
        const uint32_t cc = s * kWideChunks + c;
        if (cc < nc) glds16_asm(a.qimg + (size_t)gq[qb] * nc * 4 + (piece >> 1) * 2 * nc + cc * 2 + (piece & 1u), buf + pi * 256);
      }
    }
  };

  for (uint32_t blk0 = b0; blk0 < b1; blk0 += kWideBlocks) {
    const uint32_t nb = min((uint32_t)kWideBlocks, b1 - blk0);  // blocks of this C tile
    stage(blk0, 0, s_wide);
    if ((uint32_t)wave < nb) glds4_asm(a.xnorm + (size_t)(fb + blk0 + wave) * kWave + lane, s_norm + wave * 64);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    f32x16 acc[kWideBlocks][2];
#pragma unroll
    for (int b = 0; b < kWideBlocks; ++b)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {  // rows 8*q4 + 4*h + (0..3) of tile t live in regs 4*q4 .. 4*q4+3
          const float4 n = *reinterpret_cast<const float4 *>(s_norm + b * 64 + 32 * t + 8 * q4 + 4 * h);
          acc[b][t][4 * q4 + 0] = n.x; acc[b][t][4 * q4 + 1] = n.y; acc[b][t][4 * q4 + 2] = n.z; acc[b][t][4 * q4 + 3] = n.w;
        }
    for (uint32_t s = 0; s < nslab; ++s) {
      const float *buf = s_wide + (s & 1u) * kWideBufFloats;
      if (s + 1 < nslab) stage(blk0, s + 1, s_wide + ((s + 1u) & 1u) * kWideBufFloats);
      if (wave_live) {
        const float *bq = buf + (32 + 8 * (int)(wtile >> 1)) * 256;  // this wave's query block
        const int qcol = 32 * (int)(wtile & 1u) + j;
#pragma unroll
        for (int c = 0; c < kWideChunks; ++c) {
          if (s * kWideChunks + c < nc) {
            const bf16x8 bh = __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4 *>(bq + ((c * 4 + 0 + h) * 64 + qcol) * 4));
            const bf16x8 bl = __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4 *>(bq + ((c * 4 + 2 + h) * 64 + qcol) * 4));
#pragma unroll
            for (int b = 0; b < kWideBlocks; ++b) {
              if ((uint32_t)b < nb) {
                const float *ab = buf + (b * 8 + c * 4) * 256;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                  const bf16x8 ah = __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4 *>(ab + ((0 + h) * 64 + 32 * t + j) * 4));
                  const bf16x8 al = __builtin_bit_cast(bf16x8, *reinterpret_cast<const float4 *>(ab + ((2 + h) * 64 + 32 * t + j) * 4));
                  acc[b][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[b][t], 0, 0, 0);
                  acc[b][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[b][t], 0, 0, 0);
                  acc[b][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[b][t], 0, 0, 0);
                }
              }
            }
          }
        }
      }
      // the next step's tiles have landed (nothing but the LDS-DMA is in flight), every wave is done with this buffer
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    if (wave_live) {
      float m[kWideBlocks][2];
#pragma unroll
      for (int b = 0; b < kWideBlocks; ++b) {
        m[b][0] = INFINITY; m[b][1] = INFINITY;
        if ((uint32_t)b < nb) {
          m[b][0] = tile_min(acc[b][0]);
          m[b][1] = tile_min(acc[b][1]);
          VI_TOP4(m[b][0]) VI_TOP4(m[b][1])
        }
      }
      if (qlive) {
        const uint32_t p0 = (blk0 - b0) >> 1;
        a.brec[(size_t)bi + (2u * kGroupQ) * p0] = make_float4(m[0][0], m[0][1], m[1][0], m[1][1]);
        if (nb > 2) a.brec[(size_t)bi + (2u * kGroupQ) * (p0 + 1u)] = make_float4(m[2][0], m[2][1], m[3][0], m[3][1]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the record stores, before the next C tile counts its DMA
    __syncthreads();                                    // s_norm and both buffers are free again
  }
  if (qlive) {
    const size_t gi = (size_t)a.qoff[qid] + a.rel[slot] + 2u * seg + (uint32_t)h;
    a.gval[gi] = make_float4(T0, T1, T2, T3);
    a.gmeta[gi] = (slot - qid * a.P) | (seg << 6) | ((uint32_t)h << 13);
  }
}


template <int NG>
vi_status launch_mfma_rank_t(const FilterArgs &a, uint32_t nitems, int rank_mode, uint32_t gq, hipStream_t st) {
  if (nitems == 0) return VI_OK;
  const bool table = a.qoff == nullptr;
  const dim3 grid(nitems);
  if (gq == 32) {  // one wave per work item (lists only): single buffer, many workgroups per CU
    const dim3 block(64);
    if (rank_mode == 2) hipLaunchKernelGGL((filter_kernel<NG, 1, false, 2, 32>), grid, block, 0, st, a);
    else if (rank_mode == 1) hipLaunchKernelGGL((filter_kernel<NG, 1, false, 1, 32>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((filter_kernel<NG, 1, false, 0, 32>), grid, block, 0, st, a);
  } else {
    const dim3 block(256);
    if (rank_mode == 2) {  // half-size tiles: two buffers fit where one full image did, the next tile loads during the MFMAs
      if (table) hipLaunchKernelGGL((filter_kernel<NG, 2, true, 2, 128>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((filter_kernel<NG, 2, false, 2, 128>), grid, block, 0, st, a);
    } else if (rank_mode == 1) {  // full images: one buffer, three workgroups per CU (two buffers cost the third: measured slower)
      if (table) hipLaunchKernelGGL((filter_kernel<NG, 1, true, 1, 128>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((filter_kernel<NG, 1, false, 1, 128>), grid, block, 0, st, a);
    } else {
      if (table) hipLaunchKernelGGL((filter_kernel<NG, 1, true, 0, 128>), grid, block, 0, st, a);
      else hipLaunchKernelGGL((filter_kernel<NG, 1, false, 0, 128>), grid, block, 0, st, a);
    }
  }
  VI_HIP(hipGetLastError());
  return VI_OK;
}

vi_status launch_mfma_rank(const FilterArgs &a, uint32_t dq, uint32_t nitems, int rank_mode, uint32_t gq, hipStream_t st) {
  switch (dq / 2) {  // dq is a multiple of 4
    case 2: return launch_mfma_rank_t<2>(a, nitems, rank_mode, gq, st);
    case 4: return launch_mfma_rank_t<4>(a, nitems, rank_mode, gq, st);
    case 6: return launch_mfma_rank_t<6>(a, nitems, rank_mode, gq, st);
    case 8: return launch_mfma_rank_t<8>(a, nitems, rank_mode, gq, st);
    case 10: return launch_mfma_rank_t<10>(a, nitems, rank_mode, gq, st);
    case 12: return launch_mfma_rank_t<12>(a, nitems, rank_mode, gq, st);
    case 14: return launch_mfma_rank_t<14>(a, nitems, rank_mode, gq, st);
    case 16: return launch_mfma_rank_t<16>(a, nitems, rank_mode, gq, st);
    default: return fail(VI_ERR_OTHER, "unsupported dimension for the MFMA engine");
  }
}

// Real-valued lists (not bf16-exact) ranked from their hi planes alone instead of hi + lo (bf16 x 3): a third (queries'
// hi + lo planes: mode 1) or a sixth (queries' hi plane only: mode 2) of the matrix work, paid for with a wider margin
// (select_body: 2 |q| max|v - hi(v)|, plus |query residual| max|v| in mode 2 — the residual norms are measured, not
// bounded by 2^-8 |v|: rounding to nearest leaves about a third of that), which the select turns into more sub-blocks
// re-evaluated exactly; no result depends on a rank value (file header).  Chosen per index from its sampled spread;
// VI_RANK_APPROX=0 / 1 / 2 forces bf16 x 3 / queries hi + lo / queries' hi plane only.
int rank_approx_mode(const DeviceIndex &ix, const EngineKnobs &kn) {
  if (kn.rank_approx >= 0) return kn.rank_approx;
  // a typical query is as long as a typical stored vector, and its image's residual about twice that of a stored vector's
  const double qlen = std::sqrt((double)(ix.centered ? ix.mean_norm2_c : ix.mean_norm2));
  const double vmax = std::sqrt((double)(ix.centered ? ix.xmax2_c : ix.xmax2)), rho = std::sqrt((double)ix.rho2_max);
  const double unit1 = 2.0 * qlen * rho, unit2 = unit1 + 2.0 * rho * vmax;
  if (kn.debug_approx)
    fprintf(stderr, "[vi] approx: centred %d qlen %.4g vmax %.4g rho %.4g spread %.4g unit1/spread %.4g unit2/spread %.4g\n", (int)ix.centered,
            qlen, vmax, rho, (double)ix.mean_spread, unit1 / (double)ix.mean_spread, unit2 / (double)ix.mean_spread);
  // The margin grows by `unit`; what it admits grows with unit / (distance of a vector to its neighbours), for which the
  // spread of the lists stands in.
  if (!(ix.mean_spread > 0.0f)) return 0;
  if (unit2 <= kApproxRatio * ix.mean_spread) return 2;
  if (unit1 <= kApproxRatio * ix.mean_spread) return 1;
  return 0;
}


// ------------------------------------------------------------------------------------------
// the rank plan: which kernel ranks a batch, decided before anything runs
// ------------------------------------------------------------------------------------------
enum class RankKernel { Wide, Block, Stream };  // rank_wide_kernel, filter_kernel (block-synchronous), rank_stream.hip
enum class RankMath { F32 = 0, Bf16x3 = 1, HiPlanes = 2 };  // (the values are the kernels' RANK template parameter)

struct RankPlan {
  RankKernel kernel;
  RankMath math;
  uint32_t gq;    // queries per rank work item: 32, 128 or 256
  int approx;     // real-valued lists ranked from their hi planes (rank_approx_mode): 1 queries hi + lo, 2 queries' hi plane only; else 0
  bool hi_lists;  // the lists are ranked from their hi planes alone: bf16-exact stored values, or approx != 0
  bool i8_lists;  // the lists offer this batch an int8 image (8-bit descriptors, streaming kernel, VI_RANK_I8 not 0)
  // known after the grouping's read-back only (complete_rank_plan)
  bool rank_i8;   // ... and the batch took it: int8 products (rank_stream_i8_kernel)
  bool qlo;       // the streaming bf16 kernel multiplies the queries' lo plane too
};

// gq_hint: what the previous batch of this shape (nq, P) measured to suit it (note_group_fill), 0: none yet;
// queries_hi_only: the previous batch's queries had no lo plane.  No HIP call, nothing written.
RankPlan plan_rank(const DeviceIndex &ix, const EngineKnobs &kn, uint64_t nq, uint32_t P, uint32_t gq_hint, bool queries_hi_only) {
  RankPlan p{};
  const uint32_t dq = ix.dq;
  const bool wide = ix.dim > kNarrowDim;
  // real-valued lists: hi planes only + a wider margin (rank_approx_mode) — the streaming kernel serves them too
  p.approx = (kn.rank_bf16 && !ix.lists_lo_zero && kn.hi_only && !wide) ? rank_approx_mode(ix, kn) : 0;
  p.hi_lists = (ix.lists_lo_zero && kn.hi_only) || p.approx != 0;
  // D <= 128, stored values bf16-exact (hi planes only): the streaming kernel (rank_stream.hip).  VI_RANK_STREAM=0:
  // block-synchronous kernel.
  // (bf16 x 3 keeps the block-synchronous kernel: two tiles of hi + lo planes do not fit in the streaming kernel's registers)
  // (measured at D = 32 / 64 / 96 / 128: its helper kernels and item skeleton pay off from 7 chunks of 16 dimensions on;
  // VI_RANK_STREAM=1 forces it for any D <= 128)
  const bool stream = !wide && kn.rank_bf16 && p.hi_lists && !kn.stream_off &&
                      (dq / 4 >= 7 || kn.stream_force || (p.approx != 0 && dq / 4 >= 5));
  p.kernel = wide ? RankKernel::Wide : stream ? RankKernel::Stream : RankKernel::Block;
  // (the wide kernel multiplies bf16 x 3 whatever the lists hold: mfma_path_applicable)
  p.math = !kn.rank_bf16 ? RankMath::F32 : (p.hi_lists && !wide) ? RankMath::HiPlanes : RankMath::Bf16x3;
  switch (p.kernel) {
    case RankKernel::Wide:  // the wide kernel's C tile holds 128 queries
      p.gq = 128u;
      break;
    case RankKernel::Stream:
      // A work item holds up to 128 queries and costs MFMAs for its live 32-query tiles only, so there is no group size
      // to choose (VI_STREAM_GQ=256: groups of 256 when the queries are bf16-exact too — measured equal).
      p.gq = kn.stream_gq256 && queries_hi_only ? 256u : 128u;
      break;
    case RankKernel::Block:
      // queries per rank work item: 128 when lists are shared by many queries of the batch, 32 when a list is probed by a
      // handful (large balanced indexes): a 128-query group would keep three of its four waves idle
      // The choice needs the batch's histogram, which only the grouping produces: the first batch of a shape (nq, P) goes by
      // the mean (queries per list), every later one by what the previous batch of that shape measured — the fill a
      // 128-query grouping has (pairs per tile slot; the grouping counts its tiles whichever size runs).  The mean alone is
      // wrong on skewed indexes: the reference's k-means on unclustered data leaves a few enormous lists that every query
      // probes (C5-shaped run: 4.9 queries per list on average, yet 128-query groups are three quarters full).
      // VI_FILTER_GQ overrides both.
      if (kn.gq) p.gq = kn.gq;
      else if (gq_hint) p.gq = gq_hint;
      else p.gq = (double)nq * P / (double)std::max<uint64_t>(1, ix.nlists) >= 24.0 ? 128u : 32u;
      break;
  }
  // 8-bit descriptors against a batch of integers in 0..254 (no kStatQueryNotI8 flag, known after the grouping): the streaming
  // kernel's int8 form (rank_stream_i8_kernel), exact ranks in the frame shifted by 127.  VI_RANK_I8=0: bf16.
  p.i8_lists = stream && ix.lists_i8.p && kn.rank_i8;
  return p;
}

// the two facts about the batch's queries that split_queries_kernel raises and the grouping reads back
void complete_rank_plan(RankPlan &p, const EngineKnobs &kn, const GroupingCounts &hstats) {
  p.rank_i8 = p.i8_lists && hstats[kStatQueryNotI8] == 0;
  p.qlo = (hstats[kStatQueryLo] != 0 || !kn.hi_only) && p.approx != 2;
}

// vi_search_stats::rank_mode (vi_amd.h) of a list scan:
//   0      exact-order VALU engine (search_kernels.hip: never from here)
//   1      f32 MFMA
//   2      bf16 x 3 MFMA
//   3      bf16 MFMA on hi planes only (bf16-exact stored values)
//   4      bf16 MFMA on the hi planes of real-valued lists (wider margin, more exact re-evaluations)
//   5 / 6  = 2 / 4 with the images taken about the mean of the stored vectors
uint64_t rank_mode_code(const DeviceIndex &ix, const RankPlan &p) {
  static constexpr uint64_t kCode[4][2] = {
      // images about the origin, about the mean
      {1, 1},  // f32 MFMA (multiplies the f32 blocks: no images)
      {2, 5},  // bf16 x 3
      {3, 3},  // hi planes of bf16-exact lists
      {4, 6},  // hi planes of real-valued lists
  };
  if (p.kernel == RankKernel::Wide) return kCode[1][0];  // (the wide kernel reports 2 wherever its images are centred)
  return kCode[p.math == RankMath::HiPlanes && p.approx ? 3 : (int)p.math][ix.centered ? 1 : 0];
}

}  // namespace

// ------------------------------------------------------------------------------------------
// coarse quantizer on the matrix cores
// ------------------------------------------------------------------------------------------
// The centroid table is one "list" probed by every query.
// Leaves probes / gorder and the per-list histogram (ws.cnt) behind, like stage_coarse.
static vi_status stage_coarse_mfma(SearchBatch &b, bool histogram_cleared = false) {
  const DeviceIndex &ix = b.ix;
  const EngineKnobs &kn = b.kn;
  SearchWorkspace &ws = b.ws();
  hipStream_t st = b.st();
  const uint32_t P = b.P, dim = ix.dim, dq = ix.dq;
  const uint64_t nq = b.nq, nlists = ix.nlists;
  VI_TRY(ws.cnt.reserve(2 * subbin_words(nlists)));
  if (!histogram_cleared) VI_HIP(hipMemsetAsync(ws.cnt.p, 0, subbin_words(nlists) * sizeof(uint32_t), st));
  VI_TRY(ws.probes.reserve(nq * P));
  VI_TRY(ws.gorder.reserve(nq * P));
  // one list, every query probes it: groups of 128 queries x segments of segb blocks
  const uint32_t segb0 = 4;
  uint32_t segb;
  const uint32_t nseg = list_segments((uint32_t)nlists, segb0, &segb);
  const uint32_t recs = 2u * nseg;
  const uint32_t ngroups = (uint32_t)((nq + kGroupQ - 1) / kGroupQ);
  const uint32_t h_seg[2] = {0u, (uint32_t)nq}, h_item[2] = {0u, ngroups * nseg};
  VI_TRY(ws.c_seg.reserve(2));
  VI_TRY(ws.c_item.reserve(2));
  VI_TRY(ws.c_pairs.reserve(nq));
  VI_TRY(ws.gval.reserve(nq * recs * 4));
  VI_TRY(ws.gpos.reserve(nq * recs));
  const bool direct = ix.centroids.nblocks <= kDirectBlocks && kn.coarse_direct;
  if (direct && !ix.cent_rows.p) return fail(VI_ERR_OTHER, "coarse table without its row-major copy");  // (prepare_rank_images: D <= 128)
  VI_TRY(ws.brec.reserve((uint64_t)ngroups * (direct ? 2 * ix.centroids.nblocks : (uint64_t)nseg * seg_records(segb)) * 256 * 4));
  VI_TRY(ws.stats.reserve(kStatWords));
  if (ws.c_nq != nq) {  // the table's one-list grouping depends on the batch size only
    VI_HIP(hipMemcpyAsync(ws.c_seg.p, h_seg, 8, hipMemcpyHostToDevice, st));
    VI_HIP(hipMemcpyAsync(ws.c_item.p, h_item, 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(iota_kernel, dim3((uint32_t)((nq + 255) / 256)), dim3(256), 0, st, ws.c_pairs.p, (uint32_t)nq);
    VI_HIP(hipGetLastError());
    VI_HIP(hipStreamSynchronize(st));  // h_seg / h_item live on this stack frame
    ws.c_nq = nq;
  }
  FilterArgs a{};
  a.blocks = kn.rank_bf16 ? (const float4 *)ix.cent_bf16.p : (const float4 *)ix.centroids.blocks.p;
  a.xnorm = kn.rank_bf16 ? ix.cent_xnorm_img.p : ix.cent_xnorm.p; a.dq = dq; a.dim = dim; a.Q = b.Qd;
  a.first_block = ix.c_first.p; a.list_len = ix.c_len.p; a.item_start = ws.c_item.p; a.seg_start = ws.c_seg.p;
  a.pairs = ws.c_pairs.p; a.nlists = 1; a.P = 1; a.segb0 = segb0;
  a.qoff = nullptr; a.rel = nullptr; a.rec_stride = recs;
  a.tile_start = ix.c_first.p;  // one list: its tiles start at 0 (c_first holds a single 0)
  a.gval = (float4 *)ws.gval.p; a.gmeta = ws.gpos.p; a.brec = (float4 *)ws.brec.p;
  a.direct = direct ? 1u : 0u;
  a.qimg = kn.rank_bf16 ? (const uint4 *)ws.qimg.p : nullptr;
  VI_TRY(launch_mfma_rank(a, dq, ngroups * nseg, kn.rank_bf16 ? (ix.cent_lo_zero && kn.hi_only ? 2 : 1) : 0, kGroupQ, st));
  return launch_coarse_select(b, segb, recs, direct);
}

bool mfma_path_applicable(const DeviceIndex &ix, const EngineKnobs &kn, uint64_t k, uint32_t P) {
  if (!kn.mfma) return false;
  if (ix.order != VI_ORDER_SCALAR || ix.dim > kMaxFilterDim || (ix.dim & 3) || ix.dim < 4) return false;
  if (ix.dim > kNarrowDim && !kn.rank_bf16) return false;  // the wide kernel ranks with bf16 x 3 only
  if (k > 2 * kMaxSelect || P > kMaxSelect || P < 1) return false;  // k <= 128 (WaveTop128), n_probe <= 64
  if (ix.lists.nblocks * 64ull >= (1ull << kPosBits)) return false;  // record position < 2^26, block < 2^20
  if (!(ix.xmax2 < 1.0e30f) || !(ix.cent_xmax2 < 1.0e30f)) return false;  // norms must stay far below kBig
  // measured on the bench index from nq = 1 (0.19 ms vs 0.83 ms) to nq = 10 000 (0.93 ms vs 6 ms): the MFMA engine
  // also wins on tiny batches, because it cuts long lists into segments that run in parallel
  return true;
}

// the coarse step on the matrix cores (stage_coarse_mfma) rather than the VALU one (stage_coarse): batches of >= 256
// queries against tables of >= 1024 lists, D <= 128 (filter_kernel keeps a query in registers)
bool coarse_on_matrix_cores(const DeviceIndex &ix, const EngineKnobs &kn, uint64_t nq, uint32_t P) {
  return mfma_path_applicable(ix, kn, 1, P) && kn.coarse_mfma && nq >= 256 && ix.nlists >= 1024 && ix.dim <= kNarrowDim;
}

// the batch's queries as MFMA operands: -2 q split into bf16 hi / lo once (a query sits in n_probe work items)
static vi_status build_query_image(SearchBatch &b, uint32_t *zero = nullptr, uint64_t zero_words = 0) {
  if (!b.kn.rank_bf16) return VI_OK;
  const DeviceIndex &ix = b.ix;
  SearchWorkspace &ws = b.ws();
  const uint64_t nq = b.nq;
  hipStream_t st = b.st();
  const uint32_t nc = ix.dq / 4;
  VI_TRY(ws.qimg.reserve((uint64_t)nq * nc * 4 * 4));  // uint32 words: 4 pieces of 16 B per (query, chunk)
  const bool i8 = ix.lists_i8.p != nullptr;  // the lists have an int8 image: the batch's too (rank_stream_i8_kernel)
  if (i8) VI_TRY(ws.qimg8.reserve(std::max<uint64_t>(1, (uint64_t)nq * ((ix.dim + 31) / 32) * 8)));  // uint32 words: 32 B per (query, chunk of 32)
  VI_TRY(ws.stats.reserve(kStatWords));
  if (!ws.stats_zeroed) {  // kStatQueryLo, kStatQueryNotI8 start at zero (both are read back with the
                           // grouping's counts) — reset by item_cols_kernel after their use
    VI_HIP(hipMemsetAsync(ws.stats.p, 0, kStatWords * sizeof(uint64_t), st));
    ws.stats_zeroed = true;
  }
  const uint64_t nt = (uint64_t)nq * nc * 2;
  hipLaunchKernelGGL(split_queries_kernel, dim3((uint32_t)((nt + 255) / 256)), dim3(256), 0, st, b.Qd, (uint32_t)nq, ix.dim, nc,
                     (uint4 *)ws.qimg.p, (unsigned long long *)(ws.stats.p + kStatQueryLo), zero, (uint32_t)zero_words,
                     ix.centered ? (const float *)ix.centre.p : nullptr, i8 ? (uint2 *)ws.qimg8.p : nullptr,
                     (unsigned long long *)(ws.stats.p + kStatQueryNotI8), ws.stats.p);
  b.group_counts_cleared = true;
  VI_HIP(hipGetLastError());
  return VI_OK;
}

// coarse step alone on the matrix cores (probe export for other ranks): fills ws.probes / ws.gorder
vi_status coarse_only_mfma(SearchBatch &b) {
  VI_TRY(build_query_image(b));
  VI_TRY(b.ws().pair_rel.reserve(b.nq * b.P));
  VI_TRY(b.ws().qtot.reserve(b.nq));
  return stage_coarse_mfma(b);
}

// ------------------------------------------------------------------------------------------
// the steps of the two pipelines, in the order they run on the search stream, each on the SearchBatch.  (b.flt swaps the norms
// the LIST phase ranks with for its masked copies — excluded slots rank as pad slots do; the coarse phase keeps the table's.)
// ------------------------------------------------------------------------------------------
namespace {

// (the phase clock of the rank kernel starts right in front of it: the work-item helper kernels count as grouping)
vi_status start_rank_clock(SearchBatch &b) {
  if (b.timing && !b.rank_clock_started) VI_HIP(hipEventRecord(b.ctx.ev[2], b.st()));
  b.rank_clock_started = true;
  return VI_OK;
}

// ---- 1. coarse quantizer: the queries' image, then probes, shard visiting order, per-list histogram, record offsets ----
vi_status coarse_phase(SearchBatch &b) {
  SearchWorkspace &ws = b.ws();
  VI_TRY(ws.pair_rel.reserve(b.nq * b.P));
  VI_TRY(ws.qtot.reserve(b.nq));
  const bool coarse_mfma = !b.probes_in && coarse_on_matrix_cores(b.ix, b.kn, b.nq, b.P);
  const bool histogram_cleared = coarse_mfma && b.kn.rank_bf16;
  if (histogram_cleared) {  // (the coarse step's per-list histogram is cleared by the kernel that splits the queries)
    VI_TRY(ws.cnt.reserve(2 * subbin_words(b.ix.nlists)));
    VI_TRY(build_query_image(b, ws.cnt.p, subbin_words(b.ix.nlists)));
  } else {
    VI_TRY(build_query_image(b));
  }
  if (coarse_mfma) {
    VI_TRY(stage_coarse_mfma(b, histogram_cleared));
  } else {
    if (b.probes_in) VI_TRY(adopt_probes(b, true));
    else VI_TRY(stage_coarse(b));
    hipLaunchKernelGGL(pair_groups_kernel, dim3((uint32_t)((b.nq + 255) / 256)), dim3(256), 0, b.st(), ws.probes.p,
                       b.ix.list_len.p, (uint32_t)b.nq, b.P, b.kn.segb0, ws.pair_rel.p, ws.qtot.p);
  }
  // (the grouping scans the record offsets too: workgroups of list_totals_kernel, or the second of group_prepare_kernel)
  VI_HIP(hipGetLastError());
  return VI_OK;
}

uint32_t gq_hint_for(const SearchWorkspace &ws, uint64_t nq, uint32_t P) {
  for (const auto &h : ws.gq_hint)
    if (h.nq == nq && h.P == P) return h.gq;
  return 0u;
}

// the group size the next batch of this shape should take, from the fill a grouping by 128 queries has in this one
void note_group_fill(SearchWorkspace &ws, uint64_t nq, uint32_t P, const GroupingCounts &hstats) {
  const double fill128 = hstats[kStatTiles128] ? (double)hstats[kStatScannedVectors] / ((double)hstats[kStatTiles128] * 128.0 * 64.0) : 0.0;
  const uint32_t next = fill128 >= 0.3 ? 128u : 32u;
  for (auto &h : ws.gq_hint)
    if (h.nq == nq && h.P == P) { h.gq = next; return; }
  if (ws.gq_hint.size() >= 64) ws.gq_hint.clear();
  ws.gq_hint.push_back({nq, P, next});
}

// ---- 2. group all (query, probe) pairs by list; the counts come back (the pipeline's one synchronisation) and with them
//      the two flags that complete the plan; the record buffers are sized by them ----
vi_status group_pairs(SearchBatch &b, RankPlan &plan, GroupingCounts &hstats) {
  SearchWorkspace &ws = b.ws();
  vi_search_stats &stt = b.ctx.stats;
  VI_TRY(ws.qoff.reserve(b.nq + 1));
  // the streaming kernel's work items come out of the scatter itself when the coarse select left every pair's rank
  b.items_pushed = b.kn.item_push && plan.kernel == RankKernel::Stream && b.pair_rank_valid;
  GroupingRequest rq;
  rq.probes = ws.probes.p; rq.nq = b.nq; rq.P = b.P; rq.qg = plan.gq; rq.segb0 = b.kn.segb0; rq.histogram_done = true;
  rq.qtot = ws.qtot.p; rq.qoff = ws.qoff.p; rq.pair_rank = b.pair_rank_valid ? ws.pair_rank.p : nullptr;
  rq.push_run = b.items_pushed ? b.kn.item_run : 0u; rq.counts_cleared = b.kn.scan_in_totals && b.group_counts_cleared;
  rq.tile_start = rq.pair_pos = true;  // (the selects read both)
  VI_TRY(group_probes(b.ix, b.ctx, rq, hstats));
  note_group_fill(ws, b.nq, b.P, hstats);
  ws.queries_hi_only = hstats[kStatQueryLo] == 0;
  complete_rank_plan(plan, b.kn, hstats);
  stt.scanned_vectors = hstats[kStatScannedVectors];
  stt.scan_items = hstats[kStatItems];
  stt.filter_tile_blocks = hstats[kStatTileBlocks];
  const uint64_t nrec = hstats[kStatGroupRecords], nbrec = hstats[kStatRecordTiles] * 2 * plan.gq;  // pair records: 2 x gq per (query group, segment, 2 blocks)
  if (nrec >= (1ull << 31) || nbrec >= (1ull << 32)) return fail(VI_ERR_INVALID_INPUT, "batch too large: split nq");
  VI_TRY(ws.gval.reserve(std::max<uint64_t>(1, nrec) * 4));
  VI_TRY(ws.brec.reserve(std::max<uint64_t>(1, nbrec) * 4));
  if (!b.items_pushed) return ws.gpos.reserve(std::max<uint64_t>(1, nrec));
  // The scatter compared the same counts with the buffers it was given: where they did not fit it wrote nothing — grow
  // them, by a quarter more than asked so that a slightly larger batch fits, and push again.  (A batch shape's first
  // search; batches of a steady size never come here.)
  const uint64_t ncol = hstats[kStatItems] * plan.gq, ndesc = hstats[kStatItems] * 4;
  if (ncol <= ws.item_qcol.n && ncol <= ws.item_grec.n && ndesc <= ws.item_sdesc.n && nrec <= ws.gpos.n) return VI_OK;
  auto grow = [](DevBuf<uint32_t> &buf, uint64_t need) { return need <= buf.n ? VI_OK : buf.reserve(need + need / 4); };
  VI_TRY(grow(ws.item_qcol, ncol));
  VI_TRY(grow(ws.item_grec, ncol));
  VI_TRY(grow(ws.item_sdesc, ndesc));
  VI_TRY(grow(ws.gpos, nrec));
  return repush_items(b.ix, ws, rq, b.st());
}

// ---- 3. rank on the matrix cores: one of the three below ----
// D > 128: the GEMM-shaped kernel
vi_status rank_wide(SearchBatch &b, uint32_t nitems) {
  SearchWorkspace &ws = b.ws();
  const DeviceIndex &ix = b.ix;
  VI_TRY(launch_item_list(ix, ws, nitems, b.st()));
  if (nitems) {
    WideArgs a{(const uint4 *)ix.lists_bf16.p, b.flt ? b.flt->xnorm_img.p : ix.xnorm_img.p, (const uint4 *)ws.qimg.p, ix.dq / 4,
               ix.list_first_block.p, ix.list_len.p, ws.item_start.p, ws.seg_start.p, ws.pairs.p, ws.item_list.p, b.P, b.kn.segb0,
               ws.qoff.p, ws.pair_rel.p, ws.tile_start.p, (float4 *)ws.gval.p, ws.gpos.p, (float4 *)ws.brec.p};
    // (set on the device that launches, every time: a process may hold indexes on several GPUs)
    if (hipFuncSetAttribute((const void *)rank_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                            kWideLdsFloats * (int)sizeof(float)) != hipSuccess)
      return fail(VI_ERR_DEVICE, "cannot reserve %d bytes of LDS for the wide rank kernel", kWideLdsFloats * 4);
    VI_TRY(start_rank_clock(b));
    hipLaunchKernelGGL(rank_wide_kernel, dim3(nitems), dim3(256), kWideLdsFloats * sizeof(float), b.st(), a);
  }
  VI_HIP(hipGetLastError());
  return VI_OK;
}

// (VI_STREAM_PROF) the streaming kernel's phase clocks, read back behind it: this step synchronises
vi_status print_stream_profile(SearchBatch &b) {
  SearchWorkspace &ws = b.ws();
  uint64_t h[24];
  VI_HIP(hipMemcpyAsync(h, ws.prof.p, sizeof(h), hipMemcpyDeviceToHost, b.st()));
  VI_HIP(hipStreamSynchronize(b.st()));
  fprintf(stderr, "rank_stream wave-0 ticks (100 MHz) summed over workgroups: multiply %llu (of which waiting for tiles %llu) "
          "end-of-item wait %llu gather %llu merge %llu | items %llu steps %llu | loop total %llu\n",
          (unsigned long long)h[0], (unsigned long long)h[6], (unsigned long long)h[1], (unsigned long long)h[2],
          (unsigned long long)h[3], (unsigned long long)h[4], (unsigned long long)h[5], (unsigned long long)h[7]);
  if (const char *dump = b.kn.stream_prof_dump) {
    std::vector<uint64_t> w(4 * 1024);
    VI_HIP(hipMemcpy(w.data(), ws.prof.p + 32, w.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (FILE *f = fopen(dump, "w")) {
      uint64_t base = ~0ull;
      for (int i = 0; i < 1024; ++i) if (w[4 * i + 1]) base = std::min(base, w[4 * i]);
      for (int i = 0; i < 1024; ++i)  // workgroup, start, end (10 ns ticks after the first start), items
        if (w[4 * i + 1]) fprintf(f, "%d %llu %llu %llu\n", i, (unsigned long long)(w[4 * i] - base), (unsigned long long)(w[4 * i + 1] - base),
                                  (unsigned long long)w[4 * i + 2]);
      fclose(f);
    }
  }
  fprintf(stderr, "   loops entered over %llu ticks, last exit %llu ticks after the first entry\n", (unsigned long long)(h[17] - h[16]),
          (unsigned long long)(h[18] - h[16]));
  fprintf(stderr, "   longest workgroup loop %llu ticks, workgroups with items %llu, most items in one %llu\n", (unsigned long long)h[13],
          (unsigned long long)h[14], (unsigned long long)h[15]);
  fprintf(stderr, "   after B1: T+idx %llu, DMA issue %llu, vmcnt(0) %llu, B2 %llu | after B2: merge+stores %llu, idx read %llu, load_item %llu\n",
          (unsigned long long)h[8], (unsigned long long)h[9], (unsigned long long)h[10], (unsigned long long)h[2],
          (unsigned long long)h[11], (unsigned long long)h[12], (unsigned long long)h[3]);
  return VI_OK;
}

// D <= 128, hi planes only: queries in LDS, vectors through registers, no barrier in the block loop, persistent workgroups
// (rank_stream.hip), with int8 products when the plan says so
vi_status rank_stream(SearchBatch &b, const RankPlan &plan, uint32_t nitems) {
  SearchWorkspace &ws = b.ws();
  const DeviceIndex &ix = b.ix;
  const uint32_t gq = plan.gq;
  if (!b.items_pushed) {  // (pushed: the columns stand, in buffers sized by group_pairs)
    VI_TRY(launch_item_desc(ix, ws, b.kn, gq, nitems, b.st()));
    VI_TRY(launch_item_cols(ws, b.P, gq, nitems, b.st()));
  }
  if (plan.rank_i8) {
    RankStreamI8Args a{(const uint4 *)ix.lists_i8.p, b.flt ? b.flt->i8_norm_img.p : ix.i8_norm_img.p, (const uint4 *)ws.qimg8.p,
                       (const uint4 *)ws.item_sdesc.p, nitems, ws.item_qcol.p, ws.item_grec.p,
                       (uint32_t *)(ws.stats.p + kStatRankWork), (float4 *)ws.gval.p, (float4 *)ws.brec.p};
    VI_TRY(start_rank_clock(b));
    return launch_rank_stream_i8(a, (ix.dim + 31) / 32, nitems, gq, b.st());
  }
  RankStreamArgs a{(const uint4 *)ix.lists_bf16.p, b.flt ? b.flt->xnorm_img.p : ix.xnorm_img.p, (const uint4 *)ws.qimg.p,
                   (const uint4 *)ws.item_sdesc.p, nitems, ws.item_qcol.p, ws.item_grec.p, (uint32_t *)(ws.stats.p + kStatRankWork),
                   (float4 *)ws.gval.p, (float4 *)ws.brec.p, nullptr, b.kn.rank_xmode};
  if (b.kn.stream_prof) {
    VI_TRY(ws.prof.reserve(32 + 4 * 1024));
    VI_HIP(hipMemsetAsync(ws.prof.p, 0, (32 + 4 * 1024) * sizeof(uint64_t), b.st()));
    VI_HIP(hipMemsetAsync(ws.prof.p + 16, 0xFF, sizeof(uint64_t), b.st()));
    a.prof = (unsigned long long *)ws.prof.p;
  }
  VI_TRY(start_rank_clock(b));
  // (this kernel ranks hi planes only: plan.math is HiPlanes here)
  VI_TRY(launch_rank_stream(a, ix.dq / 4, nitems, (int)plan.math, plan.qlo, gq, b.st()));
  if (b.kn.stream_prof) VI_TRY(print_stream_profile(b));
  return VI_OK;
}

// D <= 128, everything else: the block-synchronous kernel, in the plan's arithmetic
vi_status rank_block(SearchBatch &b, const RankPlan &plan, uint32_t nitems) {
  SearchWorkspace &ws = b.ws();
  const DeviceIndex &ix = b.ix;
  const bool bf16 = b.kn.rank_bf16;
  VI_TRY(launch_item_desc(ix, ws, b.kn, plan.gq, nitems, b.st()));
  FilterArgs a{};
  a.blocks = bf16 ? (const float4 *)ix.lists_bf16.p : (const float4 *)ix.lists.blocks.p;
  a.xnorm = bf16 ? (b.flt ? b.flt->xnorm_img.p : ix.xnorm_img.p) : (b.flt ? b.flt->xnorm.p : ix.xnorm.p);
  a.dq = ix.dq; a.dim = ix.dim; a.Q = b.Qd;
  a.first_block = ix.list_first_block.p; a.list_len = ix.list_len.p; a.item_start = ws.item_start.p;
  a.seg_start = ws.seg_start.p; a.pairs = ws.pairs.p; a.nlists = (uint32_t)ix.nlists; a.P = b.P; a.segb0 = b.kn.segb0;
  a.qoff = ws.qoff.p; a.rel = ws.pair_rel.p; a.rec_stride = 0;
  a.tile_start = ws.tile_start.p;
  a.items = (const uint4 *)ws.items.p;
  a.gval = (float4 *)ws.gval.p; a.gmeta = ws.gpos.p; a.brec = (float4 *)ws.brec.p;
  a.xmode = b.kn.rank_xmode;
  a.qimg = bf16 ? (const uint4 *)ws.qimg.p : nullptr;
  VI_TRY(start_rank_clock(b));
  return launch_mfma_rank(a, ix.dq, nitems, (int)plan.math, plan.gq, b.st());
}

// (VI_FILTER_STATS with timing level 1) the selects' counters and stage clocks, read back behind the select: synchronises
vi_status report_select_stats(SearchBatch &b) {
  const EngineKnobs &kn = b.kn;
  vi_search_stats &stt = b.ctx.stats;
  uint64_t dbg[kStatSelectEnd], tks[kStatClockCount];
  VI_HIP(hipMemcpyAsync(dbg, b.ws().stats.p, sizeof(dbg), hipMemcpyDeviceToHost, b.st()));
  VI_HIP(hipMemcpyAsync(tks, b.ws().stats.p + kStatClocks, sizeof(tks), hipMemcpyDeviceToHost, b.st()));
  VI_HIP(hipStreamSynchronize(b.st()));
  if (kn.stats_coarse)
    fprintf(stderr, "coarse select ticks (every 64th query): query row %llu, records + bound %llu, flags (+ rounds a full list forces) %llu, exact rounds %llu, tail %llu; rows %llu "
            "of which in whole sub-blocks %llu\n", (unsigned long long)tks[0], (unsigned long long)tks[1], (unsigned long long)tks[2],
            (unsigned long long)tks[3], (unsigned long long)tks[4], (unsigned long long)dbg[kStatSelExact], 8ull * (unsigned long long)dbg[kStatSelScanned]);
  if (kn.stats_print)
    fprintf(stderr, "select ticks: records -> LDS %llu, threshold %llu, refinement %llu, scan of pair records (+ exact rounds it triggers) %llu, "
            "last exact rounds %llu\n", (unsigned long long)tks[0], (unsigned long long)tks[1], (unsigned long long)tks[2],
            (unsigned long long)tks[3], (unsigned long long)tks[4]);
  stt.filter_rechecked = dbg[kStatSelExact]; stt.filter_accepted = dbg[kStatSelScanned];
  if (kn.stats_print)
    fprintf(stderr, "select stats: exact %llu groups_scanned %llu queries_with_full_group %llu full_groups %llu sub_blocks %llu\n",
            (unsigned long long)dbg[kStatSelExact], (unsigned long long)dbg[kStatSelScanned], (unsigned long long)dbg[kStatSelQueriesFull],
            (unsigned long long)dbg[kStatSelFullGroups], (unsigned long long)dbg[kStatSelSubBlocks]);
  return VI_OK;
}

}  // namespace

// ---- 1 to 3 on the search stream: what both list selects (top-k, radius) start from.  Leaves the frame the lists were
//      ranked by; b.timing 1: an event at every phase boundary; 2: around the rank kernel only (every record is a
//      barrier packet the next kernel's dispatch waits behind: five of them cost 0.01 ms of a 0.5 ms step) ----
static vi_status rank_lists(SearchBatch &b, SelectFrame &ranked) {
  const DeviceIndex &ix = b.ix;
  const EngineKnobs &kn = b.kn;
  hipStream_t st = b.st();
  SearchWorkspace &ws = b.ws();
  vi_search_stats &stt = b.ctx.stats;
  const bool timing = b.timing == 1;
  VI_TRY(ws.stats.reserve(kStatWords));
  if (kn.stats) {  // the selects' counters and stage clocks
    VI_HIP(hipMemsetAsync(ws.stats.p + kStatSelExact, 0, (kStatSelectEnd - kStatSelExact) * sizeof(uint64_t), st));
    VI_HIP(hipMemsetAsync(ws.stats.p + kStatClocks, 0, kStatClockCount * sizeof(uint64_t), st));
  }
  if (timing) VI_HIP(hipEventRecord(b.ctx.ev[0], st));
  VI_TRY(coarse_phase(b));
  if (timing) VI_HIP(hipEventRecord(b.ctx.ev[1], st));

  RankPlan plan = plan_rank(ix, kn, b.nq, b.P, gq_hint_for(ws, b.nq, b.P), ws.queries_hi_only);
  GroupingCounts hstats;
  VI_TRY(group_pairs(b, plan, hstats));
  stt.rank_mode = rank_mode_code(ix, plan);
  stt.group_queries = plan.gq;
  stt.rank_int8 = plan.rank_i8 ? 1u : 0u;

  const uint32_t nitems = (uint32_t)hstats[kStatItems];
  switch (plan.kernel) {
    case RankKernel::Wide: VI_TRY(rank_wide(b, nitems)); break;
    case RankKernel::Stream: VI_TRY(rank_stream(b, plan, nitems)); break;
    case RankKernel::Block: VI_TRY(rank_block(b, plan, nitems)); break;
  }
  VI_TRY(start_rank_clock(b));  // (nothing to rank)
  if (b.timing) VI_HIP(hipEventRecord(b.ctx.ev[3], st));
  ranked = SelectFrame{plan.gq, plan.kernel == RankKernel::Stream, plan.approx, plan.rank_i8};
  return VI_OK;
}


vi_status search_mfma_pipeline(SearchBatch &b, uint64_t k, const SelectOutputs &out) {
  SelectFrame ranked;
  VI_TRY(rank_lists(b, ranked));
  VI_TRY(launch_list_select(b, k, ranked, out));
  if (b.timing == 1) VI_HIP(hipEventRecord(b.ctx.ev[4], b.st()));
  return b.timing == 1 && b.kn.stats ? report_select_stats(b) : VI_OK;
}

// the radius search: the same records, read by the radius select (range_select.hip) instead of the top-k select
vi_status range_mfma_pipeline(SearchBatch &b, float radius2, RangeResult *res) {
  SelectFrame ranked;
  VI_TRY(rank_lists(b, ranked));
  VI_TRY(launch_range_select(b, radius2, ranked, res));
  if (b.timing == 1) VI_HIP(hipEventRecord(b.ctx.ev[4], b.st()));
  return b.timing == 1 && b.kn.stats ? report_select_stats(b) : VI_OK;
}

}  // namespace vi
