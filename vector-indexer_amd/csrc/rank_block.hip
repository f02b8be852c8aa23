// rank_block.hip — the block-synchronous rank kernels of the MFMA engine: filter_kernel (D <= 128: the lists in f32 MFMA or
// bf16 x 3 arithmetic, and the coarse table) and rank_wide_kernel (128 < D <= 1536), behind rank_block.hpp.
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
// ("filter" in filter_kernel and the VI_FILTER variables is the engine's first name.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.hpp"
#include "mfma_bf16.hpp"
#include "rank_block.hpp"
#include "scan.hpp"
#include "select.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;

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
    filter_kernel(RankBlockArgs a) {  // (second bound = waves per SIMD the register allocation must allow)
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

__global__ void __launch_bounds__(256, 1) rank_wide_kernel(RankWideArgs a) {
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
vi_status launch_mfma_rank_t(const RankBlockArgs &a, uint32_t nitems, int rank_mode, uint32_t gq, hipStream_t st) {
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

}  // namespace

vi_status launch_rank_block(const RankBlockArgs &a, uint32_t dq, uint32_t nitems, int rank_mode, uint32_t gq, hipStream_t st) {
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

vi_status launch_rank_wide(const RankWideArgs &a, uint32_t nitems, hipStream_t st) {
  if (nitems == 0) return VI_OK;
  // (set on the device that launches, every time: a process may hold indexes on several GPUs)
  if (hipFuncSetAttribute((const void *)rank_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          kWideLdsFloats * (int)sizeof(float)) != hipSuccess)
    return fail(VI_ERR_DEVICE, "cannot reserve %d bytes of LDS for the wide rank kernel", kWideLdsFloats * 4);
  hipLaunchKernelGGL(rank_wide_kernel, dim3(nitems), dim3(256), kWideLdsFloats * sizeof(float), st, a);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

}  // namespace vi
