// flat_knn.hip — the exact k-NN graph of the stored records of a built index: for every record the k smallest keys
// (distance bits, ordinal) over all participants, from ONE triangular sweep on the matrix cores in which every unordered
// pair is visited once (the contract is vi_indexer_knn_graph_exact in include/vi_amd.h).
//
// The exact radius join (flat_join.hip, §4t) visits a pair (u, v), slot of v above slot of u, in u's frame only and
// compares v's rank value with the one threshold of the call's radius.  Here every record has a radius of its own — an
// upper bound B of its k-th neighbour's distance — and the pair's single visit has to keep it when EITHER record wants it.
//
//   1. seed     pass 1 over all chunks of the walk over stored records (StoredRowsWalk): the unchanged top-k search at
//               seed_probe, k (+ 1) wide; knn_bound_kernel drops the row's own slot and writes bound[slot] = the k-th
//               distance left, +inf where the seed found fewer than k (an UNBOUNDED row), 4 bytes per slot.  Pad slots
//               and slots a filter does not admit hold -inf.  knn_block_max_kernel: per block its largest finite bound.
//               The seed's hits are not copied anywhere: they lie under the bound and the sweep meets them.
//   2. prepare  per chunk of pass 2, one wave per row: the row's frame (qn, E), thr_u = radius_rank_threshold(B_u) in it
//               (-inf for a row that is not admitted) and the row's bf16 hi / lo image.
//   3. sweep    flat_knn_sweep_kernel: §4t's blocking — row tiles of 128 x segments of S blocks from the block of the
//               tile's first row on, a wave owns 32 rows, B fragments in registers at D <= 128, block images by LDS-DMA
//               into two buffers, bf16 x 3 on v_mfma_f32_32x32x16_bf16 — with the block's 64 bounds staged into LDS
//               beside its 64 norms and a TWO-SIDED compare per accumulator element:
//                   keep  <=>  !(x > thr_u)  ||  !(x - B_v > delta),   delta = (thr_u(Bmax_b) - Bmax_b) + slack
//               with delta formed once per (lane, block) from the block's largest finite bound Bmax_b.  d <= B_v implies
//               x <= thr_u(B_v) (§4s, in u's frame whatever the radius), thr_u(r) - r does not decrease in r, and the
//               slack covers the f32 roundings of both sides (§4u): the compare may let through too many pairs, never
//               too few.  B_v = +inf gives x - B_v = -inf and passes, B_v = -inf gives +inf and does not; NaN passes.
//               The drain evaluates a surviving pair once in the reference's chain and emits (row u: key(d, ord v)) if
//               d <= B_u and (row v: key(d, ord u)) if d <= B_v into §4s's pool, one atomicAdd per round of 64.
//   4. finish   lims from the per-row counts, place / sort of flat_rows.hpp, flat_knn_take_kernel cuts every row at k.
// An unbounded row evaluates every participant; a pool that proves too small grows to the count and pass 2 runs once
// more.  No result depends on a rank value, on seed_probe, on the pool or on the order entries arrive in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "device_index.hpp"
#include "flat_common.hpp"
#include "flat_knn.hpp"
#include "flat_rows.hpp"
#include "flat_search.hpp"
#include "mfma_bf16.hpp"
#include "record_fetch.hpp"
#include "search_internal.hpp"
#include "select_device.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

constexpr uint32_t kTileRows = 128;    // rows per workgroup: four waves of one 32-column B tile each
constexpr uint32_t kMaxChunks = 8;     // D <= 128: chunks of 16 dimensions whose B fragments a wave keeps in registers
constexpr uint32_t kStreamChunks = 2;  // D > 128: chunks per K step (both operands stream through LDS)
constexpr uint32_t kQueueLen = 1024;   // survivors of one wave and accumulator tile: 32 rows x 32 vectors, never more
constexpr uint32_t kSegMin = 4, kSegMax = 32;  // blocks per segment
constexpr uint32_t kMaxGridY = 65535;
constexpr float kUnbounded = 1.0e37f;  // from here on a bound says nothing (radius_rank_threshold): it is kept as +inf
// delta's slack, relative to the magnitudes delta is formed from: some ten roundings of 2^-24 on either side (§4u)
constexpr float kDeltaSlack = 3.8146973e-6f;  // 2^-18

enum { kCursor = 0, kSurvivors = 1, kUnboundedRows = 2, kKnnCounters = 3 };

// ---- step 1: the bounds ----
__global__ void knn_clear_bounds_kernel(float *bound, uint32_t nslots, unsigned long long *counters) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < kKnnCounters) counters[i] = 0ull;
  if (i < nslots) bound[i] = -INFINITY;
}

struct KnnBoundArgs {
  const float *D;             // [m][kk] the seed's rows
  const uint64_t *slots;
  const uint32_t *self_slot;  // [m]
  const uint64_t *allow;      // the filter's allow bits, or null
  uint32_t m, k, kk;          // kk = k + 1: the row's own slot is dropped
  float *bound;               // [nslots]
  unsigned long long *counters;
};

// One wave per row: the k-th distance of the seed's ascending row once the row's own slot is gone — entry k - 1, or
// entry k where the own slot is one of the first k.  Any k participants other than the row bound its k-th key from above.
__global__ void __launch_bounds__(256) knn_bound_kernel(KnnBoundArgs a) {
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (q >= a.m) return;  // (wave-uniform)
  const uint32_t s = a.self_slot[q];
  if (a.allow && !((a.allow[s >> 6] >> (s & 63u)) & 1ull)) return;  // not admitted: -inf stays
  const size_t in0 = (size_t)q * a.kk;
  bool own = false;
  if (a.kk > a.k)
    for (uint32_t j0 = 0; j0 < a.k && !own; j0 += 64u) own = __ballot(j0 + lane < a.k && a.slots[in0 + j0 + lane] == (uint64_t)s) != 0ull;
  if (lane) return;
  float d = a.D[in0 + a.k - 1u + (own ? 1u : 0u)];
  if (!(d < kUnbounded)) d = INFINITY;  // fewer than k participants in the seed (+inf padding), or nothing a threshold can use
  a.bound[s] = d;
  if (d == INFINITY) atomicAdd(a.counters + kUnboundedRows, 1ull);
}

// per block: its largest finite bound, -inf where it has none
__global__ void knn_block_max_kernel(const float *bound, uint32_t nblocks, float *bmax) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblocks) return;
  float m = -INFINITY;
  for (uint32_t v = 0; v < 64u; ++v) {
    const float x = bound[(size_t)b * 64u + v];
    if (x < INFINITY) m = fmaxf(m, x);
  }
  bmax[b] = m;
}

// ---- step 2: frame, threshold and image of every row of a chunk; one wave per row ----
struct KnnPrepareArgs {
  SelectCommon c;
  const uint32_t *self_slot;
  const float *bound;
  uint32_t m, nc;
  float *thr;
  float2 *frame;  // (qn, E)
  uint4 *qimg;
};

__global__ void __launch_bounds__(256) flat_knn_prepare_kernel(KnnPrepareArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (q >= a.m) return;
  const QueryFrame f = query_frame<false>(a.c, q, lane, nullptr, nullptr);
  const float B = a.bound[a.self_slot[q]];
  if (lane == 0) {
    a.thr[q] = B > -INFINITY ? radius_rank_threshold(a.c, f, B) : -INFINITY;  // (B = +inf: +inf, every record is evaluated)
    a.frame[q] = make_float2(f.qn, f.E);
  }
  split_query_image(a.c, q, a.nc, lane, a.qimg);
}

// before a sweep of the whole graph: the per-row counts and cursors, the cursor and the survivor count start over
__global__ void flat_knn_clear_kernel(uint32_t *cnt, uint32_t *fill, uint32_t n, unsigned long long *counters) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == kCursor || i == kSurvivors) counters[i] = 0ull;
  if (i < n) { cnt[i] = 0u; fill[i] = 0u; }
}

// ---- step 3: the sweep ----
struct KnnSweepArgs {
  const uint4 *img;     // the lists' bf16 image: [block][chunk][plane][half][64 columns] x 16 B (rank_images.hip)
  const float *xnorm;   // squared norms in image-column order, kBig on pad slots and on slots a filter excludes
  const uint4 *qimg;    // the chunk's rows: [row][plane][chunk][half] x 16 B (flat_common.hpp: split_query_image)
  const float4 *blocks;
  const float *Q;       // the chunk's rows, their stored bits
  const uint32_t *block_ord, *block_cnt;
  const uint64_t *allow;       // one allow word per block, or null
  const float *thr;            // [m] -inf: the row takes no part
  const float2 *frame;         // [m] (qn, E) of the row's frame
  const uint32_t *self_slot;   // [m] ascending: rows are in list order
  const float *bound;          // [nblocks * 64] by slot: B >= 0, +inf unbounded, -inf no participant
  const float *bmax;           // [nblocks] the block's largest finite bound, or -inf
  uint32_t *cnt;               // [N] entries of every row of the whole graph
  uint64_t *pool_key;
  uint32_t *pool_q;
  unsigned long long pool_cap;
  unsigned long long *counters;
  float gamma;          // SelectCommon::gamma of the frame the thresholds were formed in
  uint32_t row0;        // the list-order ordinal of the chunk's first row
  uint32_t m, dim, dq, nc, nblocks, seg;
  uint32_t lo_planes;   // the lists' lo planes are multiplied (some stored value is not bf16-exact)
  uint32_t keep_self;   // the pair (u, u) is one entry of u's row
};

// LDS, in 16-byte words: two K-step buffers, the norms and the bounds of two blocks, the waves' survivor queues —
// 2 x 32 KB + 0.5 KB + 0.5 KB + 8 KB = 73 KB with the rows RESIDENT in registers at D = 128: two workgroups per CU
__host__ __device__ inline uint32_t knn_step_words(bool resident, uint32_t nc) {
  return resident ? nc * 256u : kStreamChunks * (256u + 512u);
}
__host__ __device__ inline uint32_t knn_lds_words(bool resident, uint32_t nc) {
  return 2u * knn_step_words(resident, nc) + 32u + 32u + 4u * kQueueLen * 2u / 16u;
}

template <bool RESIDENT>
__global__ void __launch_bounds__(256, 2) flat_knn_sweep_kernel(KnnSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_knn[];
  const uint32_t q0 = blockIdx.x * kTileRows;
  // ---- the triangular split: this workgroup's blocks, from the block of the tile's first row on ----
  const uint32_t b_lo = max(blockIdx.y * a.seg, a.self_slot[q0] >> 6), b_hi = min((blockIdx.y + 1u) * a.seg, a.nblocks);
  if (b_lo >= b_hi) return;  // (workgroup-uniform, before any barrier)

  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const uint32_t nc = a.nc, kc = RESIDENT ? nc : kStreamChunks, nslab = RESIDENT ? 1u : (nc + kc - 1) / kc;
  const uint32_t bufsz = knn_step_words(RESIDENT, nc);
  float *s_norm = (float *)(s_knn + 2 * bufsz);  // [2][64] by K-step buffer
  float *s_bound = s_norm + 128;                 // [2][64] by the parity of the block within the segment: read in the
                                                 // block's LAST K step, while the next block's first is being staged
  uint16_t *s_queue = (uint16_t *)(s_bound + 128) + (uint32_t)wave * kQueueLen;
  const uint32_t nsteps = (b_hi - b_lo) * nslab;
  const uint64_t below = (1ull << lane) - 1ull;

  const uint32_t w0 = q0 + 32u * (uint32_t)wave, qg = w0 + (uint32_t)j;  // this lane's row: both lane halves hold column j
  const float thr = qg < a.m ? a.thr[qg] : -INFINITY;                    // (-inf: no row, or one the filter does not admit)
  const bool lane_live = thr > -INFINITY;
  const bool wave_live = __ballot(lane_live) != 0ull;
  const uint32_t wave_first = w0 < a.m ? a.self_slot[w0] >> 6 : ~0u;    // no block below it holds a slot above a row of the wave
  // the lane's frame, for the threshold of the block's largest bound: the fields radius_rank_threshold reads
  const float2 fr2 = qg < a.m ? a.frame[qg] : make_float2(0.0f, 0.0f);
  QueryFrame fr;
  fr.qn = fr2.x; fr.E = fr2.y; fr.qn_int = 0u; fr.q_bytes = false; fr.distrust = !(fr2.x < 1.0e30f);
  SelectCommon sc{};
  sc.dim = a.dim; sc.gamma = a.gamma;

  // RESIDENT: the B fragments of this lane's row, hi and lo, of every chunk: 2 x 4 VGPRs per chunk, read once.  The loop
  // is unrolled over the most chunks there can be, under a wave-uniform guard, so that every index is a constant
  bf16x8 bh[kMaxChunks], bl[kMaxChunks];
  if (RESIDENT) {
    const uint4 *qi = a.qimg + (size_t)min(qg, a.m - 1u) * 4 * nc;  // (a tile's tail repeats the last row)
#pragma unroll
    for (uint32_t c = 0; c < kMaxChunks; ++c) {
      uint4 vh = make_uint4(0u, 0u, 0u, 0u), vl = vh;
      if (c < nc) { vh = qi[2 * c + (uint32_t)h]; vl = qi[2 * nc + 2 * c + (uint32_t)h]; }
      bh[c] = __builtin_bit_cast(bf16x8, vh);
      bl[c] = __builtin_bit_cast(bf16x8, vl);
    }
  }

  // streaming: chunks [c0, c0 + kcs) of the tile's row image -> dst: piece (chunk, plane, half) of 128 rows = 2 KB
  auto stage_rows = [&](float *dst, uint32_t c0, uint32_t kcs) {
    for (uint32_t pi = wave; pi < kcs * 8u; pi += 4u) {
      const uint32_t piece = pi >> 1, qh = pi & 1u, c = piece >> 2, pc = piece & 3u;
      const uint32_t q = min(q0 + 64u * qh + (uint32_t)lane, a.m - 1u);
      glds16_asm(a.qimg + (size_t)q * 4 * nc + (pc >> 1) * 2 * nc + 2 * (c0 + c) + (pc & 1u), dst + (piece * 128u + 64u * qh) * 4u);
    }
  };
  // K step `step` of this workgroup -> buffer `buf`; a block's first step brings its norms (wave 0) and bounds (wave 1)
  auto stage = [&](uint32_t step, uint32_t buf) {
    const uint32_t b = b_lo + step / nslab, s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    float *dst = (float *)(s_knn + buf * bufsz);
    const uint4 *src = a.img + ((size_t)b * nc + c0) * 256 + lane;
    for (uint32_t p = wave; p < kcs * 4u; p += 4u) glds16_asm(src + p * 64u, dst + p * 256u);
    if (!RESIDENT) stage_rows(dst + kStreamChunks * 1024u, c0, kcs);
    if (s == 0 && wave == 0) glds4_asm(a.xnorm + (size_t)b * kWave + lane, s_norm + buf * 64u);
    if (s == 0 && wave == 1) glds4_asm(a.bound + (size_t)b * kWave + lane, s_bound + ((b - b_lo) & 1u) * 64u);
  };

  f32x16 acc0, acc1;  // vectors 0..31 and 32..63 of the block's image x this wave's 32 rows
  uint32_t nsurv = 0;

  // chunk c of the K step in s_a against the B fragments (fh, fl): the three products of bf16 x 3
  auto multiply = [&](const uint4 *s_a, uint32_t c, const bf16x8 &fh, const bf16x8 &fl) {
    const bf16x8 h0 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 0u + h) * 64u + j]);
    const bf16x8 h1 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 0u + h) * 64u + 32u + j]);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, fh, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, fh, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, fl, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, fl, acc1, 0, 0, 0);
    if (a.lo_planes) {
      const bf16x8 l0 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 2u + h) * 64u + j]);
      const bf16x8 l1 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 2u + h) * 64u + 32u + j]);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(l0, fh, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(l1, fh, acc1, 0, 0, 0);
    }
  };

  // delta of block b in this lane's frame: thr_u(r) - r does not decrease in r, so every bound of the block at or under
  // Bmax_b is covered by the value at Bmax_b; the slack covers the roundings of thr_u on both sides and of x - B_v
  auto v_side_delta = [&](uint32_t b) -> float {
    const float bm = a.bmax[b];
    if (!(bm > -INFINITY)) return -INFINITY;  // no finite bound in the block: only B_v = +inf passes (x - B_v = -inf)
    const float t = radius_rank_threshold(sc, fr, bm);
    return (t - bm) + kDeltaSlack * (bm + 2.0f * fr.qn + fr.E + fabsf(t));  // (t = +inf: +inf, everything passes)
  };

  auto emit = [&](unsigned long long pos, uint32_t row, uint32_t other, float d) {
    if (pos < a.pool_cap) {  // (nothing is written past the pool; everything is counted)
      a.pool_key[pos] = ((uint64_t)__float_as_uint(d) << 32) | other;
      a.pool_q[pos] = row;
    }
    atomicAdd(a.cnt + row, 1u);
  };

  // ---- epilogue of one accumulator tile: register r of tile t in lane half h is vector 32 t + 16 h + r of the block ----
  auto epilogue = [&](const f32x16 &acc, uint32_t t, uint32_t b, float delta) {
    const float *bv = s_bound + ((b - b_lo) & 1u) * 64u + 32u * t + 16u * (uint32_t)h;
    uint32_t m = 0u;
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const float4 B = *reinterpret_cast<const float4 *>(bv + 4 * q4);
      // (!(x > y): a NaN rank value is evaluated, never skipped)
      m |= ((!(acc[4 * q4 + 0] > thr) || !(acc[4 * q4 + 0] - B.x > delta)) ? 1u : 0u) << (4 * q4 + 0);
      m |= ((!(acc[4 * q4 + 1] > thr) || !(acc[4 * q4 + 1] - B.y > delta)) ? 1u : 0u) << (4 * q4 + 1);
      m |= ((!(acc[4 * q4 + 2] > thr) || !(acc[4 * q4 + 2] - B.z > delta)) ? 1u : 0u) << (4 * q4 + 2);
      m |= ((!(acc[4 * q4 + 3] > thr) || !(acc[4 * q4 + 3] - B.w > delta)) ? 1u : 0u) << (4 * q4 + 3);
    }
    if (!lane_live) m = 0u;
    if (__ballot(m != 0u) == 0ull) return;
    uint32_t n = 0;  // survivors, compacted into the wave's queue
    for (uint32_t bit = 0; bit < 16u; ++bit) {
      const bool sv = (m >> bit) & 1u;
      const uint64_t bal = __ballot(sv);
      if (!bal) continue;
      if (sv) s_queue[n + (uint32_t)__popcll(bal & below)] = (uint16_t)((uint32_t)j | ((32u * t + 16u * (uint32_t)h + bit) << 5));
      n += (uint32_t)__popcll(bal);
    }
    wave_lds_sync();
    nsurv += n;
    const uint32_t nrec = a.block_cnt[b], ord0 = a.block_ord[b];
    const uint64_t allow = a.allow ? a.allow[b] : ~0ull;
    // ---- the drain: 64 entries a round; one evaluation per pair, up to two directed entries ----
    for (uint32_t at = 0; at < n; at += kWave) {
      const uint32_t i = at + (uint32_t)lane;
      const uint32_t e = i < n ? s_queue[i] : 0u;
      const uint32_t q = w0 + (e & 31u), v = e >> 5, sv = b * (uint32_t)kWave + v;
      bool to_u = false, to_v = false;
      float d = INFINITY;
      if (i < n && q < a.m && v < nrec && ((allow >> v) & 1ull)) {  // a record (no pad slot) that the filter admits
        const uint32_t su = a.self_slot[q];
        if (sv > su || (sv == su && a.keep_self)) {  // the pair's one visit is from its lower slot
          d = exact_scalar(a.Q + (size_t)q * a.dim, a.blocks + (size_t)b * a.dq * kWave + v, a.dim);
          to_u = d <= a.bound[su];
          to_v = sv != su && d <= a.bound[sv];
        }
      }
      const uint64_t bu = __ballot(to_u), bw = __ballot(to_v);
      if (!(bu | bw)) continue;
      unsigned long long base = 0ull;  // the round's entries take one range of the pool
      if (lane == 0) base = atomicAdd(a.counters + kCursor, (unsigned long long)(__popcll(bu) + __popcll(bw)));
      const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
      const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
      unsigned long long pos = (((unsigned long long)bhi << 32) | blo) + (uint32_t)(__popcll(bu & below) + __popcll(bw & below));
      const uint32_t ord_u = a.row0 + q, ord_v = ord0 + v;
      if (to_u) emit(pos++, ord_u, ord_v, d);
      if (to_v) emit(pos, ord_v, ord_u, d);
    }
    wave_lds_sync();  // the queue is free again
  };

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (uint32_t step = 0; step < nsteps; ++step) {
    const uint32_t cur = step & 1u;
    const uint32_t b = b_lo + step / nslab, s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    // the next step lands in the other buffer under this step's MFMAs (every wave left it at the last barrier)
    if (step + 1 < nsteps) stage(step + 1, cur ^ 1u);
    if (wave_live && b >= wave_first) {  // (a block below every row of the wave holds no slot above one)
      const uint4 *s_a = s_knn + cur * bufsz;
      if (s == 0) {
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {  // vectors 8 q4 + 4 h + (0..3) of a tile live in registers 4 q4 .. 4 q4 + 3
          const float4 n0 = *reinterpret_cast<const float4 *>(s_norm + cur * 64u + 8 * q4 + 4 * h);
          const float4 n1 = *reinterpret_cast<const float4 *>(s_norm + cur * 64u + 32 + 8 * q4 + 4 * h);
          acc0[4 * q4 + 0] = n0.x; acc0[4 * q4 + 1] = n0.y; acc0[4 * q4 + 2] = n0.z; acc0[4 * q4 + 3] = n0.w;
          acc1[4 * q4 + 0] = n1.x; acc1[4 * q4 + 1] = n1.y; acc1[4 * q4 + 2] = n1.z; acc1[4 * q4 + 3] = n1.w;
        }
      }
      if (RESIDENT) {
#pragma unroll
        for (uint32_t c = 0; c < kMaxChunks; ++c)
          if (c < nc) multiply(s_a, c, bh[c], bl[c]);
      } else {
        const uint4 *s_b = s_a + kStreamChunks * 256u;
        for (uint32_t c = 0; c < kcs; ++c) {
          const bf16x8 fh = __builtin_bit_cast(bf16x8, s_b[(c * 4u + 0u + h) * 128u + 32u * wave + j]);
          const bf16x8 fl = __builtin_bit_cast(bf16x8, s_b[(c * 4u + 2u + h) * 128u + 32u * wave + j]);
          multiply(s_a, c, fh, fl);
        }
      }
      if (s + 1 == nslab) {  // the queue is drained once per accumulator tile: 32 x 32 entries can never overflow it
        const float delta = v_side_delta(b);
        epilogue(acc0, 0u, b, delta);
        epilogue(acc1, 1u, b, delta);
      }
    }
    // the next step has landed (this wave's loads, stores and atomics too), every wave is done with this buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  if (lane == 0 && nsurv) atomicAdd(a.counters + kSurvivors, (unsigned long long)nsurv);
}

// ---- step 4: sorted rows -> the caller's k-wide rows; one wave per row ----
struct KnnTakeArgs {
  const uint64_t *rows;   // every row's keys, ascending
  const uint64_t *lims;   // [n + 1]
  const uint32_t *block_ord;
  const uint64_t *ext_ids;
  uint32_t nblocks, k, n;
  float *D;
  int64_t *I;
  uint64_t *ord, *counts;  // or null
};

__global__ void __launch_bounds__(256) flat_knn_take_kernel(KnnTakeArgs o) {
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (q >= o.n) return;
  const uint64_t at = o.lims[q], len = min(o.lims[q + 1] - at, (uint64_t)o.k);
  for (uint32_t i = lane; i < o.k; i += 64u) {
    const size_t out = (size_t)q * o.k + i;
    if (i >= len) {
      o.D[out] = INFINITY; o.I[out] = -1;
      if (o.ord) o.ord[out] = kNoKey;
      continue;
    }
    const uint64_t key = o.rows[at + i];
    const uint32_t ordinal = (uint32_t)key, b = block_of_ordinal(o.block_ord, o.nblocks, ordinal);
    o.D[out] = __uint_as_float((uint32_t)(key >> 32));
    o.I[out] = (int64_t)o.ext_ids[(size_t)b * kWave + (ordinal - o.block_ord[b])];
    if (o.ord) o.ord[out] = ordinal;
  }
  if (o.counts && lane == 0) o.counts[q] = len;
}

thread_local vi_exact_knn_stats g_last_stats{};

struct KnnCall {
  const DeviceIndex &ix;
  SearchContext &ctx;
  const ExactKnnIO &io;
  vi_exact_knn_stats es{};
  bool timing = false;
  double t_last = 0.0;
  int cus = 1;
  DevBuf<float> bound, bmax;  // the call's scratch; freed on return
  DevBuf<float2> frame;
  unsigned long long cursor = 0;  // directed entries the last sweep counted

  KnnCall(const DeviceIndex &ix_, SearchContext &ctx_, const ExactKnnIO &io_) : ix(ix_), ctx(ctx_), io(io_) {
    const char *te = getenv("VI_EXACT_TIMING");
    timing = te && *te != '0';
    es.rows = ix.nvec_resident; es.k = io.k;
    es.seed_probe = std::min<uint64_t>(io.seed_probe ? io.seed_probe : kExactSeedProbe, std::max<uint64_t>(1, ix.nlists));
    t_last = now_ms();
  }
  vi_status lap(float &ms) {  // (VI_EXACT_TIMING) the phase that ends here
    if (!timing) return VI_OK;
    VI_HIP(hipStreamSynchronize(ctx.stream));
    const double t = now_ms();
    ms += (float)(t - t_last);
    t_last = t;
    return VI_OK;
  }

  // ---- pass 1: the bound of every slot from a seeding search of every chunk ----
  vi_status seed() {
    SearchWorkspace &ws = ctx.ws;
    auto &fr = ws.flat_range;
    hipStream_t st = ctx.stream;
    const uint32_t nblocks = (uint32_t)ix.lists.nblocks, nslots = nblocks * 64u;
    const uint64_t k = io.k, kk = k + (io.exclude_self ? 1 : 0);
    VI_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix.device));
    VI_TRY(ensure_fetch_layout(ix, st));
    VI_HIP(hipSetDevice(ix.device));
    VI_TRY(fr.block_ord.reserve(nblocks));
    VI_TRY(fr.block_cnt.reserve(nblocks));
    VI_TRY(fr.counters.reserve(kKnnCounters));
    VI_TRY(bound.reserve(nslots));
    VI_TRY(bmax.reserve(nblocks));
    hipLaunchKernelGGL(flat_blocks_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, st, ix.list_first_block.p, ix.list_len.p,
                       ix.fetch.prefix.p, (uint32_t)ix.nlists, nblocks, fr.block_ord.p, fr.block_cnt.p);
    VI_HIP(hipGetLastError());
    hipLaunchKernelGGL(knn_clear_bounds_kernel, dim3((nslots + 255) / 256), dim3(256), 0, st, bound.p, nslots, fr.counters.p);
    VI_HIP(hipGetLastError());
    const uint64_t *allow = io.filter ? io.filter->allow.p : nullptr;
    StoredRowsWalk walk(kk);
    StoredRows all;  // every resident record, in list order
    all.nq = ix.nvec_resident;
    const auto body = [&](const RowChunk &c) -> vi_status {
      const uint64_t m = c.m;
      VI_TRY(ws.D.reserve(m * kk));
      VI_TRY(ws.I.reserve(m * kk));
      VI_TRY(ws.slots.reserve(m * kk));
      SearchIO sio;
      sio.queries = ws.q.p; sio.on_device = true; sio.nq = m; sio.k = kk; sio.n_probe = es.seed_probe; sio.filter = io.filter;
      sio.D = ws.D.p; sio.I = ws.I.p; sio.slots = ws.slots.p;
      VI_TRY(topk_search(ix, ctx, sio));  // (synchronised)
      KnnBoundArgs ba{ws.D.p, ws.slots.p, ws.self_slot.p, allow, (uint32_t)m, (uint32_t)k, (uint32_t)kk, bound.p, fr.counters.p};
      hipLaunchKernelGGL(knn_bound_kernel, dim3((uint32_t)((m + 3) / 4)), dim3(256), 0, st, ba);
      VI_HIP(hipGetLastError());
      return VI_OK;
    };
    VI_TRY(walk.run(ix, ctx, all, body));
    hipLaunchKernelGGL(knn_block_max_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, st, (const float *)bound.p, nblocks, bmax.p);
    VI_HIP(hipGetLastError());
    return lap(es.ms_seed);
  }

  // blocks per segment for the chunk whose first row is q0 (§4t: some sixteen workgroups per CU over the rectangle of
  // row tiles x blocks from about the chunk's first on, of which a bare triangle keeps half)
  uint32_t segment_blocks(uint64_t q0, uint32_t ntiles) const {
    const uint64_t nblocks = ix.lists.nblocks, ahead = nblocks - std::min<uint64_t>(nblocks - 1, q0 * nblocks / std::max<uint64_t>(ix.nvec_resident, 1));
    const uint64_t s = (uint64_t)ntiles * ahead / (16ull * (uint64_t)std::max(cus, 1));
    return (uint32_t)std::max<uint64_t>(std::min<uint64_t>(std::max<uint64_t>(s, kSegMin), kSegMax), (nblocks + kMaxGridY - 1) / kMaxGridY);
  }

  // ---- pass 2: one sweep of the whole graph into a pool of `cap` entries ----
  vi_status sweep(uint64_t cap) {
    SearchWorkspace &ws = ctx.ws;
    auto &fr = ws.flat_range;
    hipStream_t st = ctx.stream;
    const uint64_t N = ix.nvec_resident;
    const uint32_t dim = ix.dim, nc = ix.dq / 4, nblocks = (uint32_t)ix.lists.nblocks;
    const bool resident = dim <= kNarrowDim;
    const int lds = (int)(knn_lds_words(resident, nc) * 16u);
    const void *fn = resident ? (const void *)flat_knn_sweep_kernel<true> : (const void *)flat_knn_sweep_kernel<false>;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
      return fail(VI_ERR_DEVICE, "cannot reserve %d bytes of LDS for the exact k-NN graph's sweep", lds);
    hipLaunchKernelGGL(flat_knn_clear_kernel, dim3(ceil_div_u32(N, 256)), dim3(256), 0, st, fr.cnt.p, fr.fill.p, (uint32_t)N, fr.counters.p);
    VI_HIP(hipGetLastError());
    StoredRowsWalk walk(64);
    es.chunk_rows = walk.chunk_rows;
    StoredRows all;
    all.nq = N;
    const auto body = [&](const RowChunk &c) -> vi_status {
      const uint64_t m = c.m;
      VI_TRY(fr.thr.reserve(m));
      VI_TRY(frame.reserve(m));
      VI_TRY(fr.qimg.reserve(m * nc * 16));
      // the frame of lists ranked with bf16 x 3 whatever the engines' switches say: this sweep multiplies nothing else
      SearchBatch b{ix, ctx, io.filter, nullptr, nullptr};
      b.kn = read_engine_knobs();
      b.kn.rank_bf16 = true; b.kn.stats = false;
      b.Qd = ws.q.p; b.nq = m;
      const SelectCommon sc = select_common(b, (const float4 *)ix.lists.blocks.p, ix.centered ? ix.xmax2_c : ix.xmax2, kTileRows);
      KnnPrepareArgs pa{sc, ws.self_slot.p, bound.p, (uint32_t)m, nc, fr.thr.p, frame.p, (uint4 *)fr.qimg.p};
      hipLaunchKernelGGL(flat_knn_prepare_kernel, dim3((uint32_t)((m + 3) / 4)), dim3(256), 0, st, pa);
      VI_HIP(hipGetLastError());
      VI_TRY(lap(es.ms_prepare));
      const uint32_t ntiles = (uint32_t)((m + kTileRows - 1) / kTileRows), seg = segment_blocks(c.q0, ntiles);
      const uint32_t nseg = (nblocks + seg - 1) / seg;
      es.tiles = std::max<uint64_t>(es.tiles, ntiles);
      es.segments = std::max<uint64_t>(es.segments, nseg);
      KnnSweepArgs a{};
      a.img = (const uint4 *)ix.lists_bf16.p; a.xnorm = io.filter ? io.filter->xnorm_img.p : ix.xnorm_img.p;
      a.qimg = (const uint4 *)fr.qimg.p; a.blocks = (const float4 *)ix.lists.blocks.p; a.Q = ws.q.p;
      a.block_ord = fr.block_ord.p; a.block_cnt = fr.block_cnt.p; a.allow = io.filter ? io.filter->allow.p : nullptr;
      a.thr = fr.thr.p; a.frame = frame.p; a.self_slot = ws.self_slot.p; a.bound = bound.p; a.bmax = bmax.p;
      a.cnt = fr.cnt.p; a.pool_key = fr.pool_key.p; a.pool_q = fr.pool_q.p; a.pool_cap = cap; a.counters = fr.counters.p;
      a.gamma = sc.gamma; a.row0 = (uint32_t)c.q0; a.m = (uint32_t)m; a.dim = dim; a.dq = ix.dq; a.nc = nc; a.nblocks = nblocks;
      a.seg = seg; a.lo_planes = ix.lists_lo_zero ? 0u : 1u; a.keep_self = io.exclude_self ? 0u : 1u;
      if (resident) hipLaunchKernelGGL(flat_knn_sweep_kernel<true>, dim3(ntiles, nseg), dim3(256), lds, st, a);
      else hipLaunchKernelGGL(flat_knn_sweep_kernel<false>, dim3(ntiles, nseg), dim3(256), lds, st, a);
      VI_HIP(hipGetLastError());
      return lap(es.ms_sweep);
    };
    const auto landed = [&](const RowChunk &) -> vi_status { if (timing) t_last = now_ms(); return VI_OK; };
    if (timing) t_last = now_ms();
    VI_TRY(walk.run(ix, ctx, all, body, landed));
    unsigned long long h_count[kKnnCounters] = {};
    VI_HIP(hipMemcpyAsync(h_count, fr.counters.p, sizeof(h_count), hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
    ++es.sweeps;
    es.survivors += h_count[kSurvivors];
    es.unbounded_rows = h_count[kUnboundedRows];
    cursor = h_count[kCursor];
    return VI_OK;
  }
};

vi_status knn_exact_in_context(const DeviceIndex &ix, SearchContext &ctx, const ExactKnnIO &io) {
  auto &fr = ctx.ws.flat_range;
  hipStream_t st = ctx.stream;
  const uint64_t N = ix.nvec_resident, k = io.k;
  const uint32_t nblocks = (uint32_t)ix.lists.nblocks;
  KnnCall kc(ix, ctx, io);
  if (N == 0 || nblocks == 0) {  // nothing is resident: no row to write
    g_last_stats = kc.es;
    return VI_OK;
  }
  VI_TRY(kc.seed());
  VI_TRY(reserve_csr_sort_lds());
  VI_TRY(fr.cnt.reserve(N));
  VI_TRY(fr.fill.reserve(N));
  // ---- the sweep, once more if the pool was too small ----
  uint64_t cap = exact_knn_pool_cap(io.pool_cap, k, N);
  for (uint32_t pass = 1; pass <= 2; ++pass) {
    VI_TRY(fr.pool_key.reserve(cap));
    VI_TRY(fr.pool_q.reserve(cap));
    kc.es.pool_cap = cap;
    VI_TRY(kc.sweep(cap));
    if (kc.cursor <= cap) break;
    if (pass == 2) return fail(VI_ERR_OTHER, "exact k-NN graph: the second sweep found more entries than the first counted");
    cap = kc.cursor;  // every entry was counted: the pool that holds them all
  }
  // ---- rows: sized from the counts, filled from the pool, sorted, cut at k ----
  const uint64_t total = kc.cursor;
  std::vector<uint32_t> h_cnt(N);
  std::vector<uint64_t> h_lims(N + 1, 0);
  VI_HIP(hipMemcpyAsync(h_cnt.data(), fr.cnt.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  for (uint64_t q = 0; q < N; ++q) h_lims[q + 1] = h_lims[q] + h_cnt[q];
  if (h_lims[N] != total) return fail(VI_ERR_OTHER, "exact k-NN graph: the per-row counts and the pool disagree");
  DevBuf<uint64_t> lims;
  VI_TRY(lims.reserve(N + 1));
  VI_HIP(hipMemcpyAsync(lims.p, h_lims.data(), (N + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  VI_TRY(fr.rows.reserve(std::max<uint64_t>(total, 1)));
  if (total) {
    hipLaunchKernelGGL(flat_range_place_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, (const uint64_t *)fr.pool_key.p,
                       (const uint32_t *)fr.pool_q.p, total, (const uint64_t *)lims.p, fr.fill.p, fr.rows.p);
    VI_HIP(hipGetLastError());
    VI_TRY(sort_csr_rows(lims.p, h_lims.data(), N, fr.rows.p, fr.longq, fr.pad, st));
  }
  // a host caller's rows are made on the device and copied once everything has succeeded
  DevBuf<float> D_stage;
  DevBuf<int64_t> I_stage;
  DevBuf<uint64_t> ord_stage, counts_stage;
  KnnTakeArgs o{fr.rows.p, lims.p, fr.block_ord.p, ix.ext_ids.p, nblocks, (uint32_t)k, (uint32_t)N, io.D, io.I, io.ord, io.counts};
  if (!io.on_device) {
    VI_TRY(D_stage.reserve(N * k));
    VI_TRY(I_stage.reserve(N * k));
    o.D = D_stage.p; o.I = I_stage.p;
    if (io.ord) { VI_TRY(ord_stage.reserve(N * k)); o.ord = ord_stage.p; }
    if (io.counts) { VI_TRY(counts_stage.reserve(N)); o.counts = counts_stage.p; }
  }
  hipLaunchKernelGGL(flat_knn_take_kernel, dim3((uint32_t)((N + 3) / 4)), dim3(256), 0, st, o);
  VI_HIP(hipGetLastError());
  VI_HIP(hipStreamSynchronize(st));  // (h_lims is read by its upload until here)
  if (!io.on_device) {
    VI_HIP(hipMemcpyAsync(io.D, o.D, N * k * sizeof(float), hipMemcpyDeviceToHost, st));
    VI_HIP(hipMemcpyAsync(io.I, o.I, N * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (io.ord) VI_HIP(hipMemcpyAsync(io.ord, o.ord, N * k * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (io.counts) VI_HIP(hipMemcpyAsync(io.counts, o.counts, N * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
  }
  VI_TRY(kc.lap(kc.es.ms_finish));
  kc.es.candidates = total;
  g_last_stats = kc.es;
  return VI_OK;
}

// the limits of the exact self-joins (§4t): VI_ERR_INVALID_INPUT before any device work
vi_status knn_limits(const DeviceIndex &ix, const ExactKnnIO &io) {
  if (ix.stripe_world > 1) return fail(VI_ERR_INVALID_INPUT, "the exact k-NN graph needs the whole index on one handle");
  if (ix.order != VI_ORDER_SCALAR) return fail(VI_ERR_INVALID_INPUT, "the exact k-NN graph needs an index whose distances are VI_ORDER_SCALAR");
  if (ix.dim < 4 || (ix.dim & 3) || ix.dim > kMaxMfmaDim)
    return fail(VI_ERR_INVALID_INPUT, "the exact k-NN graph needs a dimension that is a multiple of 4 and at most %u, not %u", kMaxMfmaDim, ix.dim);
  if (ix.lists.nblocks * 64ull >= (1ull << kPosBits))
    return fail(VI_ERR_INVALID_INPUT, "the exact k-NN graph needs an index of fewer than 2^%u slots", kPosBits);
  if (!(ix.xmax2 < 1.0e30f)) return fail(VI_ERR_INVALID_INPUT, "the exact k-NN graph needs stored vectors of squared norm below 1e30");
  if (ix.lists.nblocks && !ix.lists_bf16.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no ranking images");
  if (io.filter && io.filter->owner_serial != ix.serial) return fail(VI_ERR_INVALID_INPUT, "the filter was made for another index");
  return VI_OK;
}

}  // namespace

vi_exact_knn_stats exact_knn_last_stats() { return g_last_stats; }

vi_status device_index_knn_graph_exact(const DeviceIndex &ix, const ExactKnnIO &io) {
  g_last_stats = vi_exact_knn_stats{};
  VI_TRY(knn_limits(ix, io));
  const vi_status s = stored_record_call(ix, g_last_stats, [&](SearchContext &ctx) { return knn_exact_in_context(ix, ctx, io); });
  if (s != VI_OK) g_last_stats = vi_exact_knn_stats{};
  return s;
}

}  // namespace vi
