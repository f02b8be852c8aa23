// flat_range.hip — exact (flat) radius search over every resident record: one dense sweep of ALL blocks against ALL queries
// on the matrix cores, out to CSR (the contract is vi_indexer_range_search_exact in include/vi_amd.h).
//
//   1. prepare  flat_range_prepare_kernel, one wave per query: the rank threshold of the query's radius in the query's
//               frame (query_frame, rank_threshold and w as the radius select forms them: known before a record is read, so
//               there is no seeding search and no overflow path), -inf for an empty row, and the bf16 hi / lo image.
//   2. sweep    flat_range_sweep_kernel: a workgroup owns 128 queries and a strided share of all blocks; a wave owns one
//               32-column tile.  D <= 128: the wave keeps its queries' B fragments in registers for the whole sweep, LDS
//               holds only the double-buffered block images, so two workgroups share a CU.  Per 64-vector block it
//               accumulates ||v||^2 - 2 q.v (hi.hi + hi.lo + lo.hi), compares, ballots; the survivors of each 32 x 32
//               accumulator tile are queued, evaluated in the reference's chain, and those with d <= radius go to a pool of
//               (key = distance bits << 32 | ordinal, query) under ONE atomicAdd per drain on a global cursor.  Past the
//               pool's capacity nothing is written and everything is still counted.
//   3. size     the host reads the cursor: a pool that was too small grows to the count and the sweep runs once more.
//               range_result_place sizes lims and the result from the per-query counts.
//   4. place    (flat_rows.hpp) flat_range_place_kernel scatters the pool into the rows; flat_range_sort_kernel sorts every row of up to
//               8192 keys in LDS, longer rows go through sort_rows_u64 on padded scratch; flat_range_output_kernel writes
//               D / I / tie (the ordinal) / slot.
// Neither the order hits arrive in nor the second sweep shows in a result; no result depends on a rank value.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "device_index.hpp"
#include "flat_common.hpp"
#include "flat_range.hpp"
#include "flat_rows.hpp"
#include "flat_search.hpp"
#include "mfma_bf16.hpp"
#include "record_fetch.hpp"
#include "search_internal.hpp"
#include "select_device.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

constexpr uint32_t kTileQ = 128;       // queries per workgroup: four waves of one 32-column B tile each
constexpr uint32_t kMaxChunks = 8;     // D <= 128: chunks of 16 dimensions whose B fragments a wave keeps in registers
constexpr uint32_t kStreamChunks = 2;  // D > 128: chunks per K step (both operands stream through LDS)
constexpr uint32_t kQueueLen = 1024;   // survivors of one wave and accumulator tile: 32 queries x 32 vectors, never more

enum { kCursor = 0, kSurvivors = 1, kCounters = 2 };

// ---- step 1: threshold, radius and image of every query; one wave per query ----
struct RangePrepareArgs {
  SelectCommon c;
  const float *radii;  // per query, or null: radius2
  float radius2;
  uint32_t nq, nc;
  float *thr, *rad;    // rad: the radius the exact distances are compared with, -1 for an empty row
  uint32_t *cnt, *fill;
  uint4 *qimg;
  unsigned long long *counters;
};

__global__ void __launch_bounds__(256) flat_range_prepare_kernel(RangePrepareArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x < kCounters) a.counters[threadIdx.x] = 0ull;
  if (q >= a.nq) return;
  const QueryFrame f = query_frame<false>(a.c, q, lane, nullptr, nullptr);
  const float r = a.radii ? a.radii[q] : a.radius2;
  const bool empty = !(r >= 0.0f);  // negative or NaN: no squared distance is within it
  const float thr = radius_rank_threshold(a.c, f, r);
  if (lane == 0) {
    a.thr[q] = empty ? -INFINITY : thr;
    a.rad[q] = empty ? -1.0f : r;
    a.cnt[q] = 0u;
    a.fill[q] = 0u;
  }
  split_query_image(a.c, q, a.nc, lane, a.qimg);
}

// between two sweeps of a chunk: the counts start over
__global__ void flat_range_clear_kernel(uint32_t *cnt, uint32_t nq, unsigned long long *counters) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < kCounters) counters[q] = 0ull;
  if (q < nq) cnt[q] = 0u;
}

// ---- step 2: the sweep ----
struct RangeSweepArgs {
  const uint4 *img;     // the lists' bf16 image: [block][chunk][plane][half][64 columns] x 16 B (rank_images.hip)
  const float *xnorm;   // squared norms in image-column order, kBig on pad slots and on slots a filter excludes
  const uint4 *qimg;    // [query][plane][chunk][half] x 16 B (flat_common.hpp: split_query_image)
  const float4 *blocks;
  const float *Q;
  const uint32_t *block_ord, *block_cnt;
  const uint64_t *allow;  // one allow word per block, or null
  const float *thr, *rad;
  uint32_t *cnt;
  uint64_t *pool_key;
  uint32_t *pool_q;
  unsigned long long *counters;
  unsigned long long pool_cap;
  uint32_t nq, dim, dq, nc, nblocks, nsplit;
  uint32_t lo_planes;     // the lists' lo planes are multiplied (some stored value is not bf16-exact)
};

// LDS, in 16-byte words: two K-step buffers, the norms of two blocks, the waves' survivor queues.  A K step holds a
// block's whole image when the queries are RESIDENT in registers — 2 x 32 KB + 0.5 KB + 8 KB = 72.5 KB at D = 128, two
// workgroups per CU — and otherwise kStreamChunks chunks of it with the same chunks of the tile's 128 queries behind them.
__host__ __device__ inline uint32_t range_step_words(bool resident, uint32_t nc) {
  return resident ? nc * 256u : kStreamChunks * (256u + 512u);
}
__host__ __device__ inline uint32_t range_lds_words(bool resident, uint32_t nc) {
  return 2u * range_step_words(resident, nc) + 32u + 4u * kQueueLen * 2u / 16u;
}

template <bool RESIDENT>
__global__ void __launch_bounds__(256, 2) flat_range_sweep_kernel(RangeSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_rng[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const uint32_t nc = a.nc, kc = RESIDENT ? nc : kStreamChunks, nslab = RESIDENT ? 1u : (nc + kc - 1) / kc;
  const uint32_t bufsz = range_step_words(RESIDENT, nc);
  float *s_norm = (float *)(s_rng + 2 * bufsz);  // [2][64]
  uint16_t *s_queue = (uint16_t *)(s_norm + 128) + (uint32_t)wave * kQueueLen;
  const uint32_t q0 = blockIdx.x * kTileQ, split = blockIdx.y;
  if (split >= a.nblocks) return;  // (the host launches nsplit <= nblocks)
  const uint32_t nmine = (a.nblocks - split + a.nsplit - 1) / a.nsplit, nsteps = nmine * nslab;
  const uint64_t below = (1ull << lane) - 1ull;

  const uint32_t qg = q0 + 32u * (uint32_t)wave + (uint32_t)j;  // this lane's query: both lane halves hold column j
  const float thr = qg < a.nq ? a.thr[qg] : -INFINITY;          // (-inf: no query, or an empty row)
  const bool lane_live = thr > -INFINITY;
  const bool wave_live = __ballot(lane_live) != 0ull;

  // RESIDENT: the B fragments of this lane's query, hi and lo, of every chunk: 2 x 4 VGPRs per chunk, read once.  The loop
  // is unrolled over the most chunks there can be, under a wave-uniform guard, so that every index is a constant
  bf16x8 bh[kMaxChunks], bl[kMaxChunks];
  if (RESIDENT) {
    const uint4 *qi = a.qimg + (size_t)min(qg, a.nq - 1u) * 4 * nc;  // (a tile's tail repeats the last query)
#pragma unroll
    for (uint32_t c = 0; c < kMaxChunks; ++c) {
      uint4 vh = make_uint4(0u, 0u, 0u, 0u), vl = vh;
      if (c < nc) { vh = qi[2 * c + (uint32_t)h]; vl = qi[2 * nc + 2 * c + (uint32_t)h]; }
      bh[c] = __builtin_bit_cast(bf16x8, vh);
      bl[c] = __builtin_bit_cast(bf16x8, vl);
    }
  }

  // streaming: chunks [c0, c0 + kcs) of the tile's query image -> dst: piece (chunk, plane, half) of 128 queries = 2 KB
  auto stage_queries = [&](float *dst, uint32_t c0, uint32_t kcs) {
    for (uint32_t pi = wave; pi < kcs * 8u; pi += 4u) {
      const uint32_t piece = pi >> 1, qh = pi & 1u, c = piece >> 2, pc = piece & 3u;
      const uint32_t q = min(q0 + 64u * qh + (uint32_t)lane, a.nq - 1u);
      glds16_asm(a.qimg + (size_t)q * 4 * nc + (pc >> 1) * 2 * nc + 2 * (c0 + c) + (pc & 1u), dst + (piece * 128u + 64u * qh) * 4u);
    }
  };
  // K step `step` of this workgroup -> buffer `buf`
  auto stage = [&](uint32_t step, uint32_t buf) {
    const uint32_t b = split + (step / nslab) * a.nsplit, s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    float *dst = (float *)(s_rng + buf * bufsz);
    const uint4 *src = a.img + ((size_t)b * nc + c0) * 256 + lane;
    for (uint32_t p = wave; p < kcs * 4u; p += 4u) glds16_asm(src + p * 64u, dst + p * 256u);
    if (!RESIDENT) stage_queries(dst + kStreamChunks * 1024u, c0, kcs);
    if (s == 0 && wave == 0) glds4_asm(a.xnorm + (size_t)b * kWave + lane, s_norm + buf * 64u);
  };

  f32x16 acc0, acc1;  // rows 0..31 and 32..63 of the block's image x this wave's 32 queries
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

  // queue entry e = (query of the wave | vector << 5) of block b, one per lane: its exact distance where the record is
  // admitted (no pad slot, let through by the filter) -> a hit?
  auto evaluate = [&](uint32_t b, uint32_t e, bool live, uint32_t nrec, uint64_t allow, uint32_t &q, uint32_t &v, float &d) {
    q = q0 + 32u * (uint32_t)wave + (e & 31u);
    v = e >> 5;
    d = INFINITY;
    if (!(live && q < a.nq && v < nrec && ((allow >> v) & 1ull))) return false;
    d = exact_scalar(a.Q + (size_t)q * a.dim, a.blocks + (size_t)b * a.dq * kWave + v, a.dim);
    return d <= a.rad[q];
  };
  // `nh` hits of the wave take one range of the pool
  auto take_range = [&](uint32_t nh) {
    unsigned long long base = 0ull;
    if (lane == 0) base = atomicAdd(a.counters + kCursor, (unsigned long long)nh);
    const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
    const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
    return ((unsigned long long)bhi << 32) | blo;
  };
  auto emit = [&](unsigned long long pos, uint32_t q, uint32_t ordinal, float d) {
    if (pos < a.pool_cap) {  // (nothing is written past the pool; everything is counted)
      a.pool_key[pos] = ((uint64_t)__float_as_uint(d) << 32) | ordinal;
      a.pool_q[pos] = q;
    }
    atomicAdd(a.cnt + q, 1u);
  };

  // ---- epilogue of one accumulator tile: register r of tile t in lane half h is vector 32 t + 16 h + r of the block ----
  auto epilogue = [&](const f32x16 &acc, uint32_t t, uint32_t b) {
    uint32_t m = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) m |= (!(acc[r] > thr) ? 1u : 0u) << r;  // (!(x > thr): a NaN rank value is evaluated, never skipped)
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
    uint32_t q, v;
    float d;
    if (n <= (uint32_t)kWave) {  // the common drain: one round, the distances stay in registers
      const bool hit = evaluate(b, (uint32_t)lane < n ? s_queue[lane] : 0u, (uint32_t)lane < n, nrec, allow, q, v, d);
      const uint64_t bal = __ballot(hit);
      if (bal) {
        const unsigned long long base = take_range((uint32_t)__popcll(bal));
        if (hit) emit(base + (uint32_t)__popcll(bal & below), q, ord0 + v, d);
      }
    } else {  // a crowded tile: the hits are compacted in place first, so that the drain still takes ONE range; they are evaluated again to be written
      uint32_t nh = 0;
      for (uint32_t at = 0; at < n; at += kWave) {
        const uint32_t i = at + (uint32_t)lane, e = i < n ? s_queue[i] : 0u;
        const bool hit = evaluate(b, e, i < n, nrec, allow, q, v, d);
        const uint64_t bal = __ballot(hit);
        wave_lds_sync();  // (every lane has read its entry: the hits land at or below the places read so far)
        if (hit) s_queue[nh + (uint32_t)__popcll(bal & below)] = (uint16_t)e;
        nh += (uint32_t)__popcll(bal);
      }
      wave_lds_sync();
      if (nh) {
        const unsigned long long base = take_range(nh);
        for (uint32_t at = 0; at < nh; at += kWave) {
          const uint32_t i = at + (uint32_t)lane;
          if (evaluate(b, i < nh ? s_queue[i] : 0u, i < nh, nrec, allow, q, v, d)) emit(base + i, q, ord0 + v, d);
        }
      }
    }
    wave_lds_sync();  // the queue is free again
  };

  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (uint32_t step = 0; step < nsteps; ++step) {
    const uint32_t cur = step & 1u;
    const uint32_t b = split + (step / nslab) * a.nsplit, s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    // the next step lands in the other buffer under this step's MFMAs (every wave left it at the last barrier)
    if (step + 1 < nsteps) stage(step + 1, cur ^ 1u);
    if (wave_live) {
      const uint4 *s_a = s_rng + cur * bufsz;
      if (s == 0) {
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {  // rows 8 q4 + 4 h + (0..3) of a tile live in registers 4 q4 .. 4 q4 + 3
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
        epilogue(acc0, 0u, b);
        epilogue(acc1, 1u, b);
      }
    }
    // the next step has landed (this wave's loads, stores and atomics too), every wave is done with this buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  if (lane == 0 && nsurv) atomicAdd(a.counters + kSurvivors, (unsigned long long)nsurv);
}

thread_local vi_exact_range_stats g_last_stats{};

vi_status range_exact_in_context(const DeviceIndex &ix, SearchContext &ctx, const ExactRangeIO &io, RangeResult *out) {
  SearchWorkspace &ws = ctx.ws;
  auto &fr = ws.flat_range;
  hipStream_t st = ctx.stream;
  const uint64_t nq = io.nq;
  const uint32_t dim = ix.dim, nc = ix.dq / 4, nblocks = (uint32_t)ix.lists.nblocks;
  const char *te = getenv("VI_EXACT_TIMING");
  const bool timing = te && *te != '0';
  vi_exact_range_stats es{};
  es.nq = nq; es.query_tile = kTileQ;
  const double t0 = now_ms();
  double t_last = t0;
  auto lap = [&](float &ms) -> vi_status {  // (VI_EXACT_TIMING) the phase that ends here
    if (!timing) return VI_OK;
    VI_HIP(hipStreamSynchronize(st));
    const double t = now_ms();
    ms += (float)(t - t_last);
    t_last = t;
    return VI_OK;
  };

  VI_TRY(range_result_begin(ix, nq, out));
  // nothing to find: no query, nothing resident, or a radius no squared distance is within
  if (nq == 0 || ix.nlists == 0 || ix.nvec_resident == 0 || nblocks == 0 || (!io.radii && io.radius2 < 0.0f)) {
    VI_TRY(range_result_place(out, 0, 0, nullptr, st));
    VI_HIP(hipStreamSynchronize(st));
    g_last_stats = es;
    return VI_OK;
  }

  // ---- queries and radii on the device ----
  const float *Qd = io.queries, *radii = io.radii;
  if (!io.on_device) {
    VI_TRY(ws.q.reserve(nq * dim));
    VI_HIP(hipMemcpyAsync(ws.q.p, io.queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, st));
    Qd = ws.q.p;
    if (io.radii) {
      VI_TRY(upload(fr.radii, io.radii, nq, st));
      radii = fr.radii.p;
    }
  }
  VI_TRY(ensure_fetch_layout(ix, st));
  VI_TRY(fr.block_ord.reserve(nblocks));
  VI_TRY(fr.block_cnt.reserve(nblocks));
  VI_TRY(fr.counters.reserve(kCounters));
  hipLaunchKernelGGL(flat_blocks_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, st, ix.list_first_block.p, ix.list_len.p,
                     ix.fetch.prefix.p, (uint32_t)ix.nlists, nblocks, fr.block_ord.p, fr.block_cnt.p);
  VI_HIP(hipGetLastError());

  int cus = 0;
  VI_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix.device));
  const bool resident = dim <= kNarrowDim;
  const int lds = (int)(range_lds_words(resident, nc) * 16u);
  const void *fn = resident ? (const void *)flat_range_sweep_kernel<true> : (const void *)flat_range_sweep_kernel<false>;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return fail(VI_ERR_DEVICE, "cannot reserve %d bytes of LDS for the exact radius search's sweep", lds);
  VI_TRY(reserve_csr_sort_lds());

  for (uint64_t q0 = 0; q0 < nq; q0 += kRangeQueryChunk) {
    const uint64_t m = std::min<uint64_t>(kRangeQueryChunk, nq - q0);
    ++es.chunks;
    // ---- 1. thresholds and images ----
    VI_TRY(fr.thr.reserve(m));
    VI_TRY(fr.rad.reserve(m));
    VI_TRY(fr.cnt.reserve(m));
    VI_TRY(fr.fill.reserve(m));
    VI_TRY(fr.qimg.reserve(m * nc * 16));
    // the frame of lists ranked with bf16 x 3 whatever the engines' switches say: this sweep multiplies nothing else
    SearchBatch b{ix, ctx, io.filter, nullptr, nullptr};
    b.kn = read_engine_knobs();
    b.kn.rank_bf16 = true; b.kn.stats = false;
    b.Qd = Qd + q0 * dim; b.nq = m;
    const SelectCommon c = select_common(b, (const float4 *)ix.lists.blocks.p, ix.centered ? ix.xmax2_c : ix.xmax2, kTileQ);
    RangePrepareArgs pa{c, radii ? radii + q0 : nullptr, io.radius2, (uint32_t)m, nc, fr.thr.p, fr.rad.p, fr.cnt.p, fr.fill.p,
                        (uint4 *)fr.qimg.p, fr.counters.p};
    hipLaunchKernelGGL(flat_range_prepare_kernel, dim3((uint32_t)((m + 3) / 4)), dim3(256), 0, st, pa);
    VI_HIP(hipGetLastError());
    VI_TRY(lap(es.ms_prepare));

    // ---- 2. / 3. the sweep, once more if the pool was too small ----
    uint64_t cap = exact_range_pool_cap(io.pool_cap, m);
    const uint32_t ntiles = (uint32_t)((m + kTileQ - 1) / kTileQ);
    // two workgroups per CU at a time: two rounds of them, so that the tail of the grid is short
    const uint32_t nsplit = exact_block_splits(4u, cus, ntiles, nblocks);
    es.block_splits = nsplit;
    unsigned long long h_count[kCounters] = {};
    for (uint32_t sweep = 1; sweep <= 2; ++sweep) {
      VI_TRY(fr.pool_key.reserve(cap));
      VI_TRY(fr.pool_q.reserve(cap));
      es.pool_cap = std::max<uint64_t>(es.pool_cap, cap);
      RangeSweepArgs sa{(const uint4 *)ix.lists_bf16.p, io.filter ? io.filter->xnorm_img.p : ix.xnorm_img.p, (const uint4 *)fr.qimg.p,
                        (const float4 *)ix.lists.blocks.p, b.Qd, fr.block_ord.p, fr.block_cnt.p, io.filter ? io.filter->allow.p : nullptr,
                        fr.thr.p, fr.rad.p, fr.cnt.p, fr.pool_key.p, fr.pool_q.p, fr.counters.p, cap,
                        (uint32_t)m, dim, ix.dq, nc, nblocks, nsplit, ix.lists_lo_zero ? 0u : 1u};
      if (resident) hipLaunchKernelGGL(flat_range_sweep_kernel<true>, dim3(ntiles, nsplit), dim3(256), lds, st, sa);
      else hipLaunchKernelGGL(flat_range_sweep_kernel<false>, dim3(ntiles, nsplit), dim3(256), lds, st, sa);
      VI_HIP(hipGetLastError());
      VI_HIP(hipMemcpyAsync(h_count, fr.counters.p, sizeof(h_count), hipMemcpyDeviceToHost, st));
      VI_HIP(hipStreamSynchronize(st));
      es.survivors += h_count[kSurvivors];
      es.sweeps = std::max<uint64_t>(es.sweeps, sweep);
      if (h_count[kCursor] <= cap) break;
      if (sweep == 2) return fail(VI_ERR_OTHER, "exact radius search: the second sweep found more hits than the first counted");
      cap = h_count[kCursor];  // every hit was counted: the pool that holds them all
      hipLaunchKernelGGL(flat_range_clear_kernel, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, st, fr.cnt.p, (uint32_t)m, fr.counters.p);
      VI_HIP(hipGetLastError());
    }
    VI_TRY(lap(es.ms_sweep));

    // ---- 4. rows: sized from the counts, filled from the pool, sorted, written ----
    VI_TRY(range_result_place(out, q0, m, fr.cnt.p, st));
    const uint64_t base = out->h_lims[q0], total = out->h_lims[q0 + m] - base;
    if (total != h_count[kCursor]) return fail(VI_ERR_OTHER, "exact radius search: the per-query counts and the pool disagree");
    if (total == 0) continue;
    const uint64_t *lims = out->lims.p + q0;
    VI_TRY(fr.rows.reserve(total));
    hipLaunchKernelGGL(flat_range_place_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, (const uint64_t *)fr.pool_key.p,
                       (const uint32_t *)fr.pool_q.p, total, lims, fr.fill.p, fr.rows.p);
    VI_HIP(hipGetLastError());
    VI_TRY(lap(es.ms_place));
    VI_TRY(sort_csr_rows(lims, out->h_lims.data() + q0, m, fr.rows.p, fr.longq, fr.pad, st));
    VI_TRY(lap(es.ms_sort));
    RangeOutArgs o{fr.rows.p, total, fr.block_ord.p, ix.ext_ids.p, nblocks, out->D.p + base, out->I.p + base, out->tie.p + base,
                   out->slots.p + base};
    hipLaunchKernelGGL(flat_range_output_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, o);
    VI_HIP(hipGetLastError());
    VI_TRY(lap(es.ms_output));
  }
  VI_HIP(hipStreamSynchronize(st));
  es.hits = out->total;
  es.ms_total = timing ? (float)(now_ms() - t0) : 0.0f;
  g_last_stats = es;
  return VI_OK;
}

}  // namespace

vi_exact_range_stats exact_range_last_stats() { return g_last_stats; }

vi_status device_index_range_exact(const DeviceIndex &ix, const ExactRangeIO &io, RangeResult *out) {
  g_last_stats = vi_exact_range_stats{};
  if (ix.stripe_world > 1) return fail(VI_ERR_INVALID_INPUT, "exact radius search needs the whole index on one handle");
  if (ix.order != VI_ORDER_SCALAR) return fail(VI_ERR_INVALID_INPUT, "exact radius search needs an index whose distances are VI_ORDER_SCALAR");
  if (ix.dim < 4 || (ix.dim & 3) || ix.dim > kMaxMfmaDim)
    return fail(VI_ERR_INVALID_INPUT, "exact radius search needs a dimension that is a multiple of 4 and at most %u, not %u", kMaxMfmaDim, ix.dim);
  if (ix.lists.nblocks * 64ull >= (1ull << kPosBits))
    return fail(VI_ERR_INVALID_INPUT, "exact radius search needs an index of fewer than 2^%u slots", kPosBits);
  if (!(ix.xmax2 < 1.0e30f)) return fail(VI_ERR_INVALID_INPUT, "exact radius search needs stored vectors of squared norm below 1e30");
  if (ix.lists.nblocks && (!ix.ext_ids.p || !ix.lists_bf16.p)) return fail(VI_ERR_INVALID_INPUT, "this index keeps no external ids or ranking images");
  if (io.filter && io.filter->owner_serial != ix.serial) return fail(VI_ERR_INVALID_INPUT, "the filter was made for another index");
  const vi_status s = with_search_context(ix, [&](SearchContext &ctx) { return range_exact_in_context(ix, ctx, io, out); });
  if (s != VI_OK) (void)hipGetLastError();  // (a failed allocation is this call's failure, not the next call's)
  return s;
}

}  // namespace vi
