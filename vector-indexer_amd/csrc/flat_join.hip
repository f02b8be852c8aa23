// flat_join.hip — the exact radius self-join of a built index: every unordered pair of stored records within a distance,
// visited ONCE by a triangular sweep on the matrix cores, and consumed where it is found (the contracts are
// vi_indexer_radius_graph_exact and vi_indexer_cluster_radius_exact in include/vi_amd.h).
//
// The reference's chain gives d(u, v) and d(v, u) the same bits — (a - b)^2 and (b - a)^2 are the same f32 and the
// summation order is the same — so a pair needs one evaluation, and cluster_link (cluster_rules.hpp) is symmetric in its
// two records, so a clustering needs each undirected edge once and never the graph.
//
//   1. rows     the walk over stored records (StoredRowsWalk) gathers a chunk's stored bits into ws.q and their slots
//               into ws.self_slot; flat_join_prepare_kernel, one wave per row, forms the row's rank threshold of the
//               radius in the row's own frame (-inf for a row the filter does not admit) and its bf16 hi / lo image, as
//               the exact radius search does for a query (flat_common.hpp).
//   2. sweep    flat_join_sweep_kernel: grid = row tiles of 128 rows x segments of S consecutive blocks; a wave owns 32
//               rows.  Slot order is list order, so every record of a block below the block of the tile's first row
//               precedes every row of the tile: a workgroup starts at that block, and returns at once when its segment
//               ends below it.  Within a tile the blocking is the exact radius search's (B fragments resident in registers
//               at D <= 128, block images by LDS-DMA into two buffers, bf16 x 3 on v_mfma_f32_32x32x16_bf16, one compare
//               + ballot epilogue per 32 x 32 accumulator tile into a queue of 1024 entries per wave).  A queue entry
//               (row u at slot su, stored slot sv) is kept only if sv > su — or sv == su for the one self entry of a graph
//               that keeps it — and then evaluated in the reference's chain.  Chunks start mid-block and lists end
//               mid-tile: nothing but the test on the two slots decides.
//   3. drain    three instantiations.  DEGREE: one atomicAdd on the degree of either slot.  LINK: cluster_link on the
//               pair (and the degrees, when the call links in one pass).  EMIT: both directed entries — (row of u:
//               key(d, ord v)) and (row of v: key(d, ord u)) — into the exact radius search's pool under one atomicAdd
//               per round of 64 queue entries; the row of v lies in a later chunk, so the pool and the per-row counts
//               span the whole call.  Past the pool's capacity nothing is written and everything is still counted: the
//               pool grows to the count and the whole sweep runs once more.
//   4. finish   graph: lims from the counts, then place / sort / output of flat_rows.hpp over all N rows.  Clustering:
//               the core bits between a DEGREE and a LINK sweep, then cluster_label_kernel (cluster_kernels.hpp).
// Soundness is one-directional: d(u, v) <= r implies that v's rank value in u's frame passes u's threshold (§4s), and the
// pair's single visit is that orientation.  No result depends on a rank value or on the order pairs arrive in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "cluster_kernels.hpp"
#include "device_index.hpp"
#include "flat_common.hpp"
#include "flat_join.hpp"
#include "flat_rows.hpp"
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

enum JoinMode { kDegree = 0, kLink = 1, kEmit = 2 };
enum { kCursor = 0, kSurvivors = 1, kPairs = 2, kJoinCounters = 3 };

// ---- step 1: threshold and image of every row of a chunk; one wave per row ----
struct JoinPrepareArgs {
  SelectCommon c;
  const uint32_t *self_slot;
  const uint64_t *allow;  // the filter's allow bits, or null
  float radius2;          // >= 0
  uint32_t m, nc;
  float *thr;
  uint4 *qimg;
};

__global__ void __launch_bounds__(256) flat_join_prepare_kernel(JoinPrepareArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (q >= a.m) return;
  const QueryFrame f = query_frame<false>(a.c, q, lane, nullptr, nullptr);
  const float thr = radius_rank_threshold(a.c, f, a.radius2);
  const uint32_t s = a.self_slot[q];
  const bool admitted = !a.allow || ((a.allow[s >> 6] >> (s & 63u)) & 1ull);
  if (lane == 0) a.thr[q] = admitted ? thr : -INFINITY;
  split_query_image(a.c, q, a.nc, lane, a.qimg);
}

// before a sweep of the whole graph: the per-row counts and cursors and the call's counters start over
__global__ void flat_join_clear_kernel(uint32_t *cnt, uint32_t *fill, uint32_t n, unsigned long long *counters) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < kJoinCounters) counters[i] = 0ull;
  if (i < n && cnt) { cnt[i] = 0u; fill[i] = 0u; }
}

// ---- step 2: the sweep ----
struct JoinSweepArgs {
  const uint4 *img;     // the lists' bf16 image: [block][chunk][plane][half][64 columns] x 16 B (rank_images.hip)
  const float *xnorm;   // squared norms in image-column order, kBig on pad slots and on slots a filter excludes
  const uint4 *qimg;    // the chunk's rows: [row][plane][chunk][half] x 16 B (flat_common.hpp: split_query_image)
  const float4 *blocks;
  const float *Q;       // the chunk's rows, their stored bits
  const uint32_t *block_ord, *block_cnt;
  const uint64_t *allow;       // one allow word per block, or null
  const float *thr;            // [m] -inf: the row takes no part
  const uint32_t *self_slot;   // [m] ascending: rows are in list order
  uint32_t *degree;            // [nslots] DEGREE, and LINK when it links in one pass; else null
  const uint64_t *core;        // LINK: [nblocks] as cluster_core_kernel left it
  uint32_t *parent, *border;   // LINK: [nslots]
  uint32_t *cnt;               // EMIT: [N] entries of every row of the whole graph
  uint64_t *pool_key;          // EMIT
  uint32_t *pool_q;
  unsigned long long pool_cap;
  unsigned long long *counters;
  float radius2;
  uint32_t row0;        // the list-order ordinal of the chunk's first row
  uint32_t m, dim, dq, nc, nblocks, seg;
  uint32_t lo_planes;   // the lists' lo planes are multiplied (some stored value is not bf16-exact)
  uint32_t keep_self;   // EMIT: the pair (u, u) is one entry of u's row
};

// LDS, in 16-byte words, as the exact radius search lays it out: two K-step buffers, the norms of two blocks, the waves'
// survivor queues — 2 x 32 KB + 0.5 KB + 8 KB = 72.5 KB with the rows RESIDENT in registers at D = 128
__host__ __device__ inline uint32_t join_step_words(bool resident, uint32_t nc) {
  return resident ? nc * 256u : kStreamChunks * (256u + 512u);
}
__host__ __device__ inline uint32_t join_lds_words(bool resident, uint32_t nc) {
  return 2u * join_step_words(resident, nc) + 32u + 4u * kQueueLen * 2u / 16u;
}

template <bool RESIDENT, int MODE>
__global__ void __launch_bounds__(256, 2) flat_join_sweep_kernel(JoinSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_join[];
  const uint32_t q0 = blockIdx.x * kTileRows;
  // ---- the triangular split: this workgroup's blocks, from the block of the tile's first row on ----
  const uint32_t b_lo = max(blockIdx.y * a.seg, a.self_slot[q0] >> 6), b_hi = min((blockIdx.y + 1u) * a.seg, a.nblocks);
  if (b_lo >= b_hi) return;  // (workgroup-uniform, before any barrier)

  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const uint32_t nc = a.nc, kc = RESIDENT ? nc : kStreamChunks, nslab = RESIDENT ? 1u : (nc + kc - 1) / kc;
  const uint32_t bufsz = join_step_words(RESIDENT, nc);
  float *s_norm = (float *)(s_join + 2 * bufsz);  // [2][64]
  uint16_t *s_queue = (uint16_t *)(s_norm + 128) + (uint32_t)wave * kQueueLen;
  const uint32_t nsteps = (b_hi - b_lo) * nslab;
  const uint64_t below = (1ull << lane) - 1ull;

  const uint32_t w0 = q0 + 32u * (uint32_t)wave, qg = w0 + (uint32_t)j;  // this lane's row: both lane halves hold column j
  const float thr = qg < a.m ? a.thr[qg] : -INFINITY;                    // (-inf: no row, or one the filter does not admit)
  const bool lane_live = thr > -INFINITY;
  const bool wave_live = __ballot(lane_live) != 0ull;
  const uint32_t wave_first = w0 < a.m ? a.self_slot[w0] >> 6 : ~0u;    // no block below it holds a slot above a row of the wave

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
  // K step `step` of this workgroup -> buffer `buf`
  auto stage = [&](uint32_t step, uint32_t buf) {
    const uint32_t b = b_lo + step / nslab, s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    float *dst = (float *)(s_join + buf * bufsz);
    const uint4 *src = a.img + ((size_t)b * nc + c0) * 256 + lane;
    for (uint32_t p = wave; p < kcs * 4u; p += 4u) glds16_asm(src + p * 64u, dst + p * 256u);
    if (!RESIDENT) stage_rows(dst + kStreamChunks * 1024u, c0, kcs);
    if (s == 0 && wave == 0) glds4_asm(a.xnorm + (size_t)b * kWave + lane, s_norm + buf * 64u);
  };

  f32x16 acc0, acc1;  // vectors 0..31 and 32..63 of the block's image x this wave's 32 rows
  uint32_t nsurv = 0, npairs = 0;

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

  // queue entry e = (row of the wave | vector << 5) of block b, one per lane -> the directed entries the pair stands for:
  // 0 where it is not this orientation's to visit (sv < su, a pad or filtered slot) or lies outside the radius, 2 for a
  // pair, 1 for the self entry
  auto evaluate = [&](uint32_t b, uint32_t e, bool live, uint32_t nrec, uint64_t allow, uint32_t &q, uint32_t &su, uint32_t &sv, float &d) {
    q = w0 + (e & 31u);
    const uint32_t v = e >> 5;
    sv = b * (uint32_t)kWave + v;
    su = 0u;
    d = INFINITY;
    if (!(live && q < a.m && v < nrec && ((allow >> v) & 1ull))) return 0u;
    su = a.self_slot[q];
    if (!(sv > su || (sv == su && a.keep_self))) return 0u;  // the pair's one visit is from its lower slot
    d = exact_scalar(a.Q + (size_t)q * a.dim, a.blocks + (size_t)b * a.dq * kWave + v, a.dim);
    if (!(d <= a.radius2)) return 0u;
    return sv == su ? 1u : 2u;
  };
  auto core_of = [&](uint32_t s) { return (bool)((a.core[s >> 6] >> (s & 63u)) & 1ull); };
  auto emit = [&](unsigned long long pos, uint32_t row, uint32_t other, float d) {
    if (pos < a.pool_cap) {  // (nothing is written past the pool; everything is counted)
      a.pool_key[pos] = ((uint64_t)__float_as_uint(d) << 32) | other;
      a.pool_q[pos] = row;
    }
    atomicAdd(a.cnt + row, 1u);
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
    // ---- the drain: 64 entries a round; a pair is consumed where it is found ----
    for (uint32_t at = 0; at < n; at += kWave) {
      const uint32_t i = at + (uint32_t)lane;
      uint32_t q, su, sv;
      float d;
      const uint32_t ne = evaluate(b, i < n ? s_queue[i] : 0u, i < n, nrec, allow, q, su, sv, d);
      const uint64_t any = __ballot(ne != 0u), pairs = __ballot(ne == 2u);
      if (!any) continue;
      npairs += (uint32_t)__popcll(pairs);
      if (MODE == kEmit) {  // the round's entries take one range of the pool
        unsigned long long base = 0ull;
        if (lane == 0) base = atomicAdd(a.counters + kCursor, (unsigned long long)(__popcll(any) + __popcll(pairs)));
        const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
        const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(base >> 32));
        if (ne) {
          const unsigned long long pos = (((unsigned long long)bhi << 32) | blo) + (uint32_t)(__popcll(any & below) + __popcll(pairs & below));
          const uint32_t ord_u = a.row0 + q, ord_v = ord0 + (sv & 63u);
          emit(pos, ord_u, ord_v, d);
          if (ne == 2u) emit(pos + 1ull, ord_v, ord_u, d);
        }
      } else if (ne == 2u) {
        if (a.degree) { atomicAdd(a.degree + su, 1u); atomicAdd(a.degree + sv, 1u); }
        if (MODE == kLink) cluster_link<AgentAccess>(a.parent, a.border, su, core_of(su), sv, core_of(sv));
      }
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
      const uint4 *s_a = s_join + cur * bufsz;
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
  if (lane == 0 && npairs) atomicAdd(a.counters + kPairs, (unsigned long long)npairs);
}

template <int MODE>
vi_status launch_join_sweep(bool resident, dim3 grid, int lds, hipStream_t st, const JoinSweepArgs &sa) {
  const void *fn = resident ? (const void *)flat_join_sweep_kernel<true, MODE> : (const void *)flat_join_sweep_kernel<false, MODE>;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return fail(VI_ERR_DEVICE, "cannot reserve %d bytes of LDS for the exact radius join's sweep", lds);
  if (resident) hipLaunchKernelGGL((flat_join_sweep_kernel<true, MODE>), grid, dim3(256), lds, st, sa);
  else hipLaunchKernelGGL((flat_join_sweep_kernel<false, MODE>), grid, dim3(256), lds, st, sa);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

thread_local vi_exact_join_stats g_last_stats{};

// One call: the sweeps over all N rows of either entry, their phase clock and their counters.
struct Join {
  const DeviceIndex &ix;
  SearchContext &ctx;
  const ExactJoinIO &io;
  vi_exact_join_stats es{};
  StoredRowsWalk walk{64};
  bool timing = false;
  double t_last = 0.0;
  int cus = 1;

  Join(const DeviceIndex &ix_, SearchContext &ctx_, const ExactJoinIO &io_) : ix(ix_), ctx(ctx_), io(io_) {
    const char *te = getenv("VI_EXACT_TIMING");
    timing = te && *te != '0';
    es.rows = ix.nvec_resident; es.chunk_rows = walk.chunk_rows;
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
  // what every sweep needs: the blocks' ordinals and counts, the counters
  vi_status begin() {
    auto &fr = ctx.ws.flat_range;
    hipStream_t st = ctx.stream;
    const uint32_t nblocks = (uint32_t)ix.lists.nblocks;
    VI_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix.device));
    VI_TRY(ensure_fetch_layout(ix, st));
    VI_HIP(hipSetDevice(ix.device));
    VI_TRY(fr.block_ord.reserve(nblocks));
    VI_TRY(fr.block_cnt.reserve(nblocks));
    VI_TRY(fr.counters.reserve(kJoinCounters));
    hipLaunchKernelGGL(flat_blocks_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, st, ix.list_first_block.p, ix.list_len.p,
                       ix.fetch.prefix.p, (uint32_t)ix.nlists, nblocks, fr.block_ord.p, fr.block_cnt.p);
    VI_HIP(hipGetLastError());
    return VI_OK;
  }
  // blocks per segment for the chunk whose first row is q0: the rectangle of (row tiles) x (blocks from about the chunk's
  // first on) cut into some sixteen workgroups per CU, of which a bare triangle — the last chunks — keeps half: four full
  // rounds at two workgroups per CU.  Short segments read a tile's rows again more often, long ones leave CUs idle.
  uint32_t segment_blocks(uint64_t q0, uint32_t ntiles) const {
    const uint64_t nblocks = ix.lists.nblocks, ahead = nblocks - std::min<uint64_t>(nblocks - 1, q0 * nblocks / std::max<uint64_t>(ix.nvec_resident, 1));
    const uint64_t s = (uint64_t)ntiles * ahead / (16ull * (uint64_t)std::max(cus, 1));
    return (uint32_t)std::max<uint64_t>(std::min<uint64_t>(std::max<uint64_t>(s, kSegMin), kSegMax), (nblocks + kMaxGridY - 1) / kMaxGridY);
  }
  // one sweep of the whole graph; `sa` carries the drain's arrays, the chunk's are filled in here
  template <int MODE>
  vi_status sweep(JoinSweepArgs sa) {
    SearchWorkspace &ws = ctx.ws;
    auto &fr = ws.flat_range;
    hipStream_t st = ctx.stream;
    const uint32_t dim = ix.dim, nc = ix.dq / 4, nblocks = (uint32_t)ix.lists.nblocks;
    const bool resident = dim <= kNarrowDim;
    const int lds = (int)(join_lds_words(resident, nc) * 16u);
    const uint64_t *allow = io.filter ? io.filter->allow.p : nullptr;
    hipLaunchKernelGGL(flat_join_clear_kernel, dim3(1), dim3(64), 0, st, nullptr, nullptr, 0u, fr.counters.p);
    VI_HIP(hipGetLastError());
    StoredRows all;  // every resident record, in list order
    all.nq = ix.nvec_resident;
    const auto body = [&](const RowChunk &c) -> vi_status {
      VI_TRY(lap(es.ms_resolve));
      const uint64_t m = c.m;
      VI_TRY(fr.thr.reserve(m));
      VI_TRY(fr.qimg.reserve(m * nc * 16));
      // the frame of lists ranked with bf16 x 3 whatever the engines' switches say: this sweep multiplies nothing else
      SearchBatch b{ix, ctx, io.filter, nullptr, nullptr};
      b.kn = read_engine_knobs();
      b.kn.rank_bf16 = true; b.kn.stats = false;
      b.Qd = ws.q.p; b.nq = m;
      const SelectCommon sc = select_common(b, (const float4 *)ix.lists.blocks.p, ix.centered ? ix.xmax2_c : ix.xmax2, kTileRows);
      JoinPrepareArgs pa{sc, ws.self_slot.p, allow, io.radius2, (uint32_t)m, nc, fr.thr.p, (uint4 *)fr.qimg.p};
      hipLaunchKernelGGL(flat_join_prepare_kernel, dim3((uint32_t)((m + 3) / 4)), dim3(256), 0, st, pa);
      VI_HIP(hipGetLastError());
      VI_TRY(lap(es.ms_prepare));
      const uint32_t ntiles = (uint32_t)((m + kTileRows - 1) / kTileRows), seg = segment_blocks(c.q0, ntiles);
      const uint32_t nseg = (nblocks + seg - 1) / seg;
      es.tiles = std::max<uint64_t>(es.tiles, ntiles);
      es.segments = std::max<uint64_t>(es.segments, nseg);
      JoinSweepArgs a = sa;
      a.img = (const uint4 *)ix.lists_bf16.p; a.xnorm = io.filter ? io.filter->xnorm_img.p : ix.xnorm_img.p;
      a.qimg = (const uint4 *)fr.qimg.p; a.blocks = (const float4 *)ix.lists.blocks.p; a.Q = ws.q.p;
      a.block_ord = fr.block_ord.p; a.block_cnt = fr.block_cnt.p; a.allow = allow; a.thr = fr.thr.p; a.self_slot = ws.self_slot.p;
      a.counters = fr.counters.p; a.radius2 = io.radius2; a.row0 = (uint32_t)c.q0; a.m = (uint32_t)m; a.dim = dim; a.dq = ix.dq;
      a.nc = nc; a.nblocks = nblocks; a.seg = seg; a.lo_planes = ix.lists_lo_zero ? 0u : 1u;
      VI_TRY(launch_join_sweep<MODE>(resident, dim3(ntiles, nseg), lds, st, a));
      VI_TRY(lap(es.ms_sweep));
      return VI_OK;
    };
    const auto landed = [&](const RowChunk &) -> vi_status { if (timing) t_last = now_ms(); return VI_OK; };
    VI_TRY(walk.run(ix, ctx, all, body, landed));
    unsigned long long h_count[kJoinCounters] = {};
    VI_HIP(hipMemcpyAsync(h_count, fr.counters.p, sizeof(h_count), hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
    ++es.sweeps;
    es.survivors += h_count[kSurvivors];
    es.pairs = h_count[kPairs];
    cursor = h_count[kCursor];
    return VI_OK;
  }
  unsigned long long cursor = 0;  // EMIT: directed entries the last sweep counted
};

vi_status cluster_exact_in_context(const DeviceIndex &ix, SearchContext &ctx, const ExactJoinIO &io) {
  hipStream_t st = ctx.stream;
  const uint64_t N = ix.nvec_resident, nblocks = ix.lists.nblocks, nslots = nblocks * 64;
  const bool link = io.labels || io.n_clusters;
  const bool two = link && io.min_pts >= 2;
  Join jn(ix, ctx, io);
  if (N == 0 || nblocks == 0) {  // nothing is resident: no label to write
    if (io.n_clusters) *io.n_clusters = 0;
    g_last_stats = jn.es;
    return VI_OK;
  }
  VI_TRY(jn.begin());
  // ---- the call's scratch, by slot; freed on return ----
  DevBuf<uint32_t> parent, border, degree;
  DevBuf<uint64_t> core;
  DevBuf<unsigned long long> count;
  DevBuf<int64_t> labels_stage;   // a host caller's outputs are made here and copied once everything has succeeded
  DevBuf<uint32_t> degree_stage;
  VI_TRY(parent.reserve(nslots));
  VI_TRY(border.reserve(nslots));
  VI_TRY(degree.reserve(nslots));
  VI_TRY(core.reserve(nblocks));
  VI_TRY(count.reserve(kCounters));
  int64_t *labels = io.labels;
  uint32_t *degree_out = io.degree;
  if (!io.on_device) {
    if (io.labels) { VI_TRY(labels_stage.reserve(N)); labels = labels_stage.p; }
    if (io.degree) { VI_TRY(degree_stage.reserve(N)); degree_out = degree_stage.p; }
  }
  const ResidentLists L{ix.list_first_block.p, ix.list_len.p, (uint32_t)ix.nlists};
  const uint64_t *allow = io.filter ? io.filter->allow.p : nullptr;
  hipLaunchKernelGGL(cluster_init_kernel, dim3(ceil_div_u32(nslots, 256)), dim3(256), 0, st, parent.p, border.p, degree.p, (uint32_t)nslots);
  VI_HIP(hipGetLastError());
  VI_HIP(hipMemsetAsync(core.p, 0, nblocks * sizeof(uint64_t), st));
  VI_HIP(hipMemsetAsync(count.p, 0, kCounters * sizeof(unsigned long long), st));

  const bool edges = io.radius2 >= 0.0f;  // (a negative radius: no pair, no sweep)
  JoinSweepArgs sa{};
  sa.core = core.p; sa.parent = parent.p; sa.border = border.p;
  if (edges && (!link || two)) {  // the degrees: all the call wants, or what the core bits are made from
    sa.degree = degree.p;
    VI_TRY(jn.sweep<kDegree>(sa));
  }
  if (link) {
    hipLaunchKernelGGL(cluster_core_kernel, slot_walk_grid((uint32_t)ix.nlists), dim3(256), 0, st, L, allow, degree.p, io.min_pts, core.p);
    VI_HIP(hipGetLastError());
    sa.degree = two ? nullptr : degree.p;  // a call that links in one pass counts the degrees as it links
    if (edges) VI_TRY(jn.sweep<kLink>(sa));
  }
  // ---- labels, degrees and counts, in a launch of its own: every hook of the link sweep is visible to it ----
  LabelArgs ga{L, ix.fetch.prefix.p, core.p, parent.p, border.p, degree.p, labels, degree_out, count.p, link ? 1u : 0u};
  hipLaunchKernelGGL(cluster_label_kernel, slot_walk_grid((uint32_t)ix.nlists), dim3(256), 0, st, ga);
  VI_HIP(hipGetLastError());
  unsigned long long h_count[kCounters] = {};
  VI_HIP(hipMemcpyAsync(h_count, count.p, sizeof(h_count), hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  if (!io.on_device) {  // everything has succeeded: the caller's arrays are written now
    if (io.labels) VI_HIP(hipMemcpyAsync(io.labels, labels, N * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (io.degree) VI_HIP(hipMemcpyAsync(io.degree, degree_out, N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
  }
  VI_TRY(jn.lap(jn.es.ms_finish));
  jn.es.hits = h_count[kCountHits];
  if (io.n_clusters) *io.n_clusters = h_count[kCountRoots];
  g_last_stats = jn.es;
  return VI_OK;
}

vi_status graph_exact_in_context(const DeviceIndex &ix, SearchContext &ctx, const ExactJoinIO &io, RangeResult *out) {
  auto &fr = ctx.ws.flat_range;
  hipStream_t st = ctx.stream;
  const uint64_t N = ix.nvec_resident;
  const uint32_t nblocks = (uint32_t)ix.lists.nblocks;
  Join jn(ix, ctx, io);
  VI_TRY(range_result_begin(ix, N, out));
  if (N == 0 || nblocks == 0 || io.radius2 < 0.0f) {  // nothing to find: N empty rows
    VI_TRY(range_result_place(out, 0, 0, nullptr, st));
    VI_HIP(hipStreamSynchronize(st));
    g_last_stats = jn.es;
    return VI_OK;
  }
  VI_TRY(jn.begin());
  VI_TRY(reserve_csr_sort_lds());
  VI_TRY(fr.cnt.reserve(N));
  VI_TRY(fr.fill.reserve(N));
  // ---- the sweep, once more if the pool was too small ----
  uint64_t cap = exact_range_pool_cap(io.pool_cap, N);
  for (uint32_t pass = 1; pass <= 2; ++pass) {
    VI_TRY(fr.pool_key.reserve(cap));
    VI_TRY(fr.pool_q.reserve(cap));
    jn.es.pool_cap = cap;
    hipLaunchKernelGGL(flat_join_clear_kernel, dim3(ceil_div_u32(N, 256)), dim3(256), 0, st, fr.cnt.p, fr.fill.p, (uint32_t)N, fr.counters.p);
    VI_HIP(hipGetLastError());
    JoinSweepArgs sa{};
    sa.cnt = fr.cnt.p; sa.pool_key = fr.pool_key.p; sa.pool_q = fr.pool_q.p; sa.pool_cap = cap; sa.keep_self = io.exclude_self ? 0u : 1u;
    VI_TRY(jn.sweep<kEmit>(sa));
    if (jn.cursor <= cap) break;
    if (pass == 2) return fail(VI_ERR_OTHER, "exact radius graph: the second sweep found more entries than the first counted");
    cap = jn.cursor;  // every entry was counted: the pool that holds them all
  }
  // ---- rows: sized from the counts, filled from the pool, sorted, written ----
  VI_TRY(range_result_place(out, 0, N, fr.cnt.p, st));
  const uint64_t total = out->h_lims[N];
  if (total != jn.cursor) return fail(VI_ERR_OTHER, "exact radius graph: the per-row counts and the pool disagree");
  if (total) {
    VI_TRY(fr.rows.reserve(total));
    hipLaunchKernelGGL(flat_range_place_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, (const uint64_t *)fr.pool_key.p,
                       (const uint32_t *)fr.pool_q.p, total, (const uint64_t *)out->lims.p, fr.fill.p, fr.rows.p);
    VI_HIP(hipGetLastError());
    VI_TRY(sort_csr_rows(out->lims.p, out->h_lims.data(), N, fr.rows.p, fr.longq, fr.pad, st));
    RangeOutArgs o{fr.rows.p, total, fr.block_ord.p, ix.ext_ids.p, nblocks, out->D.p, out->I.p, out->tie.p, out->slots.p};
    hipLaunchKernelGGL(flat_range_output_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, st, o);
    VI_HIP(hipGetLastError());
  }
  VI_HIP(hipStreamSynchronize(st));
  VI_TRY(jn.lap(jn.es.ms_finish));
  jn.es.hits = total;
  g_last_stats = jn.es;
  return VI_OK;
}

// the limits of the exact calls and of the calls by stored record: VI_ERR_INVALID_INPUT before any device work
vi_status join_limits(const DeviceIndex &ix, const ExactJoinIO &io) {
  if (ix.stripe_world > 1) return fail(VI_ERR_INVALID_INPUT, "the exact radius join needs the whole index on one handle");
  if (ix.order != VI_ORDER_SCALAR) return fail(VI_ERR_INVALID_INPUT, "the exact radius join needs an index whose distances are VI_ORDER_SCALAR");
  if (ix.dim < 4 || (ix.dim & 3) || ix.dim > kMaxMfmaDim)
    return fail(VI_ERR_INVALID_INPUT, "the exact radius join needs a dimension that is a multiple of 4 and at most %u, not %u", kMaxMfmaDim, ix.dim);
  if (ix.lists.nblocks * 64ull >= (1ull << kPosBits))
    return fail(VI_ERR_INVALID_INPUT, "the exact radius join needs an index of fewer than 2^%u slots", kPosBits);
  if (!(ix.xmax2 < 1.0e30f)) return fail(VI_ERR_INVALID_INPUT, "the exact radius join needs stored vectors of squared norm below 1e30");
  if (ix.lists.nblocks && !ix.lists_bf16.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no ranking images");
  if (io.filter && io.filter->owner_serial != ix.serial) return fail(VI_ERR_INVALID_INPUT, "the filter was made for another index");
  return VI_OK;
}

}  // namespace

vi_exact_join_stats exact_join_last_stats() { return g_last_stats; }

vi_status device_index_cluster_exact(const DeviceIndex &ix, const ExactJoinIO &io) {
  g_last_stats = vi_exact_join_stats{};
  VI_TRY(join_limits(ix, io));
  const vi_status s = stored_record_call(ix, g_last_stats, [&](SearchContext &ctx) { return cluster_exact_in_context(ix, ctx, io); });
  if (s != VI_OK) g_last_stats = vi_exact_join_stats{};
  return s;
}

vi_status device_index_graph_exact(const DeviceIndex &ix, const ExactJoinIO &io, RangeResult *out) {
  g_last_stats = vi_exact_join_stats{};
  VI_TRY(join_limits(ix, io));
  const vi_status s = stored_record_call(ix, g_last_stats, [&](SearchContext &ctx) { return graph_exact_in_context(ix, ctx, io, out); });
  if (s != VI_OK) g_last_stats = vi_exact_join_stats{};
  return s;
}

}  // namespace vi
