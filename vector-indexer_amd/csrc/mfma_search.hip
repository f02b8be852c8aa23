// mfma_search.hip — the MFMA engine's host side: list scan and coarse quantizer ranked on the matrix cores (bf16 x 3 split
// arithmetic by default, f32 MFMA with VI_FILTER_BF16=0) and the few vectors that can be results re-evaluated in the
// reference's exact order.  This file plans and runs a search; every kernel family has a file and a launch header of its own:
//   coarse step   the centroid table ranked as one list probed by every query (stage_coarse_mfma: rank_block.hpp, select.hpp)
//   grouping      (query, probe) pairs by list, and the rank work items (grouping.hpp)
//   rank          decided first (RankPlan): rank_block.hpp (block-synchronous and wide kernels, where the rank arithmetic and
//                 the pair and group records are described) or rank_stream.hpp (streaming kernel, bf16 or int8)
//   select        records -> exact top-k or radius hits (select.hpp)
// Here remain the batch's query image (split_queries_kernel) and the record offsets of (query, probe).
//
// Host side: the dispatcher (search.hip) hands the pipelines their SearchBatch.
// (filter_kernel and the VI_FILTER variables keep the engine's first name.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "device_index.hpp"
#include "grouping.hpp"
#include "mfma_bf16.hpp"
#include "rank_block.hpp"
#include "rank_stream.hpp"
#include "scan.hpp"
#include "search_internal.hpp"
#include "select.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

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
// the batch's queries as MFMA operands
// ------------------------------------------------------------------------------------------
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

// the batch's queries as MFMA operands: -2 q split into bf16 hi / lo once (a query sits in n_probe work items)
vi_status build_query_image(SearchBatch &b, uint32_t *zero = nullptr, uint64_t zero_words = 0) {
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

// Real-valued lists (not bf16-exact) ranked from their hi planes alone instead of hi + lo (bf16 x 3): a third (queries'
// hi + lo planes: mode 1) or a sixth (queries' hi plane only: mode 2) of the matrix work, paid for with a wider margin
// (select_body: 2 |q| max|v - hi(v)|, plus |query residual| max|v| in mode 2 — the residual norms are measured, not
// bounded by 2^-8 |v|: rounding to nearest leaves about a third of that), which the select turns into more sub-blocks
// re-evaluated exactly; no result depends on a rank value (select.hip).  Chosen per index from its sampled spread;
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
  RankBlockArgs a{};
  a.blocks = kn.rank_bf16 ? (const float4 *)ix.cent_bf16.p : (const float4 *)ix.centroids.blocks.p;
  a.xnorm = kn.rank_bf16 ? ix.cent_xnorm_img.p : ix.cent_xnorm.p; a.dq = dq; a.dim = dim; a.Q = b.Qd;
  a.first_block = ix.c_first.p; a.list_len = ix.c_len.p; a.item_start = ws.c_item.p; a.seg_start = ws.c_seg.p;
  a.pairs = ws.c_pairs.p; a.nlists = 1; a.P = 1; a.segb0 = segb0;
  a.qoff = nullptr; a.rel = nullptr; a.rec_stride = recs;
  a.tile_start = ix.c_first.p;  // one list: its tiles start at 0 (c_first holds a single 0)
  a.gval = (float4 *)ws.gval.p; a.gmeta = ws.gpos.p; a.brec = (float4 *)ws.brec.p;
  a.direct = direct ? 1u : 0u;
  a.qimg = kn.rank_bf16 ? (const uint4 *)ws.qimg.p : nullptr;
  VI_TRY(launch_rank_block(a, dq, ngroups * nseg, kn.rank_bf16 ? (ix.cent_lo_zero && kn.hi_only ? 2 : 1) : 0, kGroupQ, st));
  return launch_coarse_select(b, segb, recs, direct);
}

bool mfma_path_applicable(const DeviceIndex &ix, const EngineKnobs &kn, uint64_t k, uint32_t P) {
  if (!kn.mfma) return false;
  if (ix.order != VI_ORDER_SCALAR || ix.dim > kMaxMfmaDim || (ix.dim & 3) || ix.dim < 4) return false;
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
  if (coarse_mfma) VI_TRY(stage_coarse_mfma(b, histogram_cleared));
  else if (b.probes_in) VI_TRY(adopt_probes(b, true));
  else VI_TRY(stage_coarse(b));
  VI_TRY(prune_staged_probes(b, true));  // (adaptive probing: shorter rows, their histogram, no pair ranks)
  if (!coarse_mfma || b.prune) {  // (the coarse select on the matrix cores leaves the record offsets of its own rows)
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
  if (!nitems) return VI_OK;
  RankWideArgs a{(const uint4 *)ix.lists_bf16.p, b.flt ? b.flt->xnorm_img.p : ix.xnorm_img.p, (const uint4 *)ws.qimg.p, ix.dq / 4,
                 ix.list_first_block.p, ix.list_len.p, ws.item_start.p, ws.seg_start.p, ws.pairs.p, ws.item_list.p, b.P, b.kn.segb0,
                 ws.qoff.p, ws.pair_rel.p, ws.tile_start.p, (float4 *)ws.gval.p, ws.gpos.p, (float4 *)ws.brec.p};
  VI_TRY(start_rank_clock(b));  // (the launch reserves the kernel's LDS first: a host call, nothing on the stream)
  return launch_rank_wide(a, nitems, b.st());
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
    VI_TRY(ws.prof.reserve(kRankStreamProfWords));
    VI_HIP(hipMemsetAsync(ws.prof.p, 0, kRankStreamProfWords * sizeof(uint64_t), b.st()));
    VI_HIP(hipMemsetAsync(ws.prof.p + 16, 0xFF, sizeof(uint64_t), b.st()));
    a.prof = (unsigned long long *)ws.prof.p;
  }
  VI_TRY(start_rank_clock(b));
  // (this kernel ranks hi planes only: plan.math is HiPlanes here)
  VI_TRY(launch_rank_stream(a, ix.dq / 4, nitems, (int)plan.math, plan.qlo, gq, b.st()));
  if (b.kn.stream_prof) VI_TRY(print_rank_stream_profile(ws.prof.p, b.kn.stream_prof_dump, b.st()));  // (synchronises)
  return VI_OK;
}

// D <= 128, everything else: the block-synchronous kernel, in the plan's arithmetic
vi_status rank_block(SearchBatch &b, const RankPlan &plan, uint32_t nitems) {
  SearchWorkspace &ws = b.ws();
  const DeviceIndex &ix = b.ix;
  const bool bf16 = b.kn.rank_bf16;
  VI_TRY(launch_item_desc(ix, ws, b.kn, plan.gq, nitems, b.st()));
  RankBlockArgs a{};
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
  return launch_rank_block(a, ix.dq, nitems, (int)plan.math, plan.gq, b.st());
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
