// range_select.hip — the radius form of the MFMA engine's list select: from the records the rank kernels leave to every
// probed vector whose reference distance is at or below radius2, in the reference's stable order.
//
// The top-k select (select.hip) spends its first stages finding a threshold from the K-th smallest rank value.  Here the
// threshold is known before anything is read: a vector with reference distance d <= radius2 has, in the frame its records
// live in (||q||^2 = qn there), a rank value
//     m <= thr = (radius2 - qn) + w + 2E + 3 gamma (radius2 + E),      w = (D/64 + 9) u' (|radius2| + qn)
// = rank_threshold((radius2 - qn) + w): E, gamma and the formula (*) are the top-k select's, formed once in
// select_device.hpp (query_frame, rank_threshold); w covers the f32 rounding of the subtraction and of qn's own sum.  So
// one pass over the records is enough: the groups whose smallest minimum is at or below thr, their pair records, and of
// those every sub-block whose minimum is at or below thr — re-evaluated as a whole in the reference's exact order, four
// sub-blocks per wave instruction: the top-k select's stage 2, on the same record walk (GroupRecords,
// scan_pair_records, push_sub / drain_pick).  What comes out depends on exact distances only.
//
// Sizing, with nothing evaluated twice: the same pass WITHOUT the evaluations (range_select_kernel<false>) counts the
// sub-blocks per query; 16 x that bounds the query's hits and sizes its row of the key scratch.  The pass with the
// evaluations writes (distance, (candidate-order rank << 26) | position) keys into the row and leaves the true count;
// the rows are sorted by key — the reference's stable order — and range_output_kernel turns them into D / I / tie / slot
// at lims[q].  Queries go through this in chunks whose rows fit the key budget.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "select.hpp"
#include "select_device.hpp"

namespace vi {

namespace {

constexpr uint64_t kMaxRangeKeys = 1ull << 27;  // keys in flight per chunk of queries (1 GiB): the generic engine's budget
constexpr uint32_t kMinRowLog = 11;             // rows of at least 2048 keys (sort_rows_u64)

struct RangeArgs {
  SelectCommon c;
  uint32_t q0, m, P;  // queries [q0, q0 + m) of the batch
  float radius2;
  ListProbes lp;
  uint32_t *bound;    // EMIT false: [nq] 16 x (sub-blocks at or below the threshold)
  uint64_t *keys;     // EMIT true: row (q - q0) of 2^logL keys, preset to ~0
  uint32_t logL;
  uint32_t *counts;   // EMIT true: [nq] hits
  uint32_t *overflow; // EMIT true: raised if a row would not hold its hits (the two passes disagree: never)
};

// exact reference distance of one (query, stored vector) pair per live lane, in the form exact_offer (select.hip) takes
// for the same index and query: 0 the f32 blocks, 1 the natural-order hi plane of bf16-exact lists, 2 one byte per
// dimension, 3 bytes against an integer-valued query.  A real function: its four loops inlined at every place the queue
// drains would be most of the kernel's code.
__device__ __attribute__((noinline)) float exact_dist_fn(uint32_t form, const float *qrow, const uint32_t *qbytes, uint32_t qn_int,
                                                         const uint4 *x, uint32_t dim, bool live) {
  float d = INFINITY;
  if (live) {
    if (form == 3u) d = exact_pair_u8_int(qbytes, qn_int, x, dim);
    else if (form == 2u) d = exact_pair_u8(qrow, x, dim);
    else if (form == 1u) d = exact_pair_bf16(qrow, x, dim);
    else d = exact_pair<kWave>(qrow, (const float4 *)x, dim);
  }
  return d;
}

// One wave per query.  EMIT false: count; EMIT true: evaluate and write keys.  FILT: only vectors whose allow bit is set
// are evaluated (the rank kernels saw the others with the pad norm, so they sit in no record minimum).
template <bool EMIT, bool FILT>
__global__ void __launch_bounds__(256, 4) range_select_kernel(RangeArgs a) {
  __shared__ uint32_t s_pick[4][kPickCap], s_lcache[4][kCacheG];
  __shared__ float4 s_tcache[4][kCacheG];
  __shared__ __attribute__((aligned(16))) uint32_t s_qbytes[4][64];  // the 4 queries as bytes (8-bit lists, D <= 256)
  extern __shared__ __attribute__((aligned(16))) float s_qrows[];    // the 4 query rows of the workgroup: 4 x dim floats
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if (blockIdx.x * 4 + wave >= a.m) return;
  const uint32_t q = a.q0 + blockIdx.x * 4 + wave;
  const SelectCommon &c = a.c;
  uint32_t *pick = s_pick[wave], *qbytes = s_qbytes[wave];
  float *qlds = s_qrows + (size_t)wave * c.dim;
  const ProbeRegs pr = load_probe_regs(a.lp, c.gq, q, a.P, lane);
  const GroupRecords gr{c, a.lp.qoff[q], a.lp.qtot[q], s_tcache[wave], s_lcache[wave]};
  const uint64_t below = (1ull << lane) - 1ull;
  const QueryFrame f = query_frame<EMIT>(c, q, lane, qlds, qbytes);
  // ---- the threshold: known before any record is read.  A radius beyond the point where the bound means anything (or,
  //      in rank_threshold, a distrusted query): no bound, everything probed is re-evaluated ----
  float thr = INFINITY;
  if (a.radius2 < 1.0e37f) {
    const float w = ((float)(c.dim >> 6) + 9.0f) * 6.1e-8f * (fabsf(a.radius2) + f.qn);  // 6.1e-8 > u' = 1.01 * 2^-24
    thr = rank_threshold(c, f, (a.radius2 - f.qn) + w);
  }
  const uint32_t form = c.u8_nat ? (f.q_bytes ? 3u : 2u) : (c.hi_nat ? 1u : 0u);
  const uint4 *xbase = c.u8_nat ? c.u8_nat : (c.hi_nat ? c.hi_nat : (const uint4 *)c.blocks);
  const uint32_t xmult = c.u8_nat ? c.dq / 4u : (c.hi_nat ? c.dq / 2u : c.dq);  // 16-byte pieces per vector
  uint64_t *row = EMIT ? a.keys + ((size_t)(q - a.q0) << a.logL) : nullptr;
  const uint32_t cap = EMIT ? 1u << a.logL : 0u;
  uint32_t npick = 0, n_exact = 0, n_scanned = 0, n_sub = 0, cursor = 0;
  // one (probe rank, position) per lane: exact distance, and a key at the query's cursor if it is within the radius
  auto exact_emit = [&](bool live, uint32_t r, uint32_t pos) {
    const uint32_t fb = (uint32_t)__shfl((int)pr.fb, (int)r);
    const uint32_t g = (uint32_t)__shfl((int)pr.g, (int)r);
    const uint32_t len = (uint32_t)__shfl((int)pr.len, (int)r);
    live = live && pos < len;
    const uint32_t p = live ? pos : 0u;
    if constexpr (FILT) live = live && ((c.allow[fb + p / kWave] >> (p % kWave)) & 1ull) != 0ull;
    n_exact += (uint32_t)__popcll(__ballot(live));
    const float d = exact_dist_fn(form, qlds, qbytes, f.qn_int, xbase + ((size_t)(fb + p / kWave) * xmult) * kWave + (p % kWave), c.dim, live);
    const bool hit = live && d <= a.radius2;
    const uint64_t m = __ballot(hit);
    if (hit) {
      const uint32_t at = cursor + (uint32_t)__popcll(m & below);
      if (at < cap) row[at] = pack_key(d, (g << kPosBits) | pos);
    }
    cursor += (uint32_t)__popcll(m);
  };
  auto drain = [&]() { drain_pick(c, pick, npick, lane, exact_emit); };
  gr.fill(lane);
  // ---- every sub-block whose minimum is at or below thr sits in a group whose smallest minimum is: those groups' pair
  //      records, and of those every sub-block at or below thr — queued for its exact distances, or counted ----
  for (uint32_t gb = 0; gb < gr.G; gb += kWave) {
    const uint32_t gidx = gb + lane;
    const bool live = gidx < gr.G;
    uint32_t r, seg, hh;
    gr.group_place(gidx, live, r, seg, hh);
    scan_pair_records(c, pr, lane, live && !(gr.group_values(gidx, live).x > thr), r, seg, hh, n_scanned,
                      [&](bool ok, float v, uint32_t, uint32_t rr, uint32_t sub, uint32_t h2) {
                        const bool want = ok && !(v > thr);  // (!(v > thr): a NaN minimum is expanded, never skipped)
                        if constexpr (EMIT) push_sub(pick, npick, n_sub, lane, want, rr, sub, h2, drain);
                        else n_sub += (uint32_t)__popcll(__ballot(want));
                      });
  }
  if constexpr (EMIT) {
    drain();
    if (lane == 0) {
      a.counts[q] = min(cursor, cap);
      if (cursor > cap) atomicOr(a.overflow, 1u);
    }
    if (c.dbg && lane == 0 && (q & c.dbg_mask) == 0u) {
      atomicAdd(&c.dbg[kStatSelExact], (unsigned long long)n_exact);
      atomicAdd(&c.dbg[kStatSelScanned], (unsigned long long)n_scanned);
      atomicAdd(&c.dbg[kStatSelSubBlocks], (unsigned long long)n_sub);
    }
  } else {
    if (lane == 0) a.bound[q] = 16u * n_sub;
  }
}

struct RangeOutArgs {
  const uint64_t *keys;  // sorted rows of 2^logL keys, row (q - q0)
  uint32_t logL, q0, m, P;
  const uint32_t *counts, *probes, *gorder, *first_block;
  const uint64_t *lims, *ext_ids;
  float *D;
  int64_t *I;
  uint64_t *tie, *slots;
};

// one wave per query: the first counts[q] keys of its sorted row to D / I / tie / slot at lims[q]; the candidate-order
// rank g of a key goes back to its probe as in select_kernel's epilogue
__global__ void __launch_bounds__(256) range_output_kernel(RangeOutArgs a) {
  __shared__ uint32_t s_fb[4][kWave];
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if (blockIdx.x * 4 + wave >= a.m) return;
  const uint32_t q = a.q0 + blockIdx.x * 4 + wave;
  if (lane < a.P) {  // first block of the probe with candidate-order rank g, at s_fb[g] (the ranks of a query's probes are distinct)
    const uint32_t l = a.probes[(size_t)q * a.P + lane], g = a.gorder[(size_t)q * a.P + lane];
    if (l != kNoPos && g < kWave) s_fb[wave][g] = a.first_block[l];
  }
  wave_lds_sync();
  const uint64_t *row = a.keys + ((size_t)(q - a.q0) << a.logL);
  const uint64_t at = a.lims[q];
  const uint32_t n = a.counts[q];
  for (uint32_t i = lane; i < n; i += kWave) {
    const uint64_t key = row[i];
    const uint32_t t = (uint32_t)key, g = t >> kPosBits, pos = t & kPosMask;
    const uint64_t gslot = (uint64_t)s_fb[wave][g & 63u] * kWave + pos;
    a.D[at + i] = sortable_f32((uint32_t)(key >> 32));
    a.I[at + i] = (int64_t)a.ext_ids[gslot];
    a.tie[at + i] = ((uint64_t)g << 32) | pos;
    a.slots[at + i] = gslot;
  }
}

}  // namespace

vi_status launch_range_select(SearchBatch &b, float radius2, const SelectFrame &f, RangeResult *res) {
  const DeviceIndex &ix = b.ix;
  const EngineKnobs &kn = b.kn;
  SearchWorkspace &ws = b.ws();
  const uint64_t nq = b.nq;
  hipStream_t st = b.st();
  VI_TRY(ws.range_bound.reserve(nq + 1));  // (the last word: the overflow flag)
  VI_TRY(ws.counts.reserve(nq));
  RangeArgs a{list_select_common(b, f), 0u, (uint32_t)nq, b.P, radius2, list_probes(b), ws.range_bound.p, nullptr, 0u, ws.counts.p,
              ws.range_bound.p + nq};
  if (b.flt) a.c.allow = b.flt->allow.p;
  unsigned long long *dbg = a.c.dbg;
  const size_t qsm = 4ull * ix.dim * sizeof(float);
  // (VI_FILTER_STATS=3 / 4) the steps' own clocks, printed like the select's: events of this call's, each read after a
  // synchronisation the step makes anyway
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  struct EventGuard { hipEvent_t *e; ~EventGuard() { for (int i = 0; i < 5; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } guard{ev};
  float ms_step[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // bound pass, evaluation, sort, placing + output
  auto mark = [&](int i) -> vi_status {
    if (!kn.stats_print) return VI_OK;
    if (!ev[i]) VI_HIP(hipEventCreate(&ev[i]));
    VI_HIP(hipEventRecord(ev[i], st));
    return VI_OK;
  };
  auto lap = [&](int step, int from, int to) {
    float ms = 0.0f;
    if (kn.stats_print && hipEventElapsedTime(&ms, ev[from], ev[to]) == hipSuccess) ms_step[step] += ms;
  };
  // ---- 1. the bound pass: 16 x (sub-blocks at or below the threshold) per query ----
  a.c.dbg = nullptr;
  VI_HIP(hipMemsetAsync(ws.range_bound.p + nq, 0, sizeof(uint32_t), st));
  VI_TRY(mark(0));
  hipLaunchKernelGGL((range_select_kernel<false, false>), dim3((uint32_t)((nq + 3) / 4)), dim3(256), qsm, st, a);
  VI_HIP(hipGetLastError());
  VI_TRY(mark(1));
  std::vector<uint32_t> h_bound(nq);
  VI_HIP(hipMemcpyAsync(h_bound.data(), ws.range_bound.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  lap(0, 0, 1);
  a.c.dbg = dbg;
  // ---- 2. per chunk of queries whose rows fit the key budget: evaluate, sort, place, write ----
  uint64_t q0 = 0;
  while (q0 < nq) {
    uint32_t logL = kMinRowLog;
    while ((1ull << logL) < h_bound[q0]) ++logL;
    if ((1ull << logL) > kMaxRangeKeys) return fail(VI_ERR_INVALID_INPUT, "a query's radius admits more candidates than the key scratch holds");
    uint64_t m = 1;
    while (q0 + m < nq) {  // grow the chunk while rows x row-length stays within the key budget
      uint32_t lg = logL;
      while ((1ull << lg) < h_bound[q0 + m]) ++lg;
      if ((m + 1) << lg > kMaxRangeKeys) break;
      logL = lg;
      ++m;
    }
    const uint64_t L = 1ull << logL;
    VI_TRY(ws.sort_keys.reserve(m * L));
    VI_TRY(mark(0));
    VI_HIP(hipMemsetAsync(ws.sort_keys.p, 0xFF, m * L * sizeof(uint64_t), st));
    a.q0 = (uint32_t)q0; a.m = (uint32_t)m; a.keys = ws.sort_keys.p; a.logL = logL;
    const dim3 grid((uint32_t)((m + 3) / 4));
    if (b.flt) hipLaunchKernelGGL((range_select_kernel<true, true>), grid, dim3(256), qsm, st, a);
    else hipLaunchKernelGGL((range_select_kernel<true, false>), grid, dim3(256), qsm, st, a);
    VI_HIP(hipGetLastError());
    VI_TRY(mark(1));
    VI_TRY(sort_rows_u64(ws.sort_keys.p, m, logL, st));
    VI_TRY(mark(2));
    VI_TRY(range_result_place(res, q0, m, ws.counts.p + q0, st));
    RangeOutArgs o{ws.sort_keys.p, logL, (uint32_t)q0, (uint32_t)m, b.P, ws.counts.p, ws.probes.p, ws.gorder.p, ix.list_first_block.p,
                   res->lims.p, ix.ext_ids.p, res->D.p, res->I.p, res->tie.p, res->slots.p};
    hipLaunchKernelGGL(range_output_kernel, grid, dim3(256), 0, st, o);
    VI_HIP(hipGetLastError());
    VI_TRY(mark(3));
    if (kn.stats_print) {
      VI_HIP(hipStreamSynchronize(st));
      lap(1, 0, 1); lap(2, 1, 2); lap(3, 2, 3);
    }
    q0 += m;
  }
  uint32_t overflow = 0;
  VI_HIP(hipMemcpyAsync(&overflow, ws.range_bound.p + nq, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  if (kn.stats_print) {
    uint64_t bound_total = 0;
    for (uint32_t b : h_bound) bound_total += b;
    fprintf(stderr, "range select ms: bound pass %.4f, evaluation %.4f, sort %.4f, placing + output %.4f; hits %llu of a bound of %llu\n",
            ms_step[0], ms_step[1], ms_step[2], ms_step[3], (unsigned long long)res->total, (unsigned long long)bound_total);
  }
  if (overflow) return fail(VI_ERR_OTHER, "radius select: a query found more hits than its bound pass counted");
  return VI_OK;
}

}  // namespace vi
