// search.hip — the dispatcher: the two public entries (device_index_search, device_index_range_search) and what is common
// to the three engines behind them.  An entry leases a SearchContext of the handle, opens a SearchBatch on it (checks, the
// clamp of n_probe, the stats reset, the knobs, the queries on the device), picks the engine — MFMA (mfma_search.hip),
// exact-order VALU (search_kernels.hip) or generic (generic_search.hip) — hands it the batch and closes it (stripe ties,
// the one synchronisation, phase times).  Also here: the RangeResult assembly the radius engines fill chunk by chunk.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device_index.hpp"
#include "search_internal.hpp"
#include "slot_filter.hpp"

namespace vi {

// striped lists: local position -> position in the whole list, so that the merge over ranks sees the
// reference's candidate order
__global__ void stripe_tie_kernel(uint64_t *tie, uint64_t n, uint32_t rank, uint32_t world) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t t = tie[i];
  if (t == ~0ull) return;
  const uint32_t p = (uint32_t)t;
  tie[i] = (t & 0xFFFFFFFF00000000ull) | (uint64_t)(((p >> 6) * world + rank) * 64u + (p & 63u));
}

namespace {

constexpr int kWave = 64;
// Minimum blocks (x64 vectors) per list segment of the VALU list scan.  Measured on the C2 workload (profiles/
// r01_experiments.md): cutting lists finer than this costs more in repeated top-k warm-up than it
// gains in load balance, so only extreme lists (> 64k vectors) are cut (seg 256 measured +9 %).
constexpr uint32_t kSegBlocksDefault = 1024;

// gather result vectors (include_vectors, api.rs:213-217) back to row-major
__global__ void gather_vectors_kernel(const float *blocks, uint32_t dq, uint32_t dim, const uint64_t *slots,
                                      uint64_t nres, float *V) {
  const uint64_t r = blockIdx.x;
  if (r >= nres) return;
  const uint64_t s = slots[r];
  for (uint32_t e = threadIdx.x; e < dim; e += blockDim.x) {
    float val = 0.0f;
    if (s != ~0ull) {
      const uint64_t blk = s / kWave, ln = s % kWave;
      val = blocks[((blk * dq + e / 4) * kWave + ln) * 4 + (e & 3)];
    }
    V[r * dim + e] = val;
  }
}

// What both entries open a batch with: the checks on the arguments (the filter's index; nq x `width` result entries indexed
// in 32 bits), n_probe clamped to the lists, the context's stats reset, the knobs read — once per call: they may change.
vi_status open_batch(SearchBatch &b, uint64_t nq, uint64_t k, uint64_t n_probe, uint64_t width) {
  if (b.flt && b.flt->owner_serial != b.ix.serial) return fail(VI_ERR_INVALID_INPUT, "the filter was made for another index");
  if (nq * width > 0x7FFFFFFFull) return fail(VI_ERR_INVALID_INPUT, "batch too large: split nq");
  b.nq = nq;
  b.P = (uint32_t)std::min<uint64_t>(n_probe, b.ix.nlists);  // take(n_probe) (ivf_index.rs:216-220)
  b.kn = read_engine_knobs();
  vi_search_stats &stt = b.ctx.stats;
  stt = vi_search_stats{};
  stt.nq = nq; stt.k = k; stt.n_probe_eff = b.P; stt.coarse_candidates = nq * b.ix.nlists;
  return VI_OK;
}
// ... and, once there is something to search, the queries on the device (b.Qd) and the counter block
vi_status stage_queries(SearchBatch &b, const float *queries, bool on_device) {
  b.Qd = queries;
  if (!on_device) {
    VI_TRY(b.ws().q.reserve(b.nq * b.ix.dim));
    b.Qd = b.ws().q.p;
    VI_HIP(hipMemcpyAsync(b.ws().q.p, queries, b.nq * b.ix.dim * sizeof(float), hipMemcpyHostToDevice, b.st()));
  }
  return b.ws().stats.reserve(kStatWords);
}
// the n tie keys of a striped index made list positions; the search's one final synchronisation; the phase times
vi_status close_batch(SearchBatch &b, uint64_t *tie, uint64_t n) {
  if (b.ix.stripe_world > 1 && tie && n) {
    hipLaunchKernelGGL(stripe_tie_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, b.st(), tie, n, b.ix.stripe_rank,
                       b.ix.stripe_world);
    VI_HIP(hipGetLastError());
  }
  VI_HIP(hipStreamSynchronize(b.st()));
  vi_search_stats &s = b.ctx.stats;
  const hipEvent_t *ev = b.ctx.ev;
  if (b.timing) (void)hipEventElapsedTime(&s.ms_scan, ev[2], ev[3]);
  if (b.timing != 1) return VI_OK;
  (void)hipEventElapsedTime(&s.ms_coarse, ev[0], ev[1]);
  (void)hipEventElapsedTime(&s.ms_group, ev[1], ev[2]);
  (void)hipEventElapsedTime(&s.ms_merge, ev[3], ev[4]);
  (void)hipEventElapsedTime(&s.ms_total, ev[0], ev[4]);
  return VI_OK;
}

}  // namespace

vi_status launch_gather_vectors(const DeviceIndex &ix, const uint64_t *slots, uint64_t nres, float *V, hipStream_t st) {
  if (nres == 0) return VI_OK;
  hipLaunchKernelGGL(gather_vectors_kernel, dim3((uint32_t)nres), dim3(64), 0, st, ix.lists.blocks.p, ix.dq, ix.dim, slots, nres, V);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

// ---- top-k search (fast engines: n_probe_eff <= 64 and k <= 64, the MFMA engine k <= 128) ----
vi_status topk_search(const DeviceIndex &ix, SearchContext &ctx, const SearchIO &io) {
  SearchWorkspace &ws = ctx.ws;
  hipStream_t st = ctx.stream;
  const uint64_t nq = io.nq, k = io.k, dim = ix.dim;
  if (nq == 0) return VI_OK;  // (before any check, the context's stats as they were)
  SearchBatch b{ix, ctx, io.filter, io.probes_in, io.order_in};
  VI_TRY(open_batch(b, nq, k, io.n_probe, std::max<uint64_t>(k, 64)));
  const uint32_t P = b.P;
  // k in (64, 128]: the MFMA engine's select keeps two entries per lane; the VALU engine's wave top-k stops at 64
  const bool mfma_ok = mfma_path_applicable(ix, b.kn, k, P);
  const bool generic = P > kMaxSelect || k > 2 * kMaxSelect || (k > kMaxSelect && !mfma_ok) || b.kn.force_generic;

  // ---- outputs / queries on device ----
  SelectOutputs out{io.D, io.I, io.tie, nullptr, nullptr};
  if (!io.on_device) {
    VI_TRY(ws.D.reserve(nq * k));
    VI_TRY(ws.I.reserve(nq * k));
    out.D = ws.D.p; out.I = ws.I.p; out.tie = nullptr;
  }
  VI_TRY(stage_queries(b, io.queries, io.on_device));
  VI_TRY(ws.counts.reserve(nq));
  out.counts = ws.counts.p;
  if (io.V) { VI_TRY(ws.slots.reserve(nq * k)); out.slots = ws.slots.p; }
  else if (io.on_device) out.slots = io.slots;

  if (P == 0 || ix.nlists == 0) {  // empty index: every query has zero results
    std::vector<float> hD(nq * k, INFINITY);
    std::vector<int64_t> hI(nq * k, -1);
    if (io.on_device) {
      VI_HIP(hipMemcpy(io.D, hD.data(), hD.size() * 4, hipMemcpyHostToDevice));
      VI_HIP(hipMemcpy(io.I, hI.data(), hI.size() * 8, hipMemcpyHostToDevice));
    } else {
      std::memcpy(io.D, hD.data(), hD.size() * 4);
      std::memcpy(io.I, hI.data(), hI.size() * 8);
      if (io.counts) std::memset(io.counts, 0, nq * 8);
      if (io.V) std::memset(io.V, 0, nq * k * dim * 4);
    }
    if (io.prune && io.prune->n_kept) {  // adaptive probing: no query probed anything
      if (io.on_device) VI_HIP(hipMemset(io.prune->n_kept, 0, nq * sizeof(uint32_t)));
      else std::memset(io.prune->n_kept, 0, nq * sizeof(uint32_t));
    }
    return VI_OK;
  }

  if (io.probes_out) {  // coarse step only (multi-GPU: this rank's slice of the queries)
    if (P > kMaxSelect) VI_TRY(generic_probe_export(b));  // any n_probe: every coarse distance, sorted
    else if (coarse_on_matrix_cores(ix, b.kn, nq, P)) VI_TRY(coarse_only_mfma(b));
    else VI_TRY(stage_coarse(b));
    VI_HIP(hipMemcpyAsync(io.probes_out, ws.probes.p, nq * P * 4, hipMemcpyDeviceToDevice, st));
    VI_HIP(hipMemcpyAsync(io.order_out, ws.gorder.p, nq * P * 4, hipMemcpyDeviceToDevice, st));
    VI_HIP(hipStreamSynchronize(st));
    return VI_OK;
  }
  b.timing = generic ? 0 : ix.timing;
  PruneRun prune;  // adaptive probing: the engine prunes the rows of its coarse step before its list phase
  if (io.prune && !io.probes_in) {
    VI_TRY(prune_begin(prune, io.prune, !io.on_device));
    b.prune = &prune;
  }
  if (generic) VI_TRY(device_index_search_generic(b, k, out));  // (k > 128 or n_probe > 64, with the caller's probe lists too)
  else if (mfma_ok) VI_TRY(search_mfma_pipeline(b, k, out));
  else VI_TRY(search_valu_pipeline(b, k, out));

  // ---- results ----
  if (!io.on_device) {
    VI_HIP(hipMemcpyAsync(io.D, out.D, nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
    VI_HIP(hipMemcpyAsync(io.I, out.I, nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (io.V) {
      VI_TRY(ws.V.reserve(nq * k * dim));
      hipLaunchKernelGGL(gather_vectors_kernel, dim3((uint32_t)(nq * k)), dim3(64), 0, st, ix.lists.blocks.p, ix.dq, ix.dim,
                         out.slots, nq * k, ws.V.p);
      VI_HIP(hipGetLastError());
      VI_HIP(hipMemcpyAsync(io.V, ws.V.p, nq * k * dim * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    if (io.counts) {
      std::vector<uint32_t> c32(nq);
      VI_HIP(hipMemcpyAsync(c32.data(), ws.counts.p, nq * 4, hipMemcpyDeviceToHost, st));
      VI_HIP(hipStreamSynchronize(st));
      for (uint64_t i = 0; i < nq; ++i) io.counts[i] = c32[i];
    }
  }
  VI_TRY(close_batch(b, out.tie, nq * k));  // (host outputs carry no tie keys)
  if (b.prune) prune_finish(prune);
  return VI_OK;
}

namespace {

// a result buffer grown to `cap` entries with its first `used` kept
template <typename T>
vi_status grow_keeping(DevBuf<T> &b, uint64_t used, uint64_t cap, hipStream_t st) {
  DevBuf<T> bigger;
  VI_TRY(bigger.reserve(cap));
  if (used) VI_HIP(hipMemcpyAsync(bigger.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, st));
  VI_HIP(hipStreamSynchronize(st));
  std::swap(b.p, bigger.p);
  std::swap(b.n, bigger.n);
  return VI_OK;
}

}  // namespace

// ---- radius search ----
vi_status radius_search(const DeviceIndex &ix, SearchContext &ctx, const RangeIO &io, RangeResult *out) {
  SearchBatch b{ix, ctx, io.filter, nullptr, nullptr};
  VI_TRY(open_batch(b, io.nq, 0, io.n_probe, 64));
  VI_TRY(range_result_begin(ix, io.nq, out));
  // nothing to find: no query, an empty index, or a radius no squared distance is within
  if (io.nq == 0 || b.P == 0 || ix.nlists == 0 || io.radius2 < 0.0f) return range_result_place(out, 0, 0, nullptr, b.st());
  VI_TRY(stage_queries(b, io.queries, io.on_device));
  // the MFMA engine has no k to limit it; everything else (D % 4 != 0, D > 1536, n_probe > 64, VI_FILTER=0) sorts every candidate
  const bool mfma = !b.kn.force_generic && mfma_path_applicable(ix, b.kn, 1, b.P);
  b.timing = mfma ? ix.timing : 0;
  if (mfma) VI_TRY(range_mfma_pipeline(b, io.radius2, out));
  else VI_TRY(device_index_range_generic(b, io.radius2, out));
  return close_batch(b, out->tie.p, out->total);
}

EngineKnobs read_engine_knobs() {
  auto on = [](const char *name) { const char *e = getenv(name); return !(e && *e == '0'); };
  auto num = [](const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; };
  auto u32 = [](const char *name, uint32_t dflt) {  // (unset or empty: the default)
    const char *e = getenv(name);
    return (e && *e) ? (uint32_t)strtoul(e, nullptr, 10) : dflt;
  };
  const char *stats = getenv("VI_FILTER_STATS"), *approx = getenv("VI_RANK_APPROX"), *gq = getenv("VI_FILTER_GQ");
  const char *stream = getenv("VI_RANK_STREAM");
  EngineKnobs kn{};
  kn.force_generic = u32("VI_FORCE_GENERIC", 0) != 0;
  kn.force_qg = u32("VI_FORCE_QG", 0);
  kn.seg_blocks = std::max<uint32_t>(1, u32("VI_SEG_BLOCKS", kSegBlocksDefault));
  kn.mfma = on("VI_FILTER");
  kn.rank_bf16 = on("VI_FILTER_BF16");
  kn.hi_only = on("VI_FILTER_HI_ONLY");
  kn.rank_approx = -1;
  if (approx) { const int v = atoi(approx); kn.rank_approx = v < 0 || v > 2 ? 1 : v; }
  kn.debug_approx = getenv("VI_DEBUG_APPROX") != nullptr;
  kn.coarse_mfma = on("VI_COARSE_FILTER");
  kn.coarse_direct = on("VI_COARSE_DIRECT");
  kn.segb0 = (uint32_t)std::max(1, num("VI_FILTER_SEGB", 32));  // <= 2048 vectors per work item
  kn.gq = gq ? (atoi(gq) == 32 ? 32u : 128u) : 0u;
  kn.stream_off = stream && *stream == '0';
  kn.stream_force = stream && *stream == '1';
  kn.stream_gq256 = num("VI_STREAM_GQ", 0) == 256;
  kn.rank_i8 = on("VI_RANK_I8");
  kn.item_run = (uint32_t)std::min(std::max(num("VI_ITEM_RUN", 8), 1), 256);
  kn.item_push = on("VI_ITEM_PUSH");
  kn.scan_in_totals = on("VI_SCAN_IN_TOTALS");
  kn.stream_prof = getenv("VI_STREAM_PROF") != nullptr;
  kn.stream_prof_dump = getenv("VI_STREAM_PROF_DUMP");
  kn.rank_xmode = (uint32_t)num("VI_FILTER_XMODE", 0);
  kn.select_xmode = (uint32_t)num("VI_SELECT_XMODE", 0);
  kn.coarse_xmode = (uint32_t)num("VI_SELECT_XMODE_COARSE", 0);
  kn.stats = stats != nullptr;
  kn.stats_coarse = stats && *stats == '2';
  kn.stats_print = stats && (*stats == '3' || *stats == '4');
  kn.stats_mask = stats && *stats == '4' ? 63u : 0u;
  return kn;
}

vi_status device_index_search(const DeviceIndex &ix, const SearchIO &io) {
  return with_search_context(ix, [&](SearchContext &ctx) { return topk_search(ix, ctx, io); });
}

vi_status device_index_range_search(const DeviceIndex &ix, const RangeIO &io, RangeResult *out) {
  return with_search_context(ix, [&](SearchContext &ctx) { return radius_search(ix, ctx, io, out); });
}

vi_status range_result_begin(const DeviceIndex &ix, uint64_t nq, RangeResult *res) {
  res->ix = &ix;
  res->device = ix.device;
  res->nq = nq;
  res->total = 0;
  res->h_lims.assign(nq + 1, 0);
  return res->lims.reserve(nq + 1);  // (written by range_result_place: every call fills it from its first query on)
}

vi_status range_result_place(RangeResult *res, uint64_t q0, uint64_t m, const uint32_t *counts_dev, hipStream_t st) {
  std::vector<uint32_t> h(m);
  if (m) {
    VI_HIP(hipMemcpyAsync(h.data(), counts_dev, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
  }
  for (uint64_t i = 0; i < m; ++i) res->h_lims[q0 + i + 1] = res->h_lims[q0 + i] + h[i];
  const uint64_t total = res->h_lims[q0 + m];
  for (uint64_t q = q0 + m; q < res->nq; ++q) res->h_lims[q + 1] = total;  // (queries still to come: empty so far)
  if (total > res->cap || !res->D.p) {
    // (one chunk — the rule — allocates exactly; a further chunk at least doubles)
    const uint64_t cap = std::max<uint64_t>(1, res->cap ? std::max(total, 2 * res->cap) : total);
    VI_TRY(grow_keeping(res->D, res->total, cap, st));
    VI_TRY(grow_keeping(res->I, res->total, cap, st));
    VI_TRY(grow_keeping(res->tie, res->total, cap, st));
    VI_TRY(grow_keeping(res->slots, res->total, cap, st));
    res->cap = cap;
  }
  res->total = total;
  VI_HIP(hipMemcpyAsync(res->lims.p + q0, res->h_lims.data() + q0, (res->nq + 1 - q0) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  return VI_OK;
}

vi_status range_result_copy(const RangeResult &r, uint64_t *lims, float *D, int64_t *I, float *V) {
  if (V && !r.ix) return fail(VI_ERR_INVALID_INPUT, "a merged result has no stored vectors: they live on the ranks");
  if (lims) std::memcpy(lims, r.h_lims.data(), (r.nq + 1) * sizeof(uint64_t));
  if (r.total == 0) return VI_OK;
  VI_HIP(hipSetDevice(r.device));
  if (D) VI_HIP(hipMemcpy(D, r.D.p, r.total * sizeof(float), hipMemcpyDeviceToHost));
  if (I) VI_HIP(hipMemcpy(I, r.I.p, r.total * sizeof(int64_t), hipMemcpyDeviceToHost));
  if (V) {
    const uint32_t dim = r.ix->dim;
    DevBuf<float> Vd;
    const uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(r.total, (1ull << 28) / dim));  // <= 1 GiB of rows at a time
    VI_TRY(Vd.reserve(step * dim));
    for (uint64_t at = 0; at < r.total; at += step) {
      const uint64_t n = std::min(step, r.total - at);
      hipLaunchKernelGGL(gather_vectors_kernel, dim3((uint32_t)n), dim3(64), 0, nullptr, r.ix->lists.blocks.p, r.ix->dq, dim,
                         r.slots.p + at, n, Vd.p);
      VI_HIP(hipGetLastError());
      VI_HIP(hipMemcpy(V + at * dim, Vd.p, n * dim * sizeof(float), hipMemcpyDeviceToHost));
    }
  }
  return VI_OK;
}

}  // namespace vi
