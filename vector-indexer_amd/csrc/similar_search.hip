// similar_search.hip — search by stored record: "what is similar to the record I already hold?", by external id
// (vi_indexer_search_by_ids) or for a range of all records in list order (vi_indexer_knn_graph), the record itself
// excluded on request.
//
// Nothing here ranks or selects.  A chunk of rows is (1) resolved to slots and gathered, device to device, into the
// query buffer of a search context (record_fetch.hip: resolve_records_by_id / resolve_records_by_range), (2) searched by
// the dispatcher as any device batch is (search.hip: topk_search), k + 1 wide with the hits' slots when the record itself
// is to go, and (3) taken to the caller's k-wide rows by self_drop_kernel, which deletes the one entry whose slot is the
// row's own (self_drop.hpp: why that is exact).  Without exclusion the search writes the caller's rows itself and
// absent_pad_kernel only overwrites the rows of absent ids.
//
// The cost cliff: the k + 1 of an excluding call is what picks the engine.  k = 64 leaves the VALU engine's wave top-k
// (65 > kMaxSelect) and k = 128 leaves the MFMA engine's select (129 > 2 kMaxSelect) for the generic engine, which sorts
// every candidate.  Every engine returns the reference's bits; only the time differs.  The one extra candidate is
// internal: max_k clamps the caller's k, not k + 1.
//
// Contexts: the call holds ONE search context for all its chunks and, inside it, one fetch context per chunk for the
// duration of the resolve — always in that order, search then fetch, and never two of a pool.  A get or an export holds
// a fetch context alone and waits for nothing else, so the order cannot close a cycle.
//
// Chunks: rows are processed C at a time (default 65 536, VI_GRAPH_CHUNK, clamped so that C * max(k + 1, 64) stays
// inside the dispatcher's 2^31 - 1 entries) in ascending order through the one context, whose workspace is reused.  Rows
// of a range are in list order, so the queries of a chunk probe the same few lists and the grouping's (list, query
// group) items stay dense.
//
// The radius form (vi_indexer_range_search_by_ids / vi_indexer_radius_graph) runs the same three steps with ragged rows:
// the chunk is searched by radius_search (search.hip) into a RangeResult of the context (ws.sim_range),
// range_find_kernel finds each row's own entry and writes the row's output length, range_result_place — the call the
// radius engines extend a result with, chunk of queries after chunk — extends the caller's result by those lengths, and
// range_move_kernel writes the entries behind the earlier chunks', one per row left out (self_drop.hpp: why that is
// exact).  Beside the search's workspace a chunk of C rows holds 4 C D bytes of queries, 28 bytes per hit of the
// intermediate result and 12 bytes per row.
#include <hip/hip_runtime.h>

#include <sys/time.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "device_index.hpp"
#include "record_fetch.hpp"
#include "search_internal.hpp"
#include "self_drop.hpp"

namespace vi {
namespace {

constexpr uint64_t kGraphChunkDefault = 65536;
constexpr uint64_t kBatchEntries = 0x7FFFFFFFull;  // open_batch's limit on nq x max(width, 64)

struct DropArgs {
  const float *D_in;          // [m][k + 1] the search's rows
  const int64_t *I_in;
  const uint64_t *tie_in;     // or null
  const uint64_t *slots_in;
  uint32_t *counts;           // [m] in: entries of the input row that hold a candidate; out: of the output row
  const uint32_t *self_slot;  // [m]
  const uint32_t *found;      // [m] records carrying the row's id; null: every row has its record (a range)
  float *D;                   // [m][k]
  int64_t *I;
  uint64_t *tie, *slots;      // or null
  uint32_t m, k;
};

// One wave per row, four rows per workgroup; lanes stride the row, so every access is a coalesced 4- or 8-byte one.  The
// position s of the row's own entry: a ballot over 64 entries at a time (slots are unique: at most one lane answers).
__global__ void __launch_bounds__(256) self_drop_kernel(DropArgs a) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= a.m) return;  // (wave-uniform)
  const uint32_t k = a.k, kin = k + 1u;
  const uint64_t in0 = (uint64_t)row * kin, out0 = (uint64_t)row * k;
  const bool absent = a.found && self_drop_row_absent(a.found[row]);
  uint32_t s = kSelfDropNoMatch;
  if (!absent) {
    const uint64_t self = a.self_slot[row];
    for (uint32_t j0 = 0; j0 < kin && s == kSelfDropNoMatch; j0 += 64u) {
      const uint32_t j = j0 + lane;
      const uint64_t hit = __ballot(j < kin && a.slots_in[in0 + j] == self);
      if (hit) s = j0 + (uint32_t)__ffsll((unsigned long long)hit) - 1u;
    }
  }
  const uint32_t n_in = absent ? 0u : a.counts[row];
  for (uint32_t j = lane; j < k; j += 64u) {
    float d = INFINITY;
    int64_t id = -1;
    uint64_t t = ~0ull, sl = ~0ull;
    if (!absent) {
      const uint64_t src = in0 + self_drop_src(j, s);  // (< in0 + kin: j < k)
      d = a.D_in[src];
      id = a.I_in[src];
      if (a.tie) t = a.tie_in[src];
      if (a.slots) sl = a.slots_in[src];
    }
    a.D[out0 + j] = d;
    a.I[out0 + j] = id;
    if (a.tie) a.tie[out0 + j] = t;
    if (a.slots) a.slots[out0 + j] = sl;
  }
  if (lane == 0) a.counts[row] = absent ? 0u : self_drop_count(n_in, s != kSelfDropNoMatch, k);
}

// exclude_self == 0: the search wrote the caller's rows; the rows of absent ids become padding, the others are not touched
__global__ void __launch_bounds__(256) absent_pad_kernel(const uint32_t *found, float *D, int64_t *I, uint64_t *tie, uint64_t *slots,
                                                          uint32_t *counts, uint32_t m, uint32_t k) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= m || !self_drop_row_absent(found[row])) return;  // (wave-uniform)
  const uint64_t out0 = (uint64_t)row * k;
  for (uint32_t j = lane; j < k; j += 64u) {
    D[out0 + j] = INFINITY;
    I[out0 + j] = -1;
    if (tie) tie[out0 + j] = ~0ull;
    if (slots) slots[out0 + j] = ~0ull;
  }
  if (lane == 0) counts[row] = 0u;
}

double now_ms() {
  struct timeval tv;
  gettimeofday(&tv, nullptr);
  return tv.tv_sec * 1e3 + tv.tv_usec * 1e-3;
}

thread_local SimilarTimes g_last_times{};

struct DropTimer {  // HIP events around self_drop_kernel, only under VI_SIMILAR_TIMING
  hipEvent_t a = nullptr, b = nullptr;
  ~DropTimer() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

vi_status similar_in_context(const DeviceIndex &ix, SearchContext &ctx, const SimilarIO &io) {
  SearchWorkspace &ws = ctx.ws;
  hipStream_t st = ctx.stream;
  const uint64_t k = io.k, kk = k + (io.exclude_self ? 1 : 0), dim = ix.dim;
  const uint64_t C = graph_chunk_rows(kk);
  const char *tenv = getenv("VI_SIMILAR_TIMING");
  const bool timing = tenv && *tenv && *tenv != '0';
  SimilarTimes tm{};
  tm.chunk_rows = C;
  DropTimer dt;
  if (timing) { VI_HIP(hipEventCreate(&dt.a)); VI_HIP(hipEventCreate(&dt.b)); }
  const bool want_slots = io.V != nullptr;        // of the caller's rows
  const bool want_tie = io.on_device && io.tie;
  std::vector<uint32_t> h32;

  for (uint64_t q0 = 0; q0 < io.nq; q0 += C) {
    const uint64_t m = std::min(C, io.nq - q0);
    // ---- (1) the chunk's queries: stored rows -> ws.q, their slots, the records carrying each id ----
    const double t0 = timing ? now_ms() : 0.0;
    VI_TRY(ws.q.reserve(m * dim));
    VI_TRY(ws.self_slot.reserve(m));
    if (io.ids) {
      VI_TRY(ws.self_found.reserve(m));
      VI_TRY(resolve_records_by_id(ix, io.ids + q0, m, io.on_device, ws.self_found.p, ws.q.p, ws.self_slot.p));
    } else {
      VI_TRY(resolve_records_by_range(ix, io.first + q0, m, ws.q.p, ws.self_slot.p));
    }
    const uint32_t *found = io.ids ? ws.self_found.p : nullptr;
    VI_HIP(hipSetDevice(ix.device));
    const double t1 = timing ? now_ms() : 0.0;
    // ---- (2) the search: k + 1 wide into the workspace when the record itself goes, else into the caller's rows ----
    float *D = io.D + q0 * k;  // the caller's rows of this chunk, on the device
    int64_t *I = io.I + q0 * k;
    uint64_t *tie = want_tie ? io.tie + q0 * k : nullptr, *slots = nullptr;
    if (!io.on_device) {
      VI_TRY(ws.sim_D.reserve(m * k));
      VI_TRY(ws.sim_I.reserve(m * k));
      D = ws.sim_D.p; I = ws.sim_I.p;
    }
    if (want_slots) { VI_TRY(ws.sim_slots.reserve(m * k)); slots = ws.sim_slots.p; }
    SearchIO sio;
    sio.queries = ws.q.p; sio.on_device = true; sio.nq = m; sio.k = kk; sio.n_probe = io.n_probe; sio.filter = io.filter;
    if (io.exclude_self) {
      VI_TRY(ws.D.reserve(m * kk));
      VI_TRY(ws.I.reserve(m * kk));
      VI_TRY(ws.slots.reserve(m * kk));
      if (want_tie) VI_TRY(ws.tie.reserve(m * kk));
      sio.D = ws.D.p; sio.I = ws.I.p; sio.slots = ws.slots.p; sio.tie = want_tie ? ws.tie.p : nullptr;
    } else {
      sio.D = D; sio.I = I; sio.tie = tie; sio.slots = slots;
    }
    VI_TRY(topk_search(ix, ctx, sio));  // (synchronised; ws.counts holds the rows' counts)
    ctx.stats.k = k;                    // the caller's k, not k + 1
    const double t2 = timing ? now_ms() : 0.0;
    // ---- (3) the caller's rows ----
    const dim3 grid((uint32_t)((m + 3) / 4)), block(256);
    if (io.exclude_self) {
      DropArgs a{ws.D.p, ws.I.p, sio.tie, ws.slots.p, ws.counts.p, ws.self_slot.p, found, D, I, tie, slots, (uint32_t)m, (uint32_t)k};
      if (timing) VI_HIP(hipEventRecord(dt.a, st));
      hipLaunchKernelGGL(self_drop_kernel, grid, block, 0, st, a);
      VI_HIP(hipGetLastError());
      if (timing) VI_HIP(hipEventRecord(dt.b, st));
      // read: D, I, slots (and tie) of k + 1 entries, the three words per row; written: the caller's k entries
      tm.drop_bytes += m * (kk * (20 + (want_tie ? 8 : 0)) + k * (12 + (want_tie ? 8 : 0) + (want_slots ? 8 : 0)) + 16);
    } else if (found) {
      hipLaunchKernelGGL(absent_pad_kernel, grid, block, 0, st, found, D, I, tie, slots, ws.counts.p, (uint32_t)m, (uint32_t)k);
      VI_HIP(hipGetLastError());
    }
    if (io.found && io.on_device) VI_HIP(hipMemcpyAsync(io.found + q0, found, m * 4, hipMemcpyDeviceToDevice, st));
    if (!io.on_device) {
      VI_HIP(hipMemcpyAsync(io.D + q0 * k, D, m * k * sizeof(float), hipMemcpyDeviceToHost, st));
      VI_HIP(hipMemcpyAsync(io.I + q0 * k, I, m * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
      if (io.found) VI_HIP(hipMemcpyAsync(io.found + q0, found, m * 4, hipMemcpyDeviceToHost, st));
      if (io.V) {
        VI_TRY(ws.V.reserve(m * k * dim));
        VI_TRY(launch_gather_vectors(ix, slots, m * k, ws.V.p, st));
        VI_HIP(hipMemcpyAsync(io.V + q0 * k * dim, ws.V.p, m * k * dim * sizeof(float), hipMemcpyDeviceToHost, st));
      }
      if (io.counts) {
        h32.resize(m);
        VI_HIP(hipMemcpyAsync(h32.data(), ws.counts.p, m * 4, hipMemcpyDeviceToHost, st));
      }
    }
    VI_HIP(hipStreamSynchronize(st));  // (the next chunk's resolve writes ws.q and ws.self_slot from a stream of its own)
    if (!io.on_device && io.counts)
      for (uint64_t i = 0; i < m; ++i) io.counts[q0 + i] = h32[i];
    if (timing) {
      tm.ms_resolve += (float)(t1 - t0);
      tm.ms_search += (float)(t2 - t1);
      if (io.exclude_self) tm.ms_drop += elapsed_ms(dt.a, dt.b);
    }
  }
  g_last_times = tm;
  return VI_OK;
}

// ---- the radius form: a chunk's CSR result -> the caller's CSR result, one entry per row deleted ----
struct RangeFindArgs {
  const uint64_t *in_lims;   // [m + 1] the chunk's search result
  const uint64_t *in_slots;
  uint32_t *self_pos;        // [m] in: the slot of the row's record; out: the position of its entry in the row, or kSelfDropNoMatch
  const uint32_t *found;     // [m] records carrying the row's id; null: every row has its record (a range)
  uint32_t *len;             // [m] out: entries of the output row
  uint32_t m, exclude;
};

// One wave per row, four rows per workgroup.  The row's slots are searched 64 at a time by ballot (slots are unique: at
// most one lane answers, and the search ends there); without exclusion nothing is read but the row's bounds.
__global__ void __launch_bounds__(256) range_find_kernel(RangeFindArgs a) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= a.m) return;  // (wave-uniform)
  const bool absent = a.found && self_drop_row_absent(a.found[row]);
  const uint64_t in0 = a.in_lims[row];
  const uint32_t len = (uint32_t)(a.in_lims[row + 1] - in0);  // (a chunk holds fewer than 2^31 entries)
  uint32_t s = kSelfDropNoMatch;
  if (a.exclude && !absent) {
    const uint64_t self = a.self_pos[row];
    for (uint32_t j0 = 0; j0 < len && s == kSelfDropNoMatch; j0 += 64u) {
      const uint32_t j = j0 + lane;
      const uint64_t hit = __ballot(j < len && a.in_slots[in0 + j] == self);
      if (hit) s = j0 + (uint32_t)__ffsll((unsigned long long)hit) - 1u;
    }
  }
  if (lane == 0) {
    a.self_pos[row] = s;
    a.len[row] = range_drop_len(len, s != kSelfDropNoMatch, absent);
  }
}

struct RangeMoveArgs {
  const uint64_t *in_lims;    // [m + 1]
  const uint64_t *out_lims;   // [m + 1] the caller's lims from this chunk's first row on
  const uint32_t *self_pos;   // [m] as range_find_kernel left it
  const float *D_in;
  const int64_t *I_in;
  const uint64_t *tie_in, *slots_in;
  float *D;
  int64_t *I;
  uint64_t *tie, *slots;
  uint32_t m;
};

// One wave per row again; lanes stride the row, so every access is a coalesced 4- or 8-byte one.  The row of an absent
// id has length 0 and moves nothing.
__global__ void __launch_bounds__(256) range_move_kernel(RangeMoveArgs a) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= a.m) return;  // (wave-uniform)
  const uint64_t out0 = a.out_lims[row];
  const uint32_t n = (uint32_t)(a.out_lims[row + 1] - out0);
  if (n == 0) return;
  const uint64_t in0 = a.in_lims[row];
  const uint32_t s = a.self_pos[row];
  for (uint32_t j = lane; j < n; j += 64u) {
    const uint64_t src = range_drop_src(in0, j, s);  // (< in_lims[row + 1]: n is the row's length less the match)
    a.D[out0 + j] = a.D_in[src];
    a.I[out0 + j] = a.I_in[src];
    a.tie[out0 + j] = a.tie_in[src];
    a.slots[out0 + j] = a.slots_in[src];
  }
}

struct EventPairs {  // HIP events around the two kernels, only under VI_SIMILAR_TIMING
  hipEvent_t ev[4] = {};
  ~EventPairs() {
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

vi_status range_similar_in_context(const DeviceIndex &ix, SearchContext &ctx, const RangeSimilarIO &io, RangeResult *out) {
  SearchWorkspace &ws = ctx.ws;
  hipStream_t st = ctx.stream;
  const uint64_t dim = ix.dim;
  const uint64_t C = graph_chunk_rows(64);
  const char *tenv = getenv("VI_SIMILAR_TIMING");
  const bool timing = tenv && *tenv && *tenv != '0';
  SimilarTimes tm{};
  tm.chunk_rows = C;
  EventPairs ep;
  if (timing)
    for (auto &e : ep.ev) VI_HIP(hipEventCreate(&e));
  RangeIO rio;
  rio.on_device = true; rio.n_probe = io.n_probe; rio.radius2 = io.radius2; rio.filter = io.filter;
  if (io.nq == 0) {  // an empty result, made as a radius search of no query makes it
    VI_TRY(radius_search(ix, ctx, rio, out));
    VI_HIP(hipStreamSynchronize(st));
    g_last_times = tm;
    return VI_OK;
  }
  // found is the caller's only once every chunk has succeeded: until then it is kept here
  const bool want_found = io.found && io.ids;
  std::vector<uint32_t> h_found;
  DevBuf<uint32_t> d_found;
  if (want_found && !io.on_device) h_found.resize(io.nq);
  if (want_found && io.on_device && io.nq > C) VI_TRY(d_found.reserve(io.nq));

  RangeResult &in = ws.sim_range;
  VI_TRY(range_result_begin(ix, io.nq, out));
  for (uint64_t q0 = 0; q0 < io.nq; q0 += C) {
    const uint64_t m = std::min(C, io.nq - q0);
    // ---- (1) the chunk's queries: stored rows -> ws.q, their slots, the records carrying each id ----
    const double t0 = timing ? now_ms() : 0.0;
    VI_TRY(ws.q.reserve(m * dim));
    VI_TRY(ws.self_slot.reserve(m));
    VI_TRY(ws.sim_len.reserve(m));
    if (io.ids) {
      VI_TRY(ws.self_found.reserve(m));
      VI_TRY(resolve_records_by_id(ix, io.ids + q0, m, io.on_device, ws.self_found.p, ws.q.p, ws.self_slot.p));
    } else {
      VI_TRY(resolve_records_by_range(ix, io.first + q0, m, ws.q.p, ws.self_slot.p));
    }
    const uint32_t *found = io.ids ? ws.self_found.p : nullptr;
    VI_HIP(hipSetDevice(ix.device));
    const double t1 = timing ? now_ms() : 0.0;
    // ---- (2) the radius search of the chunk, into the context's own result ----
    rio.queries = ws.q.p; rio.nq = m;
    VI_TRY(radius_search(ix, ctx, rio, &in));  // (synchronised)
    const double t2 = timing ? now_ms() : 0.0;
    // ---- (3) every row's own entry and its output length ----
    const dim3 grid((uint32_t)((m + 3) / 4)), block(256);
    RangeFindArgs fa{in.lims.p, in.slots.p, ws.self_slot.p, found, ws.sim_len.p, (uint32_t)m, io.exclude_self ? 1u : 0u};
    if (timing) VI_HIP(hipEventRecord(ep.ev[0], st));
    hipLaunchKernelGGL(range_find_kernel, grid, block, 0, st, fa);
    VI_HIP(hipGetLastError());
    if (timing) VI_HIP(hipEventRecord(ep.ev[1], st));
    // ---- (4) the caller's result extended by the chunk's rows ----
    VI_TRY(range_result_place(out, q0, m, ws.sim_len.p, st));
    // ---- (5) the entries ----
    const uint64_t moved = out->h_lims[q0 + m] - out->h_lims[q0];
    if (timing) VI_HIP(hipEventRecord(ep.ev[2], st));
    if (moved) {
      RangeMoveArgs ma{in.lims.p, out->lims.p + q0, ws.self_slot.p, in.D.p, in.I.p, in.tie.p, in.slots.p,
                       out->D.p, out->I.p, out->tie.p, out->slots.p, (uint32_t)m};
      hipLaunchKernelGGL(range_move_kernel, grid, block, 0, st, ma);
      VI_HIP(hipGetLastError());
    }
    if (timing) VI_HIP(hipEventRecord(ep.ev[3], st));
    // find: a row's bounds, slot, count, position and length, and (at most) its slots; move: bounds and position, 28
    // bytes per entry in and out
    tm.drop_bytes += m * 32 + (io.exclude_self ? in.total * 8 : 0) + m * 36 + moved * 56;
    if (want_found) {
      if (!io.on_device) VI_HIP(hipMemcpyAsync(h_found.data() + q0, found, m * 4, hipMemcpyDeviceToHost, st));
      else if (d_found.p) VI_HIP(hipMemcpyAsync(d_found.p + q0, found, m * 4, hipMemcpyDeviceToDevice, st));
    }
    VI_HIP(hipStreamSynchronize(st));  // (the next chunk's resolve writes ws.q and ws.self_slot from a stream of its own)
    if (timing) {
      tm.ms_resolve += (float)(t1 - t0);
      tm.ms_search += (float)(t2 - t1);
      tm.ms_drop += elapsed_ms(ep.ev[0], ep.ev[1]) + elapsed_ms(ep.ev[2], ep.ev[3]);
    }
  }
  if (want_found) {
    if (!io.on_device) std::copy(h_found.begin(), h_found.end(), io.found);
    else {
      VI_HIP(hipMemcpyAsync(io.found, d_found.p ? d_found.p : ws.self_found.p, io.nq * 4, hipMemcpyDeviceToDevice, st));
      VI_HIP(hipStreamSynchronize(st));
    }
  }
  g_last_times = tm;
  return VI_OK;
}

}  // namespace

// rows per chunk: VI_GRAPH_CHUNK or the default, inside [1, what the dispatcher takes at this width]
uint64_t graph_chunk_rows(uint64_t width) {
  const char *e = getenv("VI_GRAPH_CHUNK");
  uint64_t c = (e && *e) ? strtoull(e, nullptr, 10) : kGraphChunkDefault;
  const uint64_t most = kBatchEntries / std::max<uint64_t>(width, 64);
  return std::min(std::max<uint64_t>(c, 1), most);
}

SimilarTimes similar_last_times() { return g_last_times; }

vi_status device_index_range_similar(const DeviceIndex &ix, const RangeSimilarIO &io, RangeResult *out) {
  g_last_times = SimilarTimes{};
  if (!ix.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no external ids");
  const vi_status s = with_search_context(ix, [&](SearchContext &ctx) { return range_similar_in_context(ix, ctx, io, out); });
  if (s != VI_OK) (void)hipGetLastError();  // (a failed allocation is this call's failure, not the next call's)
  return s;
}

vi_status device_index_search_similar(const DeviceIndex &ix, const SimilarIO &io) {
  g_last_times = SimilarTimes{};
  if (!ix.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no external ids");
  return with_search_context(ix, [&](SearchContext &ctx) { return similar_in_context(ix, ctx, io); });
}

}  // namespace vi
