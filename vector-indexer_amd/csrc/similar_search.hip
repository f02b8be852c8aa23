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
// The rows come chunk by chunk from the walk over stored records (StoredRowsWalk, defined at the end of this file and
// declared in search_internal.hpp; DESIGN.md "The walk over stored records": the chunk size, the order of the two
// contexts, the synchronise between chunks, the timing).  cluster_radius.hip is its third caller.
//
// The radius form (vi_indexer_range_search_by_ids / vi_indexer_radius_graph) runs the same three steps with ragged rows:
// the chunk is searched by radius_search (search.hip) into a RangeResult of the context (ws.sim_range),
// range_find_kernel finds each row's own entry and writes the row's output length, range_result_place — the call the
// radius engines extend a result with, chunk of queries after chunk — extends the caller's result by those lengths, and
// range_move_kernel writes the entries behind the earlier chunks', one per row left out (self_drop.hpp: why that is
// exact).  Beside the search's workspace a chunk of C rows holds 4 C D bytes of queries, 28 bytes per hit of the
// intermediate result and 12 bytes per row.
#include <hip/hip_runtime.h>

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

// The position of the one entry of slots[in0, in0 + len) that holds `self`, or kSelfDropNoMatch: a ballot over 64 entries
// at a time (slots are unique: at most one lane answers, and the search ends there).  A whole wave calls it with the same
// in0, len and self, so the loop bound is wave-uniform and the ballot sees all 64 lanes.
__device__ __forceinline__ uint32_t find_self_entry(const uint64_t *slots, uint64_t in0, uint32_t len, uint64_t self, uint32_t lane) {
  uint32_t s = kSelfDropNoMatch;
  for (uint32_t j0 = 0; j0 < len && s == kSelfDropNoMatch; j0 += 64u) {
    const uint32_t j = j0 + lane;
    const uint64_t hit = __ballot(j < len && slots[in0 + j] == self);
    if (hit) s = j0 + (uint32_t)__ffsll((unsigned long long)hit) - 1u;
  }
  return s;
}

// One wave per row, four rows per workgroup; lanes stride the row, so every access is a coalesced 4- or 8-byte one.
__global__ void __launch_bounds__(256) self_drop_kernel(DropArgs a) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= a.m) return;  // (wave-uniform)
  const uint32_t k = a.k, kin = k + 1u;
  const uint64_t in0 = (uint64_t)row * kin, out0 = (uint64_t)row * k;
  const bool absent = a.found && self_drop_row_absent(a.found[row]);
  const uint32_t s = absent ? kSelfDropNoMatch : find_self_entry(a.slots_in, in0, kin, a.self_slot[row], lane);
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

thread_local SimilarTimes g_last_times{};

// the thread's report of a call that went through: the walk's figures beside the caller's ms_drop and drop_bytes
void report_times(SimilarTimes tm, const StoredRowsWalk &walk) {
  tm.ms_resolve = walk.ms_resolve; tm.ms_search = walk.ms_search; tm.chunk_rows = walk.chunk_rows;
  g_last_times = tm;
}

vi_status similar_in_context(const DeviceIndex &ix, SearchContext &ctx, const SimilarIO &io) {
  SearchWorkspace &ws = ctx.ws;
  hipStream_t st = ctx.stream;
  const bool on_device = io.rows.on_device;
  const uint64_t k = io.k, kk = k + (io.exclude_self ? 1 : 0), dim = ix.dim;
  StoredRowsWalk walk(kk);
  EventSpans<1> drop;  // around self_drop_kernel
  VI_TRY(drop.create(walk.timing));
  SimilarTimes tm{};
  const bool want_slots = io.V != nullptr;        // of the caller's rows
  const bool want_tie = on_device && io.tie;
  std::vector<uint32_t> h32;

  const auto body = [&](const RowChunk &c) -> vi_status {
    const uint64_t q0 = c.q0, m = c.m;
    // ---- the search: k + 1 wide into the workspace when the record itself goes, else into the caller's rows ----
    float *D = io.D + q0 * k;  // the caller's rows of this chunk, on the device
    int64_t *I = io.I + q0 * k;
    uint64_t *tie = want_tie ? io.tie + q0 * k : nullptr, *slots = nullptr;
    if (!on_device) {
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
    c.mark_searched();
    // ---- the caller's rows ----
    const dim3 grid((uint32_t)((m + 3) / 4)), block(256);
    if (io.exclude_self) {
      DropArgs a{ws.D.p, ws.I.p, sio.tie, ws.slots.p, ws.counts.p, ws.self_slot.p, c.found, D, I, tie, slots, (uint32_t)m, (uint32_t)k};
      VI_TRY(drop.begin(0, st));
      hipLaunchKernelGGL(self_drop_kernel, grid, block, 0, st, a);
      VI_HIP(hipGetLastError());
      VI_TRY(drop.end(0, st));
      // read: D, I, slots (and tie) of k + 1 entries, the three words per row; written: the caller's k entries
      tm.drop_bytes += m * (kk * (20 + (want_tie ? 8 : 0)) + k * (12 + (want_tie ? 8 : 0) + (want_slots ? 8 : 0)) + 16);
    } else if (c.found) {
      hipLaunchKernelGGL(absent_pad_kernel, grid, block, 0, st, c.found, D, I, tie, slots, ws.counts.p, (uint32_t)m, (uint32_t)k);
      VI_HIP(hipGetLastError());
    }
    if (io.found && on_device) VI_HIP(hipMemcpyAsync(io.found + q0, c.found, m * 4, hipMemcpyDeviceToDevice, st));
    if (!on_device) {
      VI_HIP(hipMemcpyAsync(io.D + q0 * k, D, m * k * sizeof(float), hipMemcpyDeviceToHost, st));
      VI_HIP(hipMemcpyAsync(io.I + q0 * k, I, m * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
      if (io.found) VI_HIP(hipMemcpyAsync(io.found + q0, c.found, m * 4, hipMemcpyDeviceToHost, st));
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
    return VI_OK;
  };
  const auto landed = [&](const RowChunk &c) -> vi_status {
    if (!on_device && io.counts)
      for (uint64_t i = 0; i < c.m; ++i) io.counts[c.q0 + i] = h32[i];
    if (io.exclude_self) tm.ms_drop += drop.ms(0);
    return VI_OK;
  };
  VI_TRY(walk.run(ix, ctx, io.rows, body, landed));
  report_times(tm, walk);
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

// One wave per row, four rows per workgroup.  Without exclusion nothing is read but the row's bounds.
__global__ void __launch_bounds__(256) range_find_kernel(RangeFindArgs a) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= a.m) return;  // (wave-uniform)
  const bool absent = a.found && self_drop_row_absent(a.found[row]);
  const uint64_t in0 = a.in_lims[row];
  const uint32_t len = (uint32_t)(a.in_lims[row + 1] - in0);  // (a chunk holds fewer than 2^31 entries)
  const uint32_t s = a.exclude && !absent ? find_self_entry(a.in_slots, in0, len, a.self_pos[row], lane) : kSelfDropNoMatch;
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

vi_status range_similar_in_context(const DeviceIndex &ix, SearchContext &ctx, const RangeSimilarIO &io, RangeResult *out) {
  SearchWorkspace &ws = ctx.ws;
  hipStream_t st = ctx.stream;
  const StoredRows &rows = io.rows;
  StoredRowsWalk walk(64);
  EventSpans<2> drop;  // around range_find_kernel and around range_move_kernel: not range_result_place between them
  VI_TRY(drop.create(walk.timing));
  SimilarTimes tm{};
  RangeIO rio;
  rio.on_device = true; rio.n_probe = io.n_probe; rio.radius2 = io.radius2; rio.filter = io.filter;
  if (rows.nq == 0) {  // an empty result, made as a radius search of no query makes it
    VI_TRY(radius_search(ix, ctx, rio, out));
    VI_HIP(hipStreamSynchronize(st));
    report_times(tm, walk);
    return VI_OK;
  }
  // found is the caller's only once every chunk has succeeded: until then it is kept here
  const bool want_found = io.found && rows.ids;
  std::vector<uint32_t> h_found;
  DevBuf<uint32_t> d_found;
  if (want_found && !rows.on_device) h_found.resize(rows.nq);
  if (want_found && rows.on_device && rows.nq > walk.chunk_rows) VI_TRY(d_found.reserve(rows.nq));

  RangeResult &in = ws.sim_range;
  VI_TRY(range_result_begin(ix, rows.nq, out));
  const auto body = [&](const RowChunk &c) -> vi_status {
    const uint64_t q0 = c.q0, m = c.m;
    // ---- the radius search of the chunk, into the context's own result ----
    VI_TRY(ws.sim_len.reserve(m));
    rio.queries = ws.q.p; rio.nq = m;
    VI_TRY(radius_search(ix, ctx, rio, &in));  // (synchronised)
    c.mark_searched();
    // ---- every row's own entry and its output length ----
    const dim3 grid((uint32_t)((m + 3) / 4)), block(256);
    RangeFindArgs fa{in.lims.p, in.slots.p, ws.self_slot.p, c.found, ws.sim_len.p, (uint32_t)m, io.exclude_self ? 1u : 0u};
    VI_TRY(drop.begin(0, st));
    hipLaunchKernelGGL(range_find_kernel, grid, block, 0, st, fa);
    VI_HIP(hipGetLastError());
    VI_TRY(drop.end(0, st));
    // ---- the caller's result extended by the chunk's rows ----
    VI_TRY(range_result_place(out, q0, m, ws.sim_len.p, st));
    // ---- the entries ----
    const uint64_t moved = out->h_lims[q0 + m] - out->h_lims[q0];
    VI_TRY(drop.begin(1, st));
    if (moved) {
      RangeMoveArgs ma{in.lims.p, out->lims.p + q0, ws.self_slot.p, in.D.p, in.I.p, in.tie.p, in.slots.p,
                       out->D.p, out->I.p, out->tie.p, out->slots.p, (uint32_t)m};
      hipLaunchKernelGGL(range_move_kernel, grid, block, 0, st, ma);
      VI_HIP(hipGetLastError());
    }
    VI_TRY(drop.end(1, st));
    // find: a row's bounds, slot, count, position and length, and (at most) its slots; move: bounds and position, 28
    // bytes per entry in and out
    tm.drop_bytes += m * 32 + (io.exclude_self ? in.total * 8 : 0) + m * 36 + moved * 56;
    if (want_found) {
      if (!rows.on_device) VI_HIP(hipMemcpyAsync(h_found.data() + q0, c.found, m * 4, hipMemcpyDeviceToHost, st));
      else if (d_found.p) VI_HIP(hipMemcpyAsync(d_found.p + q0, c.found, m * 4, hipMemcpyDeviceToDevice, st));
    }
    return VI_OK;
  };
  const auto landed = [&](const RowChunk &) -> vi_status { tm.ms_drop += drop.ms(0) + drop.ms(1); return VI_OK; };
  VI_TRY(walk.run(ix, ctx, rows, body, landed));
  if (want_found) {
    if (!rows.on_device) std::copy(h_found.begin(), h_found.end(), io.found);
    else {
      VI_HIP(hipMemcpyAsync(io.found, d_found.p ? d_found.p : ws.self_found.p, rows.nq * 4, hipMemcpyDeviceToDevice, st));
      VI_HIP(hipStreamSynchronize(st));
    }
  }
  report_times(tm, walk);
  return VI_OK;
}

// rows per chunk: VI_GRAPH_CHUNK or the default, inside [1, what the dispatcher takes at this width]
uint64_t graph_chunk_rows(uint64_t width) {
  const char *e = getenv("VI_GRAPH_CHUNK");
  uint64_t c = (e && *e) ? strtoull(e, nullptr, 10) : kGraphChunkDefault;
  const uint64_t most = kBatchEntries / std::max<uint64_t>(width, 64);
  return std::min(std::max<uint64_t>(c, 1), most);
}

bool similar_timing() {
  const char *e = getenv("VI_SIMILAR_TIMING");
  return e && *e && *e != '0';
}

}  // namespace

StoredRowsWalk::StoredRowsWalk(uint64_t width) : chunk_rows(graph_chunk_rows(width)), timing(similar_timing()) {}

vi_status StoredRowsWalk::run(const DeviceIndex &ix, SearchContext &ctx, const StoredRows &rows, const ChunkBody &body,
                              const ChunkBody &landed) {
  SearchWorkspace &ws = ctx.ws;
  for (uint64_t q0 = 0; q0 < rows.nq; q0 += chunk_rows) {
    const uint64_t m = std::min(chunk_rows, rows.nq - q0);
    // the chunk's queries: stored rows -> ws.q, their slots, the records carrying each id
    const double t0 = timing ? now_ms() : 0.0;
    VI_TRY(ws.q.reserve(m * ix.dim));
    VI_TRY(ws.self_slot.reserve(m));
    if (rows.ids) {
      VI_TRY(ws.self_found.reserve(m));
      VI_TRY(resolve_records_by_id(ix, rows.ids + q0, m, rows.on_device, ws.self_found.p, ws.q.p, ws.self_slot.p));
    } else {
      VI_TRY(resolve_records_by_range(ix, rows.first + q0, m, ws.q.p, ws.self_slot.p));
    }
    VI_HIP(hipSetDevice(ix.device));
    double t1 = timing ? now_ms() : 0.0, t2 = t1;
    const RowChunk chunk{q0, m, rows.ids ? ws.self_found.p : nullptr, timing ? &t2 : nullptr};
    VI_TRY(body(chunk));
    // the next chunk's resolve writes ws.q and ws.self_slot from a stream of its own: this chunk's readers end first
    VI_HIP(hipStreamSynchronize(ctx.stream));
    ms_resolve += (float)(t1 - t0);
    ms_search += (float)(t2 - t1);
    if (landed) VI_TRY(landed(chunk));
  }
  return VI_OK;
}

SimilarTimes similar_last_times() { return g_last_times; }

vi_status device_index_range_similar(const DeviceIndex &ix, const RangeSimilarIO &io, RangeResult *out) {
  return stored_record_call(ix, g_last_times, [&](SearchContext &ctx) { return range_similar_in_context(ix, ctx, io, out); });
}

vi_status device_index_search_similar(const DeviceIndex &ix, const SimilarIO &io) {
  return stored_record_call(ix, g_last_times, [&](SearchContext &ctx) { return similar_in_context(ix, ctx, io); });
}

}  // namespace vi
