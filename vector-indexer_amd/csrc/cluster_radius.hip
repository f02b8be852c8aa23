// cluster_radius.hip — clustering the stored records by radius (vi_indexer_cluster_radius): connected components and
// DBSCAN labels of the index's own radius graph, one label per record in list order.
//
// The radius graph of an index is large (28 bytes per hit) and only the input of the job; the answer is 8 bytes per
// record.  So the graph is never kept: every pass walks rows [0, N) as the radius graph call does (StoredRowsWalk,
// search_internal.hpp) and radius_searches a chunk into ws.sim_range, with a consumer in place of find / place / move.
// The consumer reads the slots of a chunk's hits and nothing else, and the chunk's result is overwritten by the next
// chunk's.  Beside one chunk's result the call holds 12 bytes and one bit per slot.
//
// Passes over the graph (every pass searches every row again):
//   min_pts <= 1              one: every participant is core, cluster_link_kernel unites as it counts the degrees
//   min_pts >= 2              two: cluster_degree_kernel, the core bits, then cluster_link_kernel — whether a HIT is core
//                             is not known before its own row has been searched
//   neither labels nor count  one: cluster_degree_kernel alone
// Then cluster_label_kernel, a launch of its own: every hook of the link kernels is visible to it.
//
// Visibility inside cluster_link_kernel: the L2 of an XCD is not coherent with the others' and a CU's L1 is not
// refreshed by other CUs' stores, so every access to parent and border is an agent-scope relaxed atomic (AgentAccess);
// none is a plain load or store.  Correctness does not rest on freshness (cluster_rules.hpp): a stale parent word costs
// a failed CAS and a retry.  No lane waits for another lane, wave or workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "cluster_rules.hpp"
#include "device_index.hpp"
#include "list_layout.hpp"
#include "record_fetch.hpp"
#include "search_internal.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

struct AgentAccess {  // the link kernel's policy: relaxed, agent scope, never a plain access
  static __device__ __forceinline__ uint32_t load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void store(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ uint32_t cas(uint32_t *p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
  static __device__ __forceinline__ void min(uint32_t *p, uint32_t v) { (void)atomicMin(p, v); }
};

enum Counter : uint32_t { kCountCore = 0, kCountBorder, kCountRoots, kCountHits, kCounters };

__global__ void __launch_bounds__(256) cluster_init_kernel(uint32_t *parent, uint32_t *border, uint32_t *degree, uint32_t nslots) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= nslots) return;
  parent[s] = s;
  border[s] = kNoBorder;
  degree[s] = 0u;
}

// bit (block, lane) = the slot holds a participant (resident, and admitted where there is a filter) that is core
__global__ void __launch_bounds__(256) cluster_core_kernel(ResidentLists L, const uint64_t *allow, const uint32_t *degree,
                                                           uint32_t min_pts, uint64_t *core) {
  for_each_resident_block(L, [&](uint32_t block, uint32_t lane, bool resident, uint32_t, uint32_t) {
    const bool part = resident && (!allow || ((allow[block] >> lane) & 1ull));
    const uint64_t word = __ballot(part && cluster_is_core(degree[block * 64u + lane], min_pts));
    if (lane == 0) core[block] = word;
  });
}

struct LinkArgs {
  const uint64_t *lims;       // [m + 1] the chunk's search result
  const uint64_t *slots;      // the slot of every hit
  const uint32_t *self_slot;  // [m] the slot of each row's record
  const uint64_t *allow;      // the filter's allow bits, or null: every resident record takes part
  const uint64_t *core;       // [nblocks] (link only) as cluster_core_kernel left it: not written while a link kernel runs
  uint32_t *parent, *border;  // [nslots] (link only)
  uint32_t *degree;           // [nslots] or null: written at the row's slot
  uint32_t m, nslots;
};

// One wave per row, four rows per workgroup; lanes stride the row's entries.  The row of a record that does not take
// part is skipped whole (its degree stays 0).  The one entry that is the row's own record is neither counted nor linked.
template <bool LINK>
__device__ __forceinline__ void cluster_row(const LinkArgs &a) {
  const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (row >= a.m) return;  // (wave-uniform)
  const uint32_t self = a.self_slot[row];
  if (self >= a.nslots) return;
  if (a.allow && !((a.allow[self >> 6] >> (self & 63u)) & 1ull)) return;
  const uint64_t in0 = a.lims[row];
  const uint32_t len = (uint32_t)(a.lims[row + 1] - in0);  // (a chunk holds fewer than 2^31 entries)
  const bool self_core = LINK && ((a.core[self >> 6] >> (self & 63u)) & 1ull);
  uint32_t n = 0;
  for (uint32_t j0 = 0; j0 < len; j0 += 64u) {  // (wave-uniform bounds: the ballot sees all 64 lanes)
    const uint32_t j = j0 + lane;
    const uint32_t b = j < len ? (uint32_t)a.slots[in0 + j] : self;
    const bool other = b != self && b < a.nslots;
    n += (uint32_t)__popcll(__ballot(other));
    if (LINK && other) cluster_link<AgentAccess>(a.parent, a.border, self, self_core, b, (a.core[b >> 6] >> (b & 63u)) & 1ull);
  }
  if (a.degree && lane == 0) a.degree[self] = n;
}

__global__ void __launch_bounds__(256) cluster_degree_kernel(LinkArgs a) { cluster_row<false>(a); }
__global__ void __launch_bounds__(256) cluster_link_kernel(LinkArgs a) { cluster_row<true>(a); }

struct LabelArgs {
  ResidentLists L;
  const uint64_t *prefix;     // [nlists] records before each list in list order (ensure_fetch_layout)
  const uint64_t *core;
  const uint32_t *parent, *border, *degree;
  int64_t *labels;            // [N] in list order, or null
  uint32_t *degree_out;       // [N] in list order, or null
  unsigned long long *count;  // [kCounters]
  uint32_t link;              // parent / border / core hold a clustering (else only the degrees are delivered)
};

// slot -> list-order ordinal, as the export numbers its rows
__device__ __forceinline__ uint64_t ordinal_of(const LabelArgs &a, uint32_t slot) {
  const uint32_t blk = slot >> 6, l = list_of_block(a.L.first_block, a.L.nlists, blk);
  return a.prefix[l] + (uint64_t)(blk - a.L.first_block[l]) * 64u + (slot & 63u);
}

// One wave per block of 64 slots; every resident slot writes its label and degree at its own ordinal.  Pad slots write
// nothing: they have no ordinal.  The counts go out with one atomic per wave and counter.
__global__ void __launch_bounds__(256) cluster_label_kernel(LabelArgs a) {
  for_each_resident_block(a.L, [&](uint32_t block, uint32_t lane, bool resident, uint32_t l, uint32_t b) {
    const uint32_t s = block * 64u + lane;
    const uint64_t ord = a.prefix[l] + (uint64_t)b * 64u + lane;
    const bool core = a.link && ((a.core[block] >> lane) & 1ull);
    uint32_t rep = kNoBorder, deg = 0;
    if (resident) {
      deg = a.degree[s];
      if (a.link) rep = cluster_label_slot<AgentAccess>(a.parent, a.border, s, core);
      if (a.labels) a.labels[ord] = rep == kNoBorder ? kLabelNoise : (int64_t)ordinal_of(a, rep);
      if (a.degree_out) a.degree_out[ord] = deg;
    }
    const uint32_t n_core = (uint32_t)__popcll(__ballot(resident && core));
    const uint32_t n_border = (uint32_t)__popcll(__ballot(resident && !core && rep != kNoBorder));
    const uint32_t n_roots = (uint32_t)__popcll(__ballot(resident && core && rep == s));
    unsigned long long hits = deg;
    for (uint32_t off = 32u; off; off >>= 1) hits += __shfl_down(hits, off, 64);
    if (lane == 0) {
      if (n_core) atomicAdd(a.count + kCountCore, (unsigned long long)n_core);
      if (n_border) atomicAdd(a.count + kCountBorder, (unsigned long long)n_border);
      if (n_roots) atomicAdd(a.count + kCountRoots, (unsigned long long)n_roots);
      if (hits) atomicAdd(a.count + kCountHits, hits);
    }
  });
}

thread_local vi_cluster_stats g_last_stats{};

vi_status cluster_in_context(const DeviceIndex &ix, SearchContext &ctx, const ClusterIO &io) {
  SearchWorkspace &ws = ctx.ws;
  hipStream_t st = ctx.stream;
  const uint64_t N = ix.nvec_resident, nblocks = ix.lists.nblocks, nslots = nblocks * 64;
  StoredRowsWalk walk(64);
  const bool link = io.labels || io.n_clusters;
  const bool two = link && io.min_pts >= 2;
  vi_cluster_stats cs{};
  cs.rows = N; cs.chunk_rows = walk.chunk_rows; cs.passes = two ? 2 : 1;
  if (N == 0 || nblocks == 0) {  // nothing is resident: no label to write
    if (io.n_clusters) *io.n_clusters = 0;
    g_last_stats = cs;
    return VI_OK;
  }
  enum { kSpanLink, kSpanLabel };  // around the degree / link kernel of a chunk; around the label kernel
  EventSpans<2> spans;
  VI_TRY(spans.create(walk.timing));
  VI_TRY(ensure_fetch_layout(ix, st));
  VI_HIP(hipSetDevice(ix.device));

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

  RangeIO rio;
  rio.on_device = true; rio.n_probe = io.n_probe; rio.radius2 = io.radius2; rio.filter = io.filter;
  RangeResult &in = ws.sim_range;
  StoredRows all;  // every resident record, in list order
  all.nq = N;
  for (uint32_t pass = 0; pass < cs.passes; ++pass) {
    const bool linking = link && pass + 1 == cs.passes;
    if (linking) {  // the core bits: from the degrees of the pass before, or (min_pts <= 1) every participant
      hipLaunchKernelGGL(cluster_core_kernel, slot_walk_grid((uint32_t)ix.nlists), dim3(256), 0, st, L, allow, degree.p, io.min_pts, core.p);
      VI_HIP(hipGetLastError());
    }
    const auto body = [&](const RowChunk &c) -> vi_status {
      // ---- the radius search of the chunk, into the context's own result ----
      rio.queries = ws.q.p; rio.nq = c.m;
      VI_TRY(radius_search(ix, ctx, rio, &in));  // (synchronised)
      c.mark_searched();
      // ---- the chunk's entries are consumed; nothing of them is kept ----
      // a pass that links in one go counts the degrees as well; the link pass of two leaves them as the first made them
      LinkArgs la{in.lims.p, in.slots.p, ws.self_slot.p, allow, core.p, parent.p, border.p,
                  linking && two ? nullptr : degree.p, (uint32_t)c.m, (uint32_t)nslots};
      const dim3 grid((uint32_t)((c.m + 3) / 4)), block(256);
      VI_TRY(spans.begin(kSpanLink, st));
      if (linking) hipLaunchKernelGGL(cluster_link_kernel, grid, block, 0, st, la);
      else hipLaunchKernelGGL(cluster_degree_kernel, grid, block, 0, st, la);
      VI_HIP(hipGetLastError());
      VI_TRY(spans.end(kSpanLink, st));
      // a row's bounds, slot and allow word, its degree, and the slot of every entry (parent / border / core words: by need)
      cs.link_bytes += c.m * 32 + in.total * 8;
      return VI_OK;
    };
    const auto landed = [&](const RowChunk &) -> vi_status { cs.ms_link += spans.ms(kSpanLink); return VI_OK; };
    VI_TRY(walk.run(ix, ctx, all, body, landed));
  }
  cs.ms_resolve = walk.ms_resolve; cs.ms_search = walk.ms_search;
  // ---- labels, degrees and counts, in a launch of its own ----
  LabelArgs ga{L, ix.fetch.prefix.p, core.p, parent.p, border.p, degree.p, labels, degree_out, count.p, link ? 1u : 0u};
  VI_TRY(spans.begin(kSpanLabel, st));
  hipLaunchKernelGGL(cluster_label_kernel, slot_walk_grid((uint32_t)ix.nlists), dim3(256), 0, st, ga);
  VI_HIP(hipGetLastError());
  VI_TRY(spans.end(kSpanLabel, st));
  unsigned long long h_count[kCounters] = {};
  VI_HIP(hipMemcpyAsync(h_count, count.p, sizeof(h_count), hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  if (!io.on_device) {  // everything has succeeded: the caller's arrays are written now
    if (io.labels) VI_HIP(hipMemcpyAsync(io.labels, labels, N * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (io.degree) VI_HIP(hipMemcpyAsync(io.degree, degree_out, N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
  }
  cs.ms_label = spans.ms(kSpanLabel);
  const uint64_t participants = io.filter ? io.filter->num_allowed : N;
  cs.hits = h_count[kCountHits];
  if (link) {
    cs.n_core = h_count[kCountCore];
    cs.n_border = h_count[kCountBorder];
    cs.n_clusters = h_count[kCountRoots];
    cs.n_noise = participants - cs.n_core - cs.n_border;
  }
  if (io.n_clusters) *io.n_clusters = cs.n_clusters;
  g_last_stats = cs;
  return VI_OK;
}

}  // namespace

vi_cluster_stats cluster_last_stats() { return g_last_stats; }

vi_status device_index_cluster_radius(const DeviceIndex &ix, const ClusterIO &io) {
  return stored_record_call(ix, g_last_stats, [&](SearchContext &ctx) { return cluster_in_context(ix, ctx, io); });
}

}  // namespace vi
