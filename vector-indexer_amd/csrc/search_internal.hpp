// search_internal.hpp — what the search engines' and the index builders' translation units (search.hip, search_kernels.hip,
// generic_search.hip, mfma_search.hip, grouping.hip, select.hip, range_select.hip, rank_images.hip, device_index.hip,
// list_build.hip, list_update.hip, kmeans.hip, similar_search.hip, cluster_radius.hip, probe_prune.hip) call in each other and share: declared once, here.  A search is one
// SearchBatch, built by the dispatcher (search.hip) and handed to the engine it chose; the engines hand it on to their
// stages.  (The probe grouping is called through a header of its own, grouping.hpp; mfma_search.hip launches its rank
// and select phases through rank_block.hpp, rank_stream.hpp and select.hpp.)
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <functional>

#include "device_index.hpp"
#include "list_layout.hpp"

namespace vi {

constexpr uint32_t kMaxMfmaDim = 1536;  // the MFMA engine's dimension limit (rank_wide_kernel above 128)
constexpr uint32_t kNarrowDim = 128;     // up to here the queries of a work item stay in registers (filter_kernel)

// ---- SearchWorkspace::stats: the engines' block of 64-bit device counters, by word ----
enum StatWord {
  // the grouping's counts (grouping.hip): reset by list_totals_kernel, written by group_prepare_kernel, read back by
  // group_probes.  With the scans inside list_totals_kernel (GroupScanArgs) its workgroups add to them instead:
  // split_queries_kernel has cleared them, and kStatTiles128, at the head of the search
  kStatScannedVectors = 0,  // sum over the lists of (queries probing it) x (its length)
  kStatItems = 1,           // scan / rank work items
  kStatSegRuns = 2,         // segment runs awaiting seg_merge_kernel (VALU engine)
  kStatTileBlocks = 3,      // (query group, block) tiles of the MFMA list phase
  kStatGroupRecords = 4,    // group records
  kStatRecordTiles = 5,     // record tiles (pair records: 2 x gq each)
  kStatListCounts = 6,      // ... words [0, 6): what list_totals_kernel resets (and kStatTiles128)
  // the selects' counters (VI_FILTER_STATS): cleared by the MFMA pipelines as [6, 12)
  kStatSelExact = 6,        // list select: vectors evaluated exactly; coarse select: single rows
  kStatSelScanned = 7,      // list select: groups scanned; coarse select: whole sub-blocks
  kStatSelQueriesFull = 8,  // queries with a full group
  kStatSelFullGroups = 9,
  kStatSelSubBlocks = 10,
  kStatSelectEnd = 12,
  kStatTiles128 = 12,       // the grouping again: tiles a grouping by 128 queries would have (the fill behind gq_hint)
  // batch flags: raised by split_queries_kernel, read back with the grouping's counts, reset by item_cols_kernel / item_push_kernel
  kStatQueryLo = 13,        // some query has a lo plane
  kStatQueryNotI8 = 14,     // some query is no int8 image
  kStatGroupingWords = 15,  // words [0, 15): what the host reads back after the grouping ...
  kStatGroupingLanding = 16,  // ... into a pinned buffer of this many
  // the streaming rank kernel's work counters: one per XCD queue, 128 bytes apart, reset by item_cols_kernel / item_push_kernel
  kStatRankWork = 16, kStatRankWorkStride = 16, kStatRankWorkCount = 8,
  // the selects' stage clocks (VI_FILTER_STATS)
  kStatClocks = 150, kStatClockCount = 8,
  kStatWords = 160          // size of the block
};
static_assert(kStatGroupingWords <= kStatGroupingLanding, "the landing buffer holds the grouping's counts");
static_assert(kStatRankWork + kStatRankWorkStride * kStatRankWorkCount <= kStatClocks && kStatClocks + kStatClockCount <= kStatWords,
              "the ranges of the counter block do not overlap");
using GroupingCounts = std::array<uint64_t, kStatGroupingWords>;  // host copy of words [0, kStatGroupingWords)

// ---- device_index.hip: the steps every route that builds a DeviceIndex takes ----
vi_status init_device_index(DeviceIndex *ix, int device, uint32_t dim, uint64_t nlists);
// Everything of an initialised index that follows from the layout of its lists, on ix->stream: lists.dq / nblocks,
// nvec_resident, the blocks and ext_ids (and timestamps, if asked for) reserved, list_first_block and list_len uploaded,
// list_shard and nshards from a host array (nshards = max + 1) or, if shard_from is given, from that index.  The copies
// are queued: `lay` and shard_host stay alive until the caller has synchronised ix->stream.
vi_status alloc_list_storage(DeviceIndex *ix, const ListLayout &lay, const uint32_t *shard_host, const DeviceIndex *shard_from,
                             bool with_timestamps);
// An initialised index that keeps the lists of `old` (unpartitioned) at new lengths full_len[l]: the layout planned (its
// two limits: VI_ERR_INVALID_INPUT), the coarse table and list_shard copied from `old` device to device, the list storage
// allocated (alloc_list_storage, with timestamps) and block_list_dev = the list of every new block.  Complete on return.
vi_status lay_out_from_old(DeviceIndex *ix, const DeviceIndex &old, const uint64_t *full_len, DevBuf<uint32_t> *block_list_dev);
// rows 0..n-1 of a row-major device matrix -> ceil(n / 64) lane-interleaved blocks, pad lanes zero; complete on return.
// ros_keep (optional): the row-of-slot scratch in a buffer of the caller's, kept from call to call.
vi_status repack_table(const float *rows_dev, uint64_t n, uint32_t dim, uint32_t dq, float *blocks, hipStream_t st,
                       DevBuf<uint32_t> *ros_keep = nullptr);
// the coarse table of an initialised index (centroids.dq / nblocks / blocks) from its nlists x dim rows on the device
vi_status coarse_table_from_rows(DeviceIndex *ix, const float *rows_dev);

// host array -> device buffer (grown to hold it), queued on st: `host` stays alive until st is synchronised
template <typename T>
vi_status upload(DevBuf<T> &buf, const T *host, size_t n, hipStream_t st) {
  VI_TRY(buf.reserve(std::max<size_t>(n, 1)));
  if (n) VI_HIP(hipMemcpyAsync(buf.p, host, n * sizeof(T), hipMemcpyHostToDevice, st));
  return VI_OK;
}

// ---- one search: what every stage of it works from ----
using SearchContext = DeviceIndex::SearchContext;
// one pruning call as it runs (probe_prune.hip): its rule, the kernel's two sums on their way back, its clock
struct PruneRun {
  const ProbePrune *rule = nullptr;
  bool host = false;        // the rule's arrays are host memory
  hipStream_t pending = nullptr;  // the stream whose copies into this object (and the rule's host array) are not known to have landed
  const uint64_t *totals = nullptr;  // the workspace's landing words: sum of real probes, sum of probes kept
  EventSpans<1> span;       // around probe_prune_kernel, under VI_PRUNE_TIMING
  ~PruneRun() { if (pending) (void)hipStreamSynchronize(pending); }  // (a call that failed behind the kernel: nothing lands later)
};
struct SearchBatch {
  const DeviceIndex &ix;
  SearchContext &ctx;      // leased for this call: workspace, stats, events and THE stream of this search
  const SlotFilter *flt;   // restricts the candidates of the list phase (the coarse step never sees it), or null
  const uint32_t *probes_in, *order_in;  // the caller's probe lists instead of a coarse step, or null
  EngineKnobs kn{};
  const float *Qd = nullptr;  // nq x dim on the device
  uint64_t nq = 0;
  uint32_t P = 0;          // n_probe clamped to the lists
  int timing = 0;          // DeviceIndex::timing for the engine chosen: 1 events at every phase boundary, 2 around the rank only
  // what this search has done so far: the coarse select filled ws.pair_rank; split_queries_kernel cleared the grouping's
  // counts of ws.stats; (MFMA engine) the event in front of the rank kernel is recorded; the grouping's scatter left the
  // streaming rank kernel's work items behind (item_push_kernel)
  bool pair_rank_valid = false, group_counts_cleared = false, rank_clock_started = false, items_pushed = false;
  PruneRun *prune = nullptr;  // adaptive probing: every engine prunes the rows of its coarse step (prune_staged_probes), or null
  SearchWorkspace &ws() const { return ctx.ws; }
  hipStream_t st() const { return ctx.stream; }
};
// device buffers of a top-k search's results: nq x k each; tie, slots and counts (nq) may be null
struct SelectOutputs { float *D; int64_t *I; uint64_t *tie, *slots; uint32_t *counts; };

// ---- search.hip: the dispatcher, for the callers that bring their own context (similar_search.hip) ----
// body(ctx) with a context of the index's pool held for its duration; the release publishes the context's stats as the
// handle's, under the pool's lock, however body ends
template <class Body>
vi_status with_search_context(const DeviceIndex &ix, Body body) {
  VI_HIP(hipSetDevice(ix.device));
  SearchContext *held = nullptr;  // (set before anything can release it)
  ContextLease lease(ix.search_contexts, make_context<SearchContext>, [&] { ix.last_stats = held->stats; });
  if (!lease.ctx) return VI_ERR_DEVICE;  // (the message is make_context's)
  held = lease.ctx;
  return body(*held);
}
// one top-k search in a context the caller holds: what device_index_search runs; synchronised on return
vi_status topk_search(const DeviceIndex &ix, SearchContext &ctx, const SearchIO &io);
// one radius search in a context the caller holds: what device_index_range_search runs; synchronised on return
vi_status radius_search(const DeviceIndex &ix, SearchContext &ctx, const RangeIO &io, RangeResult *out);
// V[r] (row-major, dim floats) = the stored vector of slots[r], zeros for ~0; queued on st
vi_status launch_gather_vectors(const DeviceIndex &ix, const uint64_t *slots, uint64_t nres, float *V, hipStream_t st);

// ---- search.hip: a radius search's result as the engines fill it, chunk of queries after chunk ----
// range_result_begin sizes lims; range_result_place reads the hit counts of queries [q0, q0 + m) back (it synchronises),
// extends lims by them on the host and the device and grows D / I / tie / slots to hold them, keeping what earlier chunks wrote
vi_status range_result_begin(const DeviceIndex &ix, uint64_t nq, RangeResult *res);
vi_status range_result_place(RangeResult *res, uint64_t q0, uint64_t m, const uint32_t *counts_dev, hipStream_t st);

// ---- similar_search.hip: the walk over stored records, for the three calls whose queries are records ----
// One chunk as its body sees it: rows [q0, q0 + m) are resolved — their vectors in ws.q, their slots in ws.self_slot —
// and `found` (device, [m]) counts the records carrying each row's id; null for a range.
struct RowChunk {
  uint64_t q0, m;
  const uint32_t *found;
  void mark_searched() const { if (searched_ms) *searched_ms = now_ms(); }  // the body's search ends here (ms_search)
  double *searched_ms;  // the walk's; null without timing
};
// Rows chunk_rows at a time (VI_GRAPH_CHUNK or 65 536, inside [1, what the dispatcher takes at rows `width` entries
// wide]) in ascending order through one search context.  run() resolves a chunk, hands it to `body` — its search, its
// consumer kernels and its copies, queued on ctx.stream — synchronises that stream and calls `landed` (optional), where
// the caller reads what its copies and events brought back.  timing: VI_SIMILAR_TIMING is set, not '0'.
using ChunkBody = std::function<vi_status(const RowChunk &)>;
struct StoredRowsWalk {
  explicit StoredRowsWalk(uint64_t width);
  const uint64_t chunk_rows;
  const bool timing;
  float ms_resolve = 0, ms_search = 0;  // over every run() of this walk
  vi_status run(const DeviceIndex &ix, SearchContext &ctx, const StoredRows &rows, const ChunkBody &body, const ChunkBody &landed = nullptr);
};
// What the three device_index_* entries of these calls are: `last` (the thread's report of the call) reset, an index
// without external ids rejected, body(ctx) under with_search_context, and no HIP error left behind by a failure.
template <class Report, class Body>
vi_status stored_record_call(const DeviceIndex &ix, Report &last, Body body) {
  last = Report{};
  if (!ix.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no external ids");
  const vi_status s = with_search_context(ix, body);
  if (s != VI_OK) (void)hipGetLastError();  // (a failed allocation is this call's failure, not the next call's)
  return s;
}

// ---- search_kernels.hip: the exact-order VALU engine ----
vi_status stage_coarse(SearchBatch &b);                   // ws.probes / gorder and the per-list histogram (ws.cnt)
vi_status adopt_probes(SearchBatch &b, bool histogram);   // ... from b.probes_in / order_in, validated
// what adopt_probes validates: rows [nq][P] of a caller (device) by validate_probes_kernel; synchronises st
vi_status validate_probe_rows(const DeviceIndex &ix, SearchWorkspace &ws, const uint32_t *probes, const uint32_t *order, uint64_t nq,
                              uint32_t P, hipStream_t st);
vi_status search_valu_pipeline(SearchBatch &b, uint64_t k, const SelectOutputs &out);

// ---- mfma_search.hip: the MFMA engine ----
vi_status search_mfma_pipeline(SearchBatch &b, uint64_t k, const SelectOutputs &out);
vi_status range_mfma_pipeline(SearchBatch &b, float radius2, RangeResult *res);
vi_status coarse_only_mfma(SearchBatch &b);
bool mfma_path_applicable(const DeviceIndex &ix, const EngineKnobs &kn, uint64_t k, uint32_t P);
bool coarse_on_matrix_cores(const DeviceIndex &ix, const EngineKnobs &kn, uint64_t nq, uint32_t P);

// ---- generic_search.hip: every candidate sorted ----
vi_status device_index_search_generic(SearchBatch &b, uint64_t k, const SelectOutputs &out);
vi_status device_index_range_generic(SearchBatch &b, float radius2, RangeResult *res);
vi_status generic_probe_export(SearchBatch &b);
vi_status sort_rows_u64(uint64_t *keys, uint64_t nrows, uint32_t logL, hipStream_t st);  // rows of 2^logL keys, each sorted ascending

// ---- probe_prune.hip: adaptive probing ----
// A search with a rule: prune_begin opens the run (this thread's PruneStats reset, the clock made), every engine calls
// prune_staged_probes behind its coarse step — ws.probes / ws.gorder pruned in place, the coarse step's per-list
// histogram counted again from the shortened rows if asked, the coarse select's pair ranks dropped; a batch without a
// run: nothing — and prune_finish, once the search's stream is synchronised, publishes the thread's PruneStats.
vi_status prune_begin(PruneRun &run, const ProbePrune *rule, bool host);
vi_status prune_staged_probes(SearchBatch &b, bool histogram);
void prune_finish(PruneRun &run);

// ---- rank_images.hip ----
// everything the MFMA engine ranks an index from, derived from its f32 blocks: norms, bf16 / int8 images, the centre, the
// margins' constants (the DeviceIndex fields from xnorm to c_len); called at the end of every index upload
vi_status prepare_rank_images(DeviceIndex *ix);

}  // namespace vi
