// device_index.hpp — HBM-resident IVF index and the search pipeline entry points.
//
// HBM layout ("lane-interleaved blocks").  Every vector set that gets scanned — the coarse
// centroid table and each inverted list — is stored in blocks of 64 vectors:
//
//     block[b] : float4 [dq][64]          dq = 4*ceil(dim/16) quads, zero padded
//     element (qd, lane).{x,y,z,w} = dims 4*qd .. 4*qd+3 of vector (64*b + lane)
//
// so that a wave64 reading quad qd of a block issues ONE global_load_dwordx4 covering a
// contiguous, 1 KiB-aligned span: lane = vector, registers = consecutive dimensions.  That
// makes the reference's strictly sequential f32 sum over d (src/utils.rs:28-30) a per-lane
// register chain with perfectly coalesced loads, and lets one loaded quad be reused by a
// whole group of queries from registers.  Lists are padded to whole blocks (pad lanes carry
// zeros and are masked by the list length).  External ids live in a parallel u64 array
// indexed by slot = 64*block + lane.  The AoS record layout of the shard files
// (24 B meta + 4·D B + pad, shards.rs:106-114) is kept only on disk.
#pragma once
#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "context_pool.hpp"
#include "rebalance_rules.hpp"
#include "shards.hpp"

namespace vi {

struct SlotFilter;  // slot_filter.hpp

constexpr uint32_t kNoPos = 0xFFFFFFFFu;   // empty slot marker in a sorted run
constexpr uint32_t kMaxSelect = 64;        // wave-resident top-k width of the fast path

struct BlockSet {               // a set of lists stored as lane-interleaved blocks
  DevBuf<float> blocks;         // [nblocks][dq][64][4]
  uint32_t dq = 0;
  uint64_t nblocks = 0;
};

struct DeviceIndex;

// Result of a radius search (device_index_range_search): CSR like Faiss's RangeSearchResult — query q owns entries
// [lims[q], lims[q + 1]) of D / I / tie / slots, sorted as the reference's stable candidate sort leaves them.  Owns its
// device buffers; outlives later searches of its index, not the index.
struct RangeResult {
  const DeviceIndex *ix = nullptr;  // the index searched (vi_range_result_copy gathers stored vectors from it); null: a
                                    // merged result (range_merge_device), which belongs to no index and has no slots
  int device = 0;                   // where the buffers live
  uint64_t nq = 0, total = 0;
  std::vector<uint64_t> h_lims;     // host copy of lims: nq + 1
  DevBuf<uint64_t> lims;            // nq + 1
  DevBuf<float> D;                  // `total` entries each, in buffers of `cap`
  DevBuf<int64_t> I;
  DevBuf<uint64_t> tie, slots;      // tie key (candidate-order rank << 32 | list position); global slot of the stored vector
  uint64_t cap = 0;
};

struct SearchWorkspace {
  DevBuf<float> q;              // queries on device (nq x dim) when the caller passed host memory
  DevBuf<float> crun_dist;      // coarse partial runs [nq][S][P]
  DevBuf<uint32_t> crun_pos;
  DevBuf<uint32_t> probes;      // [nq][P] list ids in probe-rank order
  DevBuf<uint32_t> gorder;      // [nq][P] candidate-order rank of each probe (shard visiting order)
  DevBuf<uint32_t> probe_flag;  // validation result of caller-supplied probe lists
  // adaptive probing (probe_prune.hip): real and kept probes per query [2][nq], their two sums and the page-locked words
  // the sums land in; a host caller's per-query counts in, kept counts out
  DevBuf<uint32_t> prune_counts;
  DevBuf<uint64_t> prune_totals;
  uint64_t *prune_pinned = nullptr;
  DevBuf<uint32_t> prune_limit, prune_kept;
  DevBuf<uint32_t> cnt;         // [nlists] (#queries probing list) ; cursor = second half
  DevBuf<uint32_t> list_tot;    // [nlists] queries probing each list
  DevBuf<uint32_t> seg_start;   // [nlists+1]
  DevBuf<uint32_t> item_start;  // [nlists+1]
  DevBuf<uint32_t> segrun_start;  // [nlists+1]
  // the scans inside list_totals_kernel (grouping.hip: GroupScanArgs) instead of the three arrays above: per list (pairs; items, segment
  // runs, record tiles before it within its 64 lists), per 64 lists their sums; item_push_kernel adds the two up
  DevBuf<uint32_t> list_local, list_block_sums;  // [nlists] x 4, [kGroupScanBlocks] x 4
  DevBuf<float> seg_run_dist;  // segment runs of long lists, merged by seg_merge_kernel
  DevBuf<uint32_t> seg_run_pos;
  DevBuf<uint32_t> pairs;       // [nq*P] slot ids grouped by list
  DevBuf<float> run_dist;       // [nq*P][K]
  DevBuf<uint32_t> run_pos;
  DevBuf<float> D;              // outputs when the caller wants host results
  DevBuf<int64_t> I;
  DevBuf<uint64_t> tie;
  DevBuf<uint64_t> slots;       // [nq][k] global slot of each result (include_vectors gather)
  DevBuf<uint32_t> counts;      // [nq]
  DevBuf<uint64_t> stats;       // device-side counters (layout: StatWord, search_internal.hpp)
  DevBuf<float> V;
  // MFMA engine (mfma_search.hip)
  DevBuf<uint32_t> c_seg, c_item, c_pairs;  // the coarse table grouped as one list ...
  uint64_t c_nq = 0;                        // ... for this batch size
  DevBuf<uint32_t> pair_rel, qtot, qoff;    // group-record offsets: per (query, probe), per query, scan over queries
  DevBuf<uint32_t> pair_rank;               // a pair's place among the pairs of its (list, sub-bin): from the direct coarse select
  DevBuf<uint32_t> item_list;               // list of each rank work item
  DevBuf<uint32_t> items;                   // ... or its whole descriptor (8 words), item_desc_kernel (grouping.hip)
  DevBuf<uint64_t> prof;                    // diagnostic counters (VI_STREAM_PROF)
  DevBuf<uint32_t> item_qcol, item_grec, item_sdesc;    // streaming rank kernel: per (item, column) the query / its group record (grouping.hip: item_cols_kernel, item_push_kernel)
  DevBuf<uint32_t> tile_start, pair_pos;    // pair records: first record tile of each list; position of a (query, probe) pair in its list
  DevBuf<float> gval;                       // group records: 4 smallest sub-block minima per (query, probe, segment, lane half)
  DevBuf<uint32_t> gpos;                    // ... and where each record belongs (probe rank | segment | lane half)
  DevBuf<uint32_t> qimg;                    // wide vectors: query-major bf16 hi/lo image of the batch
  DevBuf<uint32_t> qimg8;                   // int8 image of the batch (q - 127), when the lists have one (split_queries_kernel)
  DevBuf<float> brec;                       // pair records: the 4 sub-block minima of two blocks per (record tile, lane half, query of the group)
  struct GqHint { uint64_t nq; uint32_t P, gq; };
  std::vector<GqHint> gq_hint;              // queries per rank work item measured to suit a batch shape (mfma_search.hip)
  uint64_t *hstats_pinned = nullptr;        // page-locked landing buffer of the grouping's counts (kStatGroupingLanding words)
  bool stats_zeroed = false;                // the batch flags of ws.stats start at zero (StatWord, search_internal.hpp)
  bool queries_hi_only = false;             // the previous batch's -2 q were all bf16-exact (no lo plane)
  DevBuf<uint64_t> sort_keys, order_keys, total;
  DevBuf<uint64_t> total_allowed;           // generic engine with a filter: candidates per query that received a key
  DevBuf<uint32_t> gprobe, off_by_g, off_by_rank;
  DevBuf<uint32_t> range_bound;             // radius search: per query an upper bound of its hits (+ one flag word)
  // the walk over stored records (similar_search.hip: StoredRowsWalk), per chunk of rows: their vectors in q above, the
  // slot of each row's record and the number of records carrying its id — reserved and filled by the walk, read by the
  // chunk bodies of its three callers
  DevBuf<uint32_t> self_slot, self_found;
  // search by stored record: the k-wide rows of a host caller (its k + 1-wide search rows are D / I / tie / slots above)
  DevBuf<float> sim_D;
  DevBuf<int64_t> sim_I;
  DevBuf<uint64_t> sim_slots;
  // its radius form: the chunk's search result before the drop (kept: range_result_place reuses its capacity from chunk
  // to chunk and call to call) and the output length of every row; range_find_kernel leaves in self_slot the position
  // of each row's own entry
  RangeResult sim_range;
  DevBuf<uint32_t> sim_len;
};

// ---- reading records back (record_fetch.hip) ----
// A get or an export holds one FetchContext of the handle's pool (context_pool.hpp) for the duration of the call: its
// stream and events, the id table of a get and the staging of host outputs, all grow-only.
struct FetchContext : StreamEvents<5> {
  IdSetBuffers ids;                    // the requested ids; its flags carry two more words, one u64: requests that found a record
  DevBuf<uint32_t> first_slot, count;  // [capacity + 1] values beside the keys: lowest slot that carries the key, records that do
  DevBuf<uint32_t> out_count;          // host outputs are produced here and copied back
  DevBuf<float> out_values;
  DevBuf<uint64_t> out_ids, out_ts, out_where;
};
struct FetchState {
  ContextPool<FetchContext, 4> pool;
  vi_fetch_stats last{};  // of the most recent get or export that succeeded on this handle (under the pool's lock)
  // the layout of the (immutable) index, read back by the first export: first block, length and the exclusive prefix
  // of the lengths (= list-order ordinal of a list's first record), on the host and the prefix on the device too
  std::mutex layout_mu;  // guards the making of the five below; they are read freely once layout_ready was seen under it
  bool layout_ready = false;
  std::vector<uint32_t> h_first, h_len;
  std::vector<uint64_t> h_prefix;  // [nlists + 1]
  DevBuf<uint64_t> prefix;         // [nlists]
};

inline uint64_t next_index_serial() {
  static std::atomic<uint64_t> n{0};
  return ++n;
}

struct DeviceIndex {
  const uint64_t serial = next_index_serial();  // never reused in a process: what a SlotFilter names its index by
  int device = 0;
  int order = VI_ORDER_SCALAR;  // summation order of every distance this index computes
  uint32_t dim = 0, dq = 0;
  uint64_t nlists = 0;          // k' (non-empty centroids of the index)
  uint64_t nvec_resident = 0;   // vectors whose lists are resident on this GPU
  uint64_t nshards = 0;
  BlockSet centroids;           // the coarse table as one list of k' vectors
  BlockSet lists;               // all resident inverted lists back to back
  DevBuf<uint32_t> list_first_block;  // [nlists]
  DevBuf<uint32_t> list_len;          // [nlists]  (0 => not resident here / empty)
  DevBuf<uint32_t> list_shard;        // [nlists]
  DevBuf<uint64_t> ext_ids;           // [lists.nblocks*64]
  DevBuf<uint64_t> timestamps;        // [lists.nblocks*64] stored timestamp per slot (pad slots 0, never read); null on the
                                      // k-means hierarchy's indexes (device_index_from_rows)
  uint32_t stripe_rank = 0, stripe_world = 1;  // multi-GPU: block b of a list lives on rank b % world
  DevBuf<float> xnorm;                // [lists.nblocks*64] squared norm per slot (3e38 on pad slots)
  DevBuf<float> xnorm_img, cent_xnorm_img;  // the same in the column order of the bf16 images (slot_filter.hpp: image_column)
  DevBuf<uint32_t> lists_bf16, cent_bf16;  // bf16 hi/lo images of the blocks for the MFMA ranking (rank_images.hip)
  DevBuf<uint32_t> lists_u8_nat;           // 8-bit descriptors (integers 0..255): one byte per dimension, same order (exact re-evaluation)
  DevBuf<uint32_t> lists_hi_nat;           // bf16-exact lists: their hi plane in the blocks' own vector order (exact re-evaluation)
  // 8-bit descriptors, D <= 128: int8 image 127 - v of the lists (block and column order of the bf16 image), h(v) =
  // ceil(|v - 127|^2 / 2) in image-column order, the frame's centre (dim x 127.0f) and max |v - 127|^2 (rank_stream_i8_kernel)
  DevBuf<uint32_t> lists_i8;
  DevBuf<int> i8_norm_img;
  DevBuf<float> i8_centre;
  float i8_xmax2 = 0.0f;
  bool lists_lo_zero = false, cent_lo_zero = false;  // every stored value is bf16-exact (lo planes all zero)
  // sampled means over the stored vectors: ||v - centroid of its list||^2 and ||v||^2 (what the ranking arithmetic of
  // real-valued lists is chosen by: mfma_search.hip, rank_approx_mode)
  float mean_spread = 0.0f, mean_norm2 = 0.0f;
  float rho2_max = 0.0f;  // max |x - hi(x)|^2 over the stored vectors (x = v - mu when centred): the hi-plane ranking's margin
  // Real-valued lists far from the origin (SIFT-like values with noise, embeddings with a common offset): the bf16 images
  // are taken about the mean mu of the stored vectors — ||q - v|| does not change, the norms the rank margins scale with
  // shrink to the spread of the data.  Only the ranking sees mu; the exact evaluation reads the stored f32 values.
  bool centered = false;
  DevBuf<float> centre;  // mu: dq * 4 floats (zero beyond dim)
  float mean_norm2_c = 0.0f, xmax2_c = 0.0f, cent_xmax2_c = 0.0f;  // ... and the norms about mu
  float xmax2 = 0.0f;                 // max squared norm of a stored vector (MFMA engine's rank margin)
  DevBuf<float> cent_xnorm;           // same for the coarse table
  DevBuf<float> cent_rows;            // the coarse table row-major (coarse select: single-row exact re-evaluation)
  float cent_xmax2 = 0.0f;
  DevBuf<uint32_t> c_first, c_len;    // the coarse table described as one list
  hipStream_t stream = nullptr;       // uploads and index construction
  // Searches: the reference's search is &self and runs concurrently from several OS threads
  // (tests/ivf_index_tests.rs:768-807).  A search holds one SearchContext of the pool (context_pool.hpp) — its own
  // stream, events, workspace — for the duration of the call: up to four calls run at once on one handle.  The call's
  // SearchBatch (search_internal.hpp) carries it to every stage; what is in it outlives the search (grow-only buffers, gq_hint, ...).
  struct SearchContext : StreamEvents<6> {
    SearchWorkspace ws;
    vi_search_stats stats{};
    ~SearchContext() {
      if (ws.hstats_pinned) (void)hipHostFree(ws.hstats_pinned);
      if (ws.prune_pinned) (void)hipHostFree(ws.prune_pinned);
    }
  };
  mutable ContextPool<SearchContext, 4> search_contexts;
  mutable vi_search_stats last_stats{};  // of the most recent search that finished on this handle (under the pool's lock)
  int timing = 0;  // 0 off, 1 HIP events at every phase boundary, 2 around the list-rank kernel only
  mutable FetchState fetch;  // gets and exports: const on the index, like searches

  ~DeviceIndex();
};

// ---- the five routes to a resident index ----
// Each lays its lists out by list_layout.hpp, reserves and uploads through alloc_list_storage, builds (or copies) the
// coarse table and ends with prepare_rank_images (search_internal.hpp, device_index.hip); what differs is where the list
// blocks come from.  The last two start from an older index and share their frame and the vocabulary of their block
// kernels (list_blocks.hpp: refuse_update, begin_update, launch_block_kernel, copy_old_block, fill_block_column).  Who calls which, and
// in what order with the files, is index_lifecycle.cpp:
//   device_index_load        (device_index.hip)  records of the shard files, in stripes or by shard placement: a load, and
//                                                the build of a rank of a multi-GPU run (index_lifecycle.cpp: attach_device)
//   device_index_from_rows   (device_index.hip)  rows of a device matrix, grouped on the host: the two-level hierarchy of
//                                                the k-means assignment (kmeans.hip)
//   device_index_from_order  (list_build.hip)    rows of a device matrix, grouped on the device: a single-GPU build (index_lifecycle.cpp: fit_and_save)
//   device_index_update      (list_update.hip)   the blocks of an older index, less the records a filter excludes and / or
//                                                with new rows behind them: vi_indexer_add_records, vi_indexer_retain /
//                                                vi_indexer_remove_ids, vi_indexer_upsert_records (index_lifecycle.cpp: update_records)
//
// Upload: centroid table + this rank's part of the lists, repacked on the GPU.  placement 0: a stripe of every list
// (block b on rank b % world); 1: the whole lists of the shard files dealt to this rank (greedy by bytes).
vi_status device_index_load(const IndexMeta &meta, const std::string &shards_dir, int device, int rank,
                            int world, int placement, DeviceIndex *out);
// owner rank of every shard under placement 1: shards by descending bytes, each to the least loaded rank so far
std::vector<uint32_t> shard_owners(const std::vector<uint64_t> &shard_bytes, uint32_t world);
// Build a device index from device-resident arrays (the k-means path, where the "index" is the two-level centroid
// hierarchy of assign_points_hierarchical, kmeans.rs:474-581).  table: ntable x dim row-major (device) = coarse table;
// rows: row-major device matrix the lists draw from; list_off[nlists+1] (host) delimits
// member_rows (host, row index per list member, list order = scan order); ids (device,
// optional) = external id per row (null => row index); list_shard (host, optional).  No timestamps are kept.
vi_status device_index_from_rows(int device, int order, uint32_t dim, const float *table_dev, uint64_t ntable,
                                 const float *rows_dev, const std::vector<uint64_t> &list_off,
                                 const std::vector<uint32_t> &member_rows, const uint64_t *ids_dev,
                                 const std::vector<uint32_t> *list_shard, DeviceIndex *out);
// resident index straight from device data: list l = rows order[src_off[l] .. + len[l]) of X_dev; ts_dev (optional) =
// timestamp per row, 0 or no array => now (what shard_export_device writes)
vi_status device_index_from_order(int device, uint32_t dim, const float *table_host, uint64_t nlists, const float *X_dev,
                                  const uint32_t *order_dev, const std::vector<uint64_t> &src_off,
                                  const std::vector<uint32_t> &len, const std::vector<uint32_t> &list_shard,
                                  const uint64_t *ids_dev, const uint64_t *ts_dev, uint64_t now, DeviceIndex *out);
// `out` = a fresh index holding, list by list, the records of `old` (unpartitioned; only read) that stay, closed up in
// their old order, followed by the rows the list receives.  Both halves are optional:
//   keep (a filter of `old`, or null): the records whose allow bit is 1 stay.  Null: all stay, nothing is counted or read
//     back, and the lengths come from old_len_host (a host copy of old's list_len; not read where keep is given).
//   n rows (or 0): list l receives rows order_dev[seg[l] .. seg[l + 1]) of rows_dev (seg on the device and the host:
//     group_ids_by_label_device); row_ext_dev / row_ts_dev: external id and stored timestamp of every row.  n == 0: none
//     of the six row arguments is read.
// A list may keep nothing and receive rows, or keep nothing and receive none (it stays as an empty list).  Old blocks are
// copied or gathered device to device, nothing comes from the shard files; old and new index coexist until the caller
// drops the old one.  ms_kernel / kernel_bytes (optional): HIP-event time of update_blocks_kernel and the bytes it moves.
vi_status device_index_update(const DeviceIndex &old, const SlotFilter *keep, const float *rows_dev, uint64_t n,
                              const uint32_t *order_dev, const uint32_t *seg_dev, const std::vector<uint64_t> &seg_host,
                              const uint64_t *row_ext_dev, const uint64_t *row_ts_dev, const std::vector<uint32_t> &old_len_host,
                              DeviceIndex *out, float *ms_kernel, uint64_t *kernel_bytes);
//   device_index_refine      (list_refine.hip)   the blocks of an older index, every record re-homed to the list of its
//                                                nearest centre after `iters` Lloyd iterations warm-started from the
//                                                old table: vi_indexer_refine (index_lifecycle.cpp: refine_records)
// What a refine hands back beside the index: the new table (nlists x dim, host), the lengths before and after, the counts
// of the contract (include/vi_amd.h: vi_refine_stats), the host clock of the phases and the HIP-event time and bytes of
// list_means_kernel (summed over the iterations) and rehome_blocks_kernel.
struct RefineResult {
  std::vector<float> table;
  std::vector<uint32_t> old_len, new_len;
  uint64_t iterations_run = 0, moved = 0, lists_emptied = 0, means_bytes = 0, rehome_bytes = 0;
  float ms_means = 0, ms_label = 0, ms_rehome = 0, ms_images = 0, ms_means_kernel = 0, ms_rehome_kernel = 0;
};
// The members of the lists of a resident index as a refine's kernels take them: list l's own records in their own order
// (cur == nullptr; seg is not read), or the list-order ordinals cur[seg[l] .. seg[l + 1]) (refine_rules.hpp).
struct ListMembers {
  const float4 *blocks;
  uint32_t dq, dim, nlists;
  const uint32_t *first_block, *old_len;   // per list
  const uint64_t *prefix;                  // per list: ordinal of its first record
  const uint32_t *cur, *seg;
};
// The split step a rebalance adds to the first split_rounds iterations of a refine (include/vi_amd.h: vi_rebalance_rule),
// and what it counts: the fields of vi_rebalance_stats, ms_kernels in HIP-event time, ms in wall time.
struct SplitRule {
  uint64_t split_rounds = 0;
  double split_factor = 2.0;
  uint64_t receiver_max_len = 0, max_splits = 0;
  uint32_t split_iters = 4;
};
struct SplitStats {
  uint64_t pairs_planned = 0, splits_done = 0, splits_skipped = 0, inner_iterations = 0, split_bytes = 0;
  float ms = 0, ms_kernels = 0;
};
// `out` = a fresh index holding the records of `old` (unpartitioned, at least one record; only read) in the lists that
// `iters` >= 1 iterations leave them in; table_host: old's coarse table, nlists x dim.  One iteration: every list with a
// record gets the mean of its records as its centre (one sequential f32 chain per column in list order, then one divide;
// an empty list keeps its centroid bits), every record the label of the first probe of the coarse step on the new table,
// every list the records of its label in their previous order.  Stops early after an iteration that moved nothing and
// changed no word of the table.  The old blocks are read until the end and never written; complete on return.
// rule (optional; with it, split: what the split steps counted): the first rule->split_rounds iterations carry the split
// step of a rebalance between centres and labels.  Without it no launch and no byte differs from a plain refine.
vi_status device_index_refine(const DeviceIndex &old, const float *table_host, uint64_t iters, DeviceIndex *out, RefineResult *res,
                              const SplitRule *rule = nullptr, SplitStats *split = nullptr);
//   device_split_lists       (list_split.hip)    the split step of vi_indexer_rebalance for the pairs of one iteration:
//                                                table_host (nlists x dim, the centres of step 1) gets ca in the donor's
//                                                row and cb in the receiver's row of every pair that was not skipped.
//                                                len_host: the lengths the plan was made from.  Synchronises `st`.
vi_status device_split_lists(const ListMembers &m, const std::vector<RebalancePair> &pairs, const uint64_t *len_host, uint32_t split_iters,
                             float *table_host, hipStream_t st, SplitStats *stats);

// ---- adaptive probing (probe_prune.hip, probe_rules.hpp): per-query probe counts between coarse step and list phase ----
// A search's rule (vi_probe_rule) and where the number of probes each query kept goes.  The two arrays are host memory on
// a search with host queries, device memory otherwise.
struct ProbePrune {
  uint32_t min_probe = 0;
  float ratio2 = 0.0f;
  uint64_t max_codes = 0;
  const uint32_t *n_probe_q = nullptr;  // nq counts, optional
  uint32_t *n_kept = nullptr;           // nq, optional
};
// probe rows [nq][P] of a coarse step (device), pruned in place over the queries they belong to; the rows are validated as
// a list phase validates them.  Synchronised on return.
vi_status device_index_prune_probes(const DeviceIndex &ix, const float *queries_dev, uint64_t nq, uint32_t P, uint32_t *probes_dev,
                                    uint32_t *order_dev, const ProbePrune &rule);
// of this thread's last pruning call (device_index_prune_probes, or a search with SearchIO::prune): real probes in, probes
// kept, and under VI_PRUNE_TIMING (set, not '0') the HIP-event time of probe_prune_kernel; zeros after a call that failed
// or pruned nothing (no query, an empty index): the entries of the C ABI reset them first (prune_reset_stats)
struct PruneStats { uint64_t probes_in = 0, probes_kept = 0; float ms_prune = 0.0f; };
PruneStats prune_last_stats();
void prune_reset_stats();

struct SearchIO {
  const float *queries = nullptr;  // host or device (queries_on_device)
  bool on_device = false;          // queries and D/I/tie are device pointers
  uint64_t nq = 0, k = 0, n_probe = 0;
  float *D = nullptr;
  int64_t *I = nullptr;
  uint64_t *tie = nullptr;
  uint64_t *slots = nullptr;       // device only, optional: the global slot of every result (~0 on padding)
  float *V = nullptr;              // host only
  uint64_t *counts = nullptr;      // host only
  // multi-GPU: the coarse step of a query slice can run on another rank (device pointers, [nq][n_probe_eff])
  const uint32_t *probes_in = nullptr, *order_in = nullptr;  // skip the coarse step, use these probe lists
  uint32_t *probes_out = nullptr, *order_out = nullptr;      // coarse step only: probe lists + candidate-order ranks
  const SlotFilter *filter = nullptr;  // restrict the candidates to the filter's slots (the coarse step never sees it)
  const ProbePrune *prune = nullptr;   // adaptive probing: the rows of this search's own coarse step pruned before its list phase
};
vi_status device_index_search(const DeviceIndex &ix, const SearchIO &io);

// ---- the calls whose queries are records of the index itself (similar_search.hip, cluster_radius.hip) ----
// The rows of such a call.  Row i is the stored f32 bits of a record: by id — the first record in list order carrying
// ids[i], the one a get reports — or by range — record first + i of list order.
struct StoredRows {
  const uint64_t *ids = nullptr;   // by id: nq ids (host, or device with on_device); null: by range
  uint64_t first = 0;              // by range: rows are records [first, first + nq) of list order
  uint64_t nq = 0;
  bool on_device = false;          // ids and the call's outputs (SimilarIO: every output; RangeSimilarIO: found) are device pointers
};

// ---- search by stored record (similar_search.hip) ----
// Row i is the top-k of the record rows names.  exclude_self deletes that one record (its slot, not its id, not its
// bits) from the row's candidates.  The contract is vi_indexer_search_by_ids / vi_indexer_knn_graph in
// include/vi_amd.h; arguments are checked by the caller (api.cpp): nq > 0, k > 0, n_probe > 0, an unpartitioned index.
struct SimilarIO {
  StoredRows rows;
  uint64_t k = 0, n_probe = 0;
  bool exclude_self = true;
  const SlotFilter *filter = nullptr;
  float *D = nullptr;              // nq x k
  int64_t *I = nullptr;
  uint64_t *tie = nullptr;         // device only, optional
  float *V = nullptr;              // host only, optional: nq x k x dim
  uint64_t *counts = nullptr;      // host only, optional
  uint32_t *found = nullptr;       // by id, optional: records carrying each id
};
vi_status device_index_search_similar(const DeviceIndex &ix, const SimilarIO &io);
// this thread's last device_index_search_similar, summed over its chunks: the rows per chunk used and the bytes
// self_drop_kernel moved; under VI_SIMILAR_TIMING (set, not '0') the host clock around the resolve + gather of the
// queries and around the search and HIP events around self_drop_kernel, else zeros.  device_index_range_similar reports
// the same way: ms_drop / drop_bytes then cover range_find_kernel and range_move_kernel.
struct SimilarTimes { float ms_resolve = 0, ms_search = 0, ms_drop = 0; uint64_t drop_bytes = 0, chunk_rows = 0; };
SimilarTimes similar_last_times();

struct RangeIO {
  const float *queries = nullptr;  // host or device (on_device)
  bool on_device = false;
  uint64_t nq = 0, n_probe = 0;
  float radius2 = 0.0f;            // squared L2 radius, inclusive; not NaN
  const SlotFilter *filter = nullptr;
};
// every probed candidate with reference distance <= radius2, per query in the reference's stable order: all or nothing
vi_status device_index_range_search(const DeviceIndex &ix, const RangeIO &io, RangeResult *out);
// host copies of a result: lims (nq + 1), D, I (total each), V (optional, total x dim: the stored vectors)
vi_status range_result_copy(const RangeResult &r, uint64_t *lims, float *D, int64_t *I, float *V);

// ---- radius search by stored record (similar_search.hip): SimilarIO's rows, a RangeResult for the answer ----
// Row i is the radius search of the record rows names; exclude_self deletes that one record (its slot) from the row, an
// absent id has an empty row.  The contract is vi_indexer_range_search_by_ids / vi_indexer_radius_graph in
// include/vi_amd.h; arguments are checked by the caller (api.cpp): n_probe > 0, radius2 no NaN, an unpartitioned index.
// All or nothing: `found` is written once every chunk has succeeded.
struct RangeSimilarIO {
  StoredRows rows;
  uint64_t n_probe = 0;
  float radius2 = 0.0f;
  bool exclude_self = true;
  const SlotFilter *filter = nullptr;
  uint32_t *found = nullptr;       // by id, optional: records carrying each id
};
vi_status device_index_range_similar(const DeviceIndex &ix, const RangeSimilarIO &io, RangeResult *out);

// ---- clustering the stored records by radius (cluster_radius.hip): the radius graph consumed chunk by chunk ----
// One label and one degree per resident record, in list order.  The contract is vi_indexer_cluster_radius in
// include/vi_amd.h; arguments are checked by the caller (api.cpp): n_probe > 0, radius2 no NaN, an output wanted, an
// unpartitioned index.  All or nothing: the outputs are written once every chunk of every pass has succeeded.
struct ClusterIO {
  bool on_device = false;          // labels and degree are device pointers (n_clusters is a host pointer either way)
  uint64_t n_probe = 0;
  float radius2 = 0.0f;
  uint32_t min_pts = 1;
  const SlotFilter *filter = nullptr;
  int64_t *labels = nullptr;       // [nvec_resident], optional
  uint32_t *degree = nullptr;      // [nvec_resident], optional
  uint64_t *n_clusters = nullptr;  // host, optional
};
vi_status device_index_cluster_radius(const DeviceIndex &ix, const ClusterIO &io);
vi_cluster_stats cluster_last_stats();  // of this thread's last device_index_cluster_radius; zeros after a failed one

// The search engines' environment options, read once per search by read_engine_knobs (search.hip) into the call's SearchBatch.
// A '0' as the first character turns an on-by-default option off.  (The MFMA engine's variables keep its first name, VI_FILTER.)
struct EngineKnobs {
  bool force_generic;       // VI_FORCE_GENERIC (non-zero): the generic engine
  uint32_t force_qg;        // VI_FORCE_QG: queries per group of the VALU list scan (0: chosen)
  uint32_t seg_blocks;      // VI_SEG_BLOCKS: blocks per list segment of the VALU list scan
  bool mfma;                // VI_FILTER=0: the VALU engine instead of the MFMA engine
  bool rank_bf16;           // VI_FILTER_BF16=0: rank with f32 MFMAs instead of bf16 x 3
  bool hi_only;             // VI_FILTER_HI_ONLY=0: never rank from the hi planes alone
  int rank_approx;          // VI_RANK_APPROX: hi-plane ranking of real-valued lists, 0..2 (-1: chosen per index)
  bool debug_approx;        // VI_DEBUG_APPROX: print what rank_approx_mode chose by
  bool coarse_mfma;         // VI_COARSE_FILTER=0: never run the coarse step on the matrix cores
  bool coarse_direct;       // VI_COARSE_DIRECT=0: the coarse select with group records on tables of <= 256 blocks too
  uint32_t segb0;           // VI_FILTER_SEGB: blocks per list segment of the MFMA list phase
  uint32_t gq;              // VI_FILTER_GQ: queries per rank work item, 32 or 128 (0: chosen)
  bool stream_off;          // VI_RANK_STREAM=0: the block-synchronous rank kernel
  bool stream_force;        // VI_RANK_STREAM=1: the streaming rank kernel for any D <= 128
  bool stream_gq256;        // VI_STREAM_GQ=256: streaming groups of 256 bf16-exact queries
  bool rank_i8;             // VI_RANK_I8=0: rank 8-bit descriptors with bf16
  uint32_t item_run;        // VI_ITEM_RUN: work items of one tile stream dealt to one XCD in a row
  bool item_push;           // VI_ITEM_PUSH=0: the work items' columns by kernels of their own behind the scatter
  bool scan_in_totals;      // VI_SCAN_IN_TOTALS=0: the grouping's scans by group_prepare_kernel, a launch of its own, as everywhere without item_push
  bool stream_prof;         // VI_STREAM_PROF: clock the streaming rank kernel
  const char *stream_prof_dump;  // VI_STREAM_PROF_DUMP: file for its per-workgroup clocks, or null
  uint32_t rank_xmode;      // VI_FILTER_XMODE: rank kernel ablations
  uint32_t select_xmode;    // VI_SELECT_XMODE: list select ablations (wrong results)
  uint32_t coarse_xmode;    // VI_SELECT_XMODE_COARSE: coarse select ablations (wrong results)
  // VI_FILTER_STATS (set): the selects' counters; '2': the coarse select's instead, and its clocks; '3' / '4': print
  // the list select's clocks and counters; '4': count every 64th query only
  bool stats, stats_coarse, stats_print;
  uint32_t stats_mask;
};
EngineKnobs read_engine_knobs();

// ---- grouping ids by list on the GPU (list_build.hip; device_index_from_order is declared with the routes above) ----
// ids 0..n-1 grouped by label, ascending id inside a label (stable radix sort): order (device, n u32), seg (device,
// k+1 u32 offsets into order) and the offsets on the host if off_host is given.  Complete on return.  scratch_keep
// (optional): the sort's scratch (3 n + 256 n / 4096 words) in a buffer of the caller's, kept from call to call.
vi_status group_ids_by_label_device(const uint32_t *labels_dev, uint64_t n, uint64_t k, DevBuf<uint32_t> &order,
                                    DevBuf<uint32_t> &seg, std::vector<uint64_t> *off_host, hipStream_t st,
                                    DevBuf<uint32_t> *scratch_keep = nullptr);
// ---- shard files from records in HBM (shard_export.hip) ----
struct ShardExportWs {  // staging of an export, reused from shard to shard
  DevBuf<uint8_t> image;
  DevBuf<uint64_t> d_src, d_id0, d_dst;
  DevBuf<uint32_t> d_first;
  uint8_t *host = nullptr;  // pinned
  uint64_t host_cap = 0;
  ~ShardExportWs();
};
// shard_<id>.bin from device-resident points, byte-identical to shard_save_to (shards.cpp): list i of the shard is rows
// order_dev[src_off[i] .. + len[i]) of X_dev, VectorMeta.id the row; written under its final name
vi_status shard_export_device(const std::string &shards_dir, uint64_t shard_id, uint32_t dim, const std::vector<uint64_t> &cids,
                              const float *cvecs_host, const std::vector<uint64_t> &src_off, const std::vector<uint32_t> &len,
                              const float *X_dev, const uint32_t *order_dev, const uint64_t *ext_dev, const uint64_t *ts_dev,
                              uint64_t now, ShardExportWs &ws, hipStream_t st);
// the same from the blocks of a resident index: the lists cids in file order with the records, external ids and
// timestamps the index holds, VectorMeta.id = the record's list-order ordinal, written to `path`
vi_status shard_export_blocks(const DeviceIndex &ix, const std::string &path, uint64_t shard_id, const std::vector<uint64_t> &cids,
                              const float *cvecs_host, ShardExportWs &ws, uint64_t *bytes_out);

// ---- appending records to a resident index (list_update.hip; device_index_update is declared with the routes above) ----
// labels_dev[i] (device, n u32) = the list the reference's coarse step probes first for row i of rows_dev (device, n x dim):
// the index's own coarse step with n_probe = 1, in chunks
vi_status device_index_label_rows(const DeviceIndex &ix, const float *rows_dev, uint64_t n, uint32_t *labels_dev);
// one chunk of it, and of a refine's labelling (list_refine.hip), as one search: m rows, k 1, n_probe 1, probes_out =
// labels_dev; order_scratch: m words of the caller's, written and not read
vi_status device_index_label_chunk(const DeviceIndex &ix, const float *rows_dev, uint64_t m, uint32_t *labels_dev, uint32_t *order_scratch);

vi_status merge_partials_packed_device(int device, uint64_t nq, uint64_t k, uint32_t parts, const void *packed,
                                       float *D_out, int64_t *I_out);
vi_status merge_partials_device(int device, uint64_t nq, uint64_t k, uint32_t parts, const float *D_parts,
                                const int64_t *I_parts, const uint64_t *tie_parts, float *D_out,
                                int64_t *I_out);

// ---- merging per-rank radius results (range_merge.hip) ----
// `parts` (1..kRangeMergeMaxParts) CSR radius results of the same nq queries, every row sorted by (bits(D), tie) -> one
// result in that order on `device`, owned by *out (ix == nullptr).  The four arrays are HOST arrays of device pointers.
// One stream, one synchronisation before the output is allocated, synchronised on return.  Sortedness is not checked:
// unsorted rows give an unspecified order, never an access outside the buffers.
constexpr uint32_t kRangeMergeMaxParts = 64;
vi_status range_merge_device(int device, uint64_t nq, uint32_t parts, const uint64_t *const *lims_dev, const float *const *D_dev,
                             const int64_t *const *I_dev, const uint64_t *const *tie_dev, RangeResult *out);
// HIP-event times of this thread's last range_merge_device under VI_RANGE_MERGE_TIMING (set, not '0'); zeros otherwise
struct RangeMergeTimes { float ms_lims = 0, ms_alloc = 0, ms_place = 0; };  // ms_alloc: lims read-back, the sync, the allocations
RangeMergeTimes range_merge_last_times();

vi_status l2sq_pairs_device(const float *a, const float *b, uint64_t n, uint32_t d, int order, float *out);

}  // namespace vi
