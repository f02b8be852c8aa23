// grouping.hpp — the probe grouping (grouping.hip): the counting sort of a batch's nq x n_probe (query, probe) pairs by
// list, the scans over the lists built from it (where each list's pairs, work items, segment runs and record tiles start)
// and the MFMA engine's rank work items.  One request, one entry; which chain of launches serves a request is a value
// (GroupingRoute) computed from the request alone.  It takes no SearchBatch (the generic engine groups chunks of one): the index,
// the workspace it fills and the stream (group_probes: the context, whose event it waits on).
#pragma once
#include <cstdint>

#include "device_index.hpp"
#include "search_internal.hpp"

namespace vi {

// The grouping's scans inside list_totals_kernel, completed by item_push_kernel (two launches, no group_prepare_kernel):
// every workgroup of item_push_kernel scans the sums of the 64-list workgroups of list_totals_kernel itself, one per
// thread — so at most this many of them (16 384 lists: every table the direct coarse select, which item_push_kernel
// depends on, takes).  Above that the route is GroupingRoute::PreparePush.
constexpr uint32_t kGroupScanBlocks = 256;
inline bool group_scan_in_totals_applicable(uint64_t nlists) { return (nlists + 63) / 64 <= kGroupScanBlocks; }

// What to group and what the caller has ready for it.  The grouping fills ws.{cnt, list_tot, seg_start, item_start,
// segrun_start, pairs} and the grouping's counts of ws.stats (StatWord, search_internal.hpp).
struct GroupingRequest {
  const uint32_t *probes = nullptr;  // [nq][P] list ids, kNoPos: no probe
  uint64_t nq = 0;
  uint32_t P = 0;
  uint32_t qg = 0;               // queries per work item
  uint32_t segb0 = 0;            // blocks per list segment (list_segments, scan.hpp)
  bool histogram_done = false;   // ws.cnt holds the batch's histogram: the coarse step of the fast paths leaves it behind
  // ---- the MFMA engine ----
  const uint32_t *qtot = nullptr;  // [nq] the queries' record totals, scanned into ...
  uint32_t *qoff = nullptr;        // ... [nq + 1] their offsets
  const uint32_t *pair_rank = nullptr;  // a pair's place among the pairs of its (list, sub-bin): the increments of that histogram
  uint32_t push_run = 0;         // not 0: the scatter builds the streaming rank kernel's work items too (item_push_kernel),
                                 // dealt to the XCDs in runs of this many; the caller compares the counts it gets back
                                 // with the item and record buffers, grows them and pushes again (repush_items)
  bool counts_cleared = false;   // the grouping's counts were cleared ahead (split_queries_kernel), so the scans may ride in
                                 // list_totals_kernel, whose every workgroup adds to them (VI_SCAN_IN_TOTALS=0: left false)
  // ---- optional outputs (the item push leaves both whatever is asked) ----
  bool tile_start = false;       // ws.tile_start: first record tile of each list
  bool pair_pos = false;         // ws.pair_pos: where each pair sits among the pairs of its list
};

// the chains of launches behind the (optional) histogram
enum class GroupingRoute {
  AtomicScatter,  // list totals, group_prepare_kernel, cursor_kernel, group_scatter_kernel
  RankedScatter,  // ... the same with group_scatter_ranked_kernel: the pairs' ranks instead of returning atomics
  PreparePush,    // list totals with the sub-bins' prefixes, group_prepare_kernel, item_push_kernel
  ScansPush       // list totals with the scans of the lists and the queries, item_push_kernel
};
GroupingRoute grouping_route(const GroupingRequest &rq, uint64_t nlists);

// Groups the pairs on ctx.stream; `counts` is the host copy of the grouping's counts, read back behind ctx.ev[5] while
// the scatter runs (the pipeline's one synchronisation point).
vi_status group_probes(const DeviceIndex &ix, SearchContext &ctx, const GroupingRequest &rq, GroupingCounts &counts);
// the item push of a request once more, into item and record buffers the caller has grown since group_probes
vi_status repush_items(const DeviceIndex &ix, SearchWorkspace &ws, const GroupingRequest &rq, hipStream_t st);

// clears the sub-bin counters (ws.cnt) and counts `total` = nq x P probes into them
vi_status launch_probe_histogram(const DeviceIndex &ix, SearchWorkspace &ws, const uint32_t *probes, uint32_t total, uint32_t P, hipStream_t st);

// ---- the rank work items where the scatter did not push them: kernels of their own behind it ----
// ws.item_list: the list of every work item
vi_status launch_item_list(const DeviceIndex &ix, SearchWorkspace &ws, uint32_t nitems, hipStream_t st);
// ws.items: every work item's descriptor, dealt to the XCDs in runs of kn.item_run
vi_status launch_item_desc(const DeviceIndex &ix, SearchWorkspace &ws, const EngineKnobs &kn, uint32_t gq, uint32_t nitems, hipStream_t st);
// ws.item_{qcol, grec, sdesc}, ws.gpos: the streaming rank kernel's columns, from ws.items
vi_status launch_item_cols(SearchWorkspace &ws, uint32_t P, uint32_t gq, uint32_t nitems, hipStream_t st);

}  // namespace vi
