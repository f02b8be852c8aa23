// flat_join.hpp — the exact radius self-join of a built index (flat_join.hip): the exact radius graph of its stored
// records and the clustering over it.  The contracts are vi_indexer_radius_graph_exact and vi_indexer_cluster_radius_exact
// in include/vi_amd.h; DESIGN.md §4t has the design.  Arguments are checked by the caller (api.cpp): radius2 no NaN, an
// output wanted, an unpartitioned handle; what depends on the index is checked here, before any device work.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace vi {

struct DeviceIndex;
struct SlotFilter;
struct RangeResult;

struct ExactJoinIO {
  float radius2 = 0.0f;            // not NaN; negative: no pair
  const SlotFilter *filter = nullptr;
  // the clustering
  bool on_device = false;          // labels and degree are device pointers (n_clusters is a host pointer either way)
  uint32_t min_pts = 1;
  int64_t *labels = nullptr;       // [nvec_resident], optional
  uint32_t *degree = nullptr;      // [nvec_resident], optional
  uint64_t *n_clusters = nullptr;  // host, optional
  // the graph
  bool exclude_self = true;
  uint64_t pool_cap = 0;           // 0: the default; never changes a result
};
// labels, degrees and the cluster count of the exact radius graph, which is never held: all or nothing
vi_status device_index_cluster_exact(const DeviceIndex &ix, const ExactJoinIO &io);
// the whole exact radius graph, rows sorted by (distance bits, ordinal), tie = ordinal: all or nothing
vi_status device_index_graph_exact(const DeviceIndex &ix, const ExactJoinIO &io, RangeResult *out);
vi_exact_join_stats exact_join_last_stats();  // of this thread's last call of either; zeros after a failed one

}  // namespace vi
