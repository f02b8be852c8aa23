// flat_ip_range.hpp — exact (flat) inner-product threshold search over every resident record of a built index
// (flat_ip_range.hip): per query every admitted record whose chain score s >= min_score, out to CSR.  The contract is
// vi_indexer_range_search_exact_ip in include/vi_amd.h; DESIGN.md §4w has the design.  Arguments are checked by the caller
// (api.cpp): the scalar threshold no NaN, an unpartitioned handle; what depends on the index is checked here, before any
// device work.  The pool, the query chunks and the report are those of the exact radius search (flat_range.hpp).
#pragma once
#include <cstdint>

#include "common.hpp"
#include "flat_range.hpp"

namespace vi {

struct ExactIpRangeIO {
  const float *queries = nullptr;     // host or device (on_device)
  bool on_device = false;             // queries and min_scores are device pointers
  uint64_t nq = 0;
  float min_score = 0.0f;             // every query's threshold where min_scores is null; not NaN
  const float *min_scores = nullptr;  // optional: nq thresholds, a NaN one is an empty row
  uint64_t pool_cap = 0;              // 0: the default (exact_range_pool_cap); never changes a result
  const SlotFilter *filter = nullptr;
};
// every admitted record with chain score >= the query's threshold, rows sorted by (score descending, ordinal), D = the
// scores, tie = ordinal: all or nothing
vi_status device_index_range_exact_ip(const DeviceIndex &ix, const ExactIpRangeIO &io, RangeResult *out);
vi_exact_range_stats exact_ip_range_last_stats();  // of this thread's last device_index_range_exact_ip; zeros after a failed one

}  // namespace vi
