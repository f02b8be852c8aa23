// flat_range.hpp — exact (flat) radius search over every resident record of a built index (flat_range.hip).  The contract
// is vi_indexer_range_search_exact in include/vi_amd.h; DESIGN.md §4s has the design.  Arguments are checked by the caller
// (api.cpp): the scalar radius no NaN, an unpartitioned handle; what depends on the index is checked here, before any
// device work.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace vi {

struct DeviceIndex;
struct SlotFilter;
struct RangeResult;

constexpr uint64_t kRangeSortLds = 8192;        // keys of one row a wave sorts in LDS (64 KB); longer rows: sort_rows_u64
constexpr uint64_t kRangeQueryChunk = 65536;    // queries swept at a time
constexpr uint64_t kRangePoolMin = 1ull << 22;  // default pool: max(this, 256 per query of the chunk) hits, 12 bytes each

inline uint64_t exact_range_pool_cap(uint64_t asked, uint64_t chunk_queries) {
  return asked ? asked : (256 * chunk_queries < kRangePoolMin ? kRangePoolMin : 256 * chunk_queries);
}

struct ExactRangeIO {
  const float *queries = nullptr;  // host or device (on_device)
  bool on_device = false;          // queries and radii are device pointers
  uint64_t nq = 0;
  float radius2 = 0.0f;            // every query's radius where radii is null; not NaN
  const float *radii = nullptr;    // optional: nq radii, a NaN or negative one is an empty row
  uint64_t pool_cap = 0;           // 0: the default; never changes a result
  const SlotFilter *filter = nullptr;
};
// every admitted record with reference distance <= the query's radius, rows sorted by (distance bits, ordinal), tie =
// ordinal: all or nothing
vi_status device_index_range_exact(const DeviceIndex &ix, const ExactRangeIO &io, RangeResult *out);
vi_exact_range_stats exact_range_last_stats();  // of this thread's last device_index_range_exact; zeros after a failed one

}  // namespace vi
