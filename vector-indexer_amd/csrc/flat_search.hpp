// flat_search.hpp — exact (flat) k-NN over every resident record of a built index (flat_search.hip).  The contract is
// vi_indexer_search_exact in include/vi_amd.h; DESIGN.md §4r has the design.  Arguments are checked by the caller
// (api.cpp): nq > 0, 1 <= k <= 128, the outputs present, an unpartitioned handle; what depends on the index is checked
// here, before any device work.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace vi {

struct DeviceIndex;
struct SlotFilter;

constexpr uint64_t kExactMaxK = 128;        // the MFMA engine's widest select, which seeds the bound
constexpr uint64_t kExactMaxCap = 8192;     // candidates per query one wave sorts in LDS (64 KB of keys)
constexpr uint64_t kExactSeedProbe = 16;    // n_probe of the seeding search when the caller leaves it to the call

// a result key: distance bits above the record's list-order ordinal — distances are non-negative, so unsigned order is
// (distance, ordinal) order; all ones: no record
inline uint64_t exact_key(uint32_t dist_bits, uint32_t ordinal) { return ((uint64_t)dist_bits << 32) | ordinal; }
// candidates a query may collect before it is sent down the sort-everything path
inline uint64_t exact_cand_cap(uint64_t asked, uint64_t k) {
  const uint64_t cap = asked ? (asked < k ? k : asked) : (8 * k < 1024 ? 1024 : 8 * k);
  return cap < kExactMaxCap ? cap : kExactMaxCap;
}

struct ExactIO {
  const float *queries = nullptr;  // host or device (on_device)
  bool on_device = false;          // queries and every output are device pointers
  uint64_t nq = 0, k = 0;
  const SlotFilter *filter = nullptr;
  uint64_t seed_probe = 0, cand_cap = 0;  // 0: the call's defaults; neither changes a result
  float *D = nullptr;              // nq x k
  int64_t *I = nullptr;
  uint64_t *ord = nullptr;         // optional: list-order ordinals, all ones on padding
  uint64_t *counts = nullptr;      // optional: results per query
};
vi_status device_index_search_exact(const DeviceIndex &ix, const ExactIO &io);
vi_exact_stats exact_last_stats();  // of this thread's last device_index_search_exact; zeros after a failed one

}  // namespace vi
