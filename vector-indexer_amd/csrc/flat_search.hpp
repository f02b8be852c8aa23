// flat_search.hpp — exact (flat) k-NN over every resident record of a built index (flat_search.hip).  The contract is
// vi_indexer_search_exact in include/vi_amd.h; DESIGN.md §4r has the design.  Arguments are checked by the caller
// (api.cpp): nq > 0, 1 <= k <= 128, the outputs present, an unpartitioned handle; what depends on the index is checked
// here, before any device work.
#pragma once
#include <cstdint>
#include <cstdlib>

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
// workgroups that share one query tile's `nwork` blocks in a query-side sweep (the grid's y): `rounds` workgroups per CU
// over the tiles, each walking the blocks split, split + nsplit, ...  VI_EXACT_BLOCK_SPLITS=n (n >= 1, read on every
// call) caps the count — a tuning and test knob: fewer splits are longer walks.  Unset, empty, 0 or no number: no cap.
// No result depends on it.
inline uint32_t exact_block_splits(uint32_t rounds, int cus, uint32_t ntiles, uint32_t nwork) {
  const uint32_t fill = (rounds * (uint32_t)(cus > 1 ? cus : 1) + ntiles - 1) / ntiles;
  uint32_t nsplit = nwork < fill ? nwork : fill;  // (fill >= 1)
  if (const char *e = getenv("VI_EXACT_BLOCK_SPLITS")) {
    uint64_t n = 0;
    const char *p = e;
    for (; *p >= '0' && *p <= '9'; ++p) n = n < (1ull << 32) ? n * 10 + (uint64_t)(*p - '0') : n;
    if (p != e && *p == '\0' && n >= 1 && n < nsplit) nsplit = (uint32_t)n;
  }
  return nsplit;
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
