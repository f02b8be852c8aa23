// flat_knn.hpp — the exact k-NN graph of the stored records of a built index (flat_knn.hip): a bounded triangular
// self-join.  The contract is vi_indexer_knn_graph_exact in include/vi_amd.h; DESIGN.md §4u has the design.  Arguments
// are checked by the caller (api.cpp): 1 <= k <= 128, D and I present, an unpartitioned handle; what depends on the index
// is checked here, before any device work.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace vi {

struct DeviceIndex;
struct SlotFilter;

constexpr uint64_t kKnnPoolMin = 1ull << 22;  // default pool: max(this, 2 k + 16 per row) entries, 12 bytes each

inline uint64_t exact_knn_pool_cap(uint64_t asked, uint64_t k, uint64_t rows) {
  const uint64_t want = (2 * k + 16) * rows;
  return asked ? asked : (want < kKnnPoolMin ? kKnnPoolMin : want);
}

struct ExactKnnIO {
  const SlotFilter *filter = nullptr;
  uint64_t k = 0;
  bool exclude_self = true;
  uint64_t seed_probe = 0, pool_cap = 0;  // 0: the call's defaults; neither changes a result
  bool on_device = false;                 // every output is a device pointer
  float *D = nullptr;                     // [nvec_resident][k]
  int64_t *I = nullptr;
  uint64_t *ord = nullptr;                // optional: list-order ordinals, all ones on padding
  uint64_t *counts = nullptr;             // optional: entries per row
};
// the k smallest keys (distance bits, ordinal) of every stored record over the participants: all or nothing
vi_status device_index_knn_graph_exact(const DeviceIndex &ix, const ExactKnnIO &io);
vi_exact_knn_stats exact_knn_last_stats();  // of this thread's last device_index_knn_graph_exact; zeros after a failed one

}  // namespace vi
