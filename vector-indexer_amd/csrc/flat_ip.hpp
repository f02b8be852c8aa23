// flat_ip.hpp — exact (flat) inner-product k-NN over every resident record of a built index (flat_ip.hip).  The contract is
// vi_indexer_search_exact_ip in include/vi_amd.h; DESIGN.md §4v has the design.  Arguments are checked by the caller
// (api.cpp): nq > 0, 1 <= k <= 128, the outputs present, an unpartitioned handle; what depends on the index is checked
// here, before any device work.  The call's arguments, options and report are those of the exact L2 search (ExactIO,
// exact_cand_cap, vi_exact_stats: flat_search.hpp); D carries scores, larger first, padded with -inf.
#pragma once
#include "common.hpp"
#include "flat_search.hpp"

namespace vi {

vi_status device_index_search_exact_ip(const DeviceIndex &ix, const ExactIO &io);
vi_exact_stats exact_ip_last_stats();  // of this thread's last device_index_search_exact_ip; zeros after a failed one
vi_exact_ip_seed_stats exact_ip_seed_last_stats();  // ... and of its ladder (flat_ip_seed.hip); zeros after a failed one

}  // namespace vi
