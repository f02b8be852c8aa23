// rebalance_rules.hpp — the rules of vi_indexer_rebalance's split step (list_split.hip, list_refine.hip) that are plain
// arithmetic: which lists give and which receive (the plan), one term of the distance chain, the key that orders the
// members of a donor by "largest distance, lowest position", the side a member falls on and when a pair is skipped.
// Nothing of HIP is included, so a host program runs the very same functions on plain arrays
// (tests/rebalance_rules_check.cpp); the kernels and the host loop call them as they stand.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define VI_REBALANCE_FN __host__ __device__ inline
#else
#define VI_REBALANCE_FN inline
#endif

namespace vi {

// One term of the reference's euclidean_distance_squared (src/utils.rs:28-30): an unfused (a - b) * (a - b) added to the
// chain, column after column from +0.0.  (The library is built with -ffp-contract=off; so is every program that uses this.)
VI_REBALANCE_FN float rebalance_dist_add(float acc, float a, float b) {
  const float t = a - b;
  const float sq = t * t;
  return acc + sq;
}
// ... and the whole chain over two rows of dim values, as a host reads it
VI_REBALANCE_FN float rebalance_dist(const float *a, const float *b, uint32_t dim) {
  float acc = 0.0f;
  for (uint32_t j = 0; j < dim; ++j) acc = rebalance_dist_add(acc, a[j], b[j]);
  return acc;
}

VI_REBALANCE_FN uint32_t rebalance_float_bits(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}

// The farthest-member key: the distance's bits above the inverted position, so that ONE unsigned maximum gives "the
// largest distance, and among equal distances the lowest position".  A distance of the chain above is never negative
// and never -0.0 (a sum of squares from +0.0), so its bit pattern orders as its value does.  Positions are below
// 2^32 - 1, so no member's key is 0: 0 is "no member yet".
VI_REBALANCE_FN uint64_t rebalance_far_key(float dist, uint32_t pos) {
  return ((uint64_t)rebalance_float_bits(dist) << 32) | (uint64_t)(uint32_t)~pos;
}
VI_REBALANCE_FN uint32_t rebalance_key_pos(uint64_t key) { return ~(uint32_t)key; }
VI_REBALANCE_FN uint32_t rebalance_key_dist_bits(uint64_t key) { return (uint32_t)(key >> 32); }
// a pair is skipped when its second seed lies ON the first: d(x_b, x_a) == 0, every member equal (+0.0 is the only zero)
VI_REBALANCE_FN bool rebalance_skip(uint64_t key_b) { return rebalance_key_dist_bits(key_b) == 0; }

// the side of a member at distance da from ca and db from cb: 1 only where cb is strictly nearer; a tie stays on side 0
VI_REBALANCE_FN uint32_t rebalance_side(float da, float db) { return db < da ? 1u : 0u; }

// an inner iteration ends a pair when a side came out empty (the centres stay) or when no bit of either centre changed
VI_REBALANCE_FN bool rebalance_side_empty(uint32_t count0, uint32_t count1) { return count0 == 0 || count1 == 0; }

// ---- the plan (host) ----
struct RebalancePair {
  uint32_t donor, receiver;
};

// Over the list lengths at the start of an iteration, mean = n / lists in double (n = the sum of the lengths):
//   donors     len >= 2 and (double)len > split_factor * mean, by (len descending, index ascending)
//   receivers  len <= receiver_max_len and not a donor,        by (len ascending, index ascending)
// pair i = (donor i, receiver i), i < min(#donors, #receivers, max_splits or no cap)
template <typename L>
inline std::vector<RebalancePair> rebalance_plan(const L *len, uint64_t nlists, double split_factor, uint64_t receiver_max_len,
                                                 uint64_t max_splits) {
  uint64_t n = 0;
  for (uint64_t l = 0; l < nlists; ++l) n += (uint64_t)len[l];
  std::vector<RebalancePair> pairs;
  if (nlists == 0) return pairs;
  const double mean = (double)n / (double)nlists;
  std::vector<uint32_t> donors, receivers;
  for (uint64_t l = 0; l < nlists; ++l) {
    const uint64_t v = (uint64_t)len[l];
    if (v >= 2 && (double)v > split_factor * mean) donors.push_back((uint32_t)l);
    else if (v <= receiver_max_len) receivers.push_back((uint32_t)l);
  }
  std::stable_sort(donors.begin(), donors.end(), [&](uint32_t a, uint32_t b) { return (uint64_t)len[a] > (uint64_t)len[b]; });
  std::stable_sort(receivers.begin(), receivers.end(), [&](uint32_t a, uint32_t b) { return (uint64_t)len[a] < (uint64_t)len[b]; });
  uint64_t m = std::min<uint64_t>(donors.size(), receivers.size());
  if (max_splits) m = std::min(m, max_splits);
  pairs.resize(m);
  for (uint64_t i = 0; i < m; ++i) pairs[i] = RebalancePair{donors[i], receivers[i]};
  return pairs;
}

}  // namespace vi
