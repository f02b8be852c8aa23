// rebalance_rules_check.cpp — a host program over csrc/rebalance_rules.hpp alone: the functions vi_indexer_rebalance's
// kernels and host loop call, run on plain arrays.
//   no argument: the checks below; prints one line per failed check, exit status 1 if any failed
//     * the plan: both orderings, the caps, a list that qualifies as donor and receiver, no donor, no receiver
//     * the farthest-member key: one unsigned maximum = largest distance, lowest position among equals; +0.0 against
//       the smallest distances; positions up to 2^32 - 2
//     * the side rule (ties to side 0) and the skip rule
//     * the distance chain against a plain unfused loop
//   plan <split_factor> <receiver_max_len> <max_splits> <len> ...: prints "donor receiver" per pair of the plan
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rebalance_rules.hpp"

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
    }                               \
  } while (0)

using Pairs = std::vector<vi::RebalancePair>;

static bool same(const Pairs &got, const std::vector<std::pair<uint32_t, uint32_t>> &want) {
  if (got.size() != want.size()) return false;
  for (size_t i = 0; i < got.size(); ++i)
    if (got[i].donor != want[i].first || got[i].receiver != want[i].second) return false;
  return true;
}

static void check_plan() {
  {  // n = 200, mean 20: donors are longer than 40 — 90 (list 2), 50 twice (lists 0 and 5, the lower index first)
    const std::vector<uint32_t> len{50, 0, 90, 1, 0, 50, 4, 3, 2, 0};
    CHECK(same(vi::rebalance_plan(len.data(), len.size(), 2.0, 0, 0), {{2, 1}, {0, 4}, {5, 9}}), "plan: empty receivers in index order");
    CHECK(same(vi::rebalance_plan(len.data(), len.size(), 2.0, 2, 0), {{2, 1}, {0, 4}, {5, 9}}), "plan: the empty lists come before the short ones");
    CHECK(same(vi::rebalance_plan(len.data(), len.size(), 2.0, 0, 2), {{2, 1}, {0, 4}}), "plan: max_splits caps the pairs");
    CHECK(same(vi::rebalance_plan(len.data(), len.size(), 2.0, 0, 1), {{2, 1}}), "plan: max_splits 1");
    CHECK(same(vi::rebalance_plan(len.data(), len.size(), 3.0, 0, 0), {{2, 1}}), "plan: a higher factor leaves one donor");
    CHECK(vi::rebalance_plan(len.data(), len.size(), 5.0, 0, 0).empty(), "plan: no donor");
  }
  {  // receivers by (length ascending, index ascending); more donors than receivers
    const std::vector<uint64_t> len{3, 100, 1, 200, 1, 150, 2, 0};
    // n = 457, mean 57.125: donors 200 (3), 150 (5); 100 is not above 114.25
    CHECK(same(vi::rebalance_plan(len.data(), len.size(), 2.0, 3, 0), {{3, 7}, {5, 2}}), "plan: receivers by length, then index");
    CHECK(same(vi::rebalance_plan(len.data(), len.size(), 1.0, 1, 0), {{3, 7}, {5, 2}, {1, 4}}), "plan: factor 1, three donors");
    CHECK(same(vi::rebalance_plan(len.data(), len.size(), 1.0, 0, 0), {{3, 7}}), "plan: fewer receivers than donors");
  }
  {  // a list that qualifies as both is a donor only: lengths 4 and 0 x 7 -> mean 0.5, the list of 4 is a donor and, at
     // receiver_max_len 10, would be a receiver too
    const std::vector<uint32_t> len{0, 4, 0, 0, 0, 0, 0, 0};
    CHECK(same(vi::rebalance_plan(len.data(), len.size(), 2.0, 10, 0), {{1, 0}}), "plan: donor and receiver overlap");
    const std::vector<uint32_t> two{5, 5};
    CHECK(vi::rebalance_plan(two.data(), two.size(), 1.0, 100, 0).empty(), "plan: equal lists at factor 1 give no donor");
    const std::vector<uint32_t> ones{1, 0, 0, 0};  // longer than the mean, but a list of one record is never split
    CHECK(vi::rebalance_plan(ones.data(), ones.size(), 1.0, 0, 0).empty(), "plan: a list of one record is no donor");
    CHECK(vi::rebalance_plan((const uint32_t *)nullptr, 0, 2.0, 0, 0).empty(), "plan: no list");
    const std::vector<uint32_t> full{9, 9, 40};
    CHECK(vi::rebalance_plan(full.data(), full.size(), 2.0, 0, 0).empty(), "plan: no receiver");
  }
}

static uint64_t max_key(const std::vector<float> &dist, const std::vector<uint32_t> &pos) {
  uint64_t best = 0;
  for (size_t i = 0; i < dist.size(); ++i) {
    const uint64_t k = vi::rebalance_far_key(dist[i], pos[i]);
    if (k > best) best = k;
  }
  return best;
}

static void check_keys() {
  const float tiny = std::nextafter(0.0f, 1.0f);  // the smallest subnormal
  {
    const std::vector<float> d{1.0f, 7.5f, 7.5f, 3.0f, 7.5f};
    const uint64_t k = max_key(d, {0, 1, 2, 3, 4});
    CHECK(vi::rebalance_key_pos(k) == 1 && vi::rebalance_key_dist_bits(k) == vi::rebalance_float_bits(7.5f), "key: lowest position among equal distances");
    const uint64_t r = max_key(d, {40, 30, 20, 10, 25});  // (the order members arrive in does not matter)
    CHECK(vi::rebalance_key_pos(r) == 20, "key: lowest position, members in any order");
  }
  {
    const uint64_t k = max_key({0.0f, tiny, 0.0f}, {0, 1, 2});
    CHECK(vi::rebalance_key_pos(k) == 1 && !vi::rebalance_skip(k), "key: the smallest distance beats +0.0, and is no skip");
    const uint64_t z = max_key({0.0f, 0.0f, 0.0f}, {5, 3, 4});
    CHECK(vi::rebalance_key_pos(z) == 3 && vi::rebalance_skip(z), "key: all distances +0.0 -> lowest position, skipped");
    CHECK(vi::rebalance_far_key(0.0f, 0xFFFFFFFEu) != 0, "key: no member's key is 0");
    CHECK(vi::rebalance_key_pos(vi::rebalance_far_key(2.0f, 0xFFFFFFFEu)) == 0xFFFFFFFEu, "key: the last position survives");
    CHECK(vi::rebalance_far_key(tiny, 0xFFFFFFFEu) > vi::rebalance_far_key(0.0f, 0), "key: distance outranks position");
    CHECK(vi::rebalance_far_key(INFINITY, 9) > vi::rebalance_far_key(3.0e38f, 0), "key: +inf is the largest distance");
  }
  // bit patterns of non-negative floats order as the values do
  const float v[] = {0.0f, tiny, 1e-30f, 0.5f, 1.0f, std::nextafter(1.0f, 2.0f), 255.0f * 255.0f * 4096.0f, 3.0e38f, INFINITY};
  for (size_t i = 0; i + 1 < sizeof(v) / sizeof(v[0]); ++i)
    CHECK(vi::rebalance_far_key(v[i], 7) < vi::rebalance_far_key(v[i + 1], 7), "key: order of distance %zu and %zu", i, i + 1);
}

static void check_sides_and_chain() {
  CHECK(vi::rebalance_side(2.0f, 1.0f) == 1 && vi::rebalance_side(1.0f, 2.0f) == 0, "side: the nearer centre");
  CHECK(vi::rebalance_side(3.0f, 3.0f) == 0 && vi::rebalance_side(0.0f, 0.0f) == 0, "side: a tie goes to side 0");
  CHECK(vi::rebalance_side(std::nextafter(3.0f, 4.0f), 3.0f) == 1, "side: one ulp decides");
  CHECK(vi::rebalance_side_empty(0, 5) && vi::rebalance_side_empty(5, 0) && !vi::rebalance_side_empty(1, 1), "side: empty");
  // the chain: a plain loop with separate subtract, multiply and add, on values whose products round
  std::vector<float> a(37), b(37);
  uint32_t s = 12345;
  for (size_t i = 0; i < a.size(); ++i) {
    s = s * 1664525u + 1013904223u;
    a[i] = (float)(s >> 8) / 65536.0f - 128.0f;
    s = s * 1664525u + 1013904223u;
    b[i] = (float)(s >> 8) / 65536.0f - 128.0f;
  }
  volatile float acc = 0.0f;
  for (size_t i = 0; i < a.size(); ++i) {
    volatile float t = a[i] - b[i];
    volatile float sq = t * t;
    acc = acc + sq;
  }
  const float got = vi::rebalance_dist(a.data(), b.data(), (uint32_t)a.size());
  CHECK(vi::rebalance_float_bits(got) == vi::rebalance_float_bits((float)acc), "chain: differs from the unfused loop");
  CHECK(vi::rebalance_float_bits(vi::rebalance_dist(a.data(), a.data(), 37)) == 0, "chain: a row against itself is +0.0");
  const float neg[] = {-0.0f}, pos[] = {0.0f};
  CHECK(vi::rebalance_float_bits(vi::rebalance_dist(neg, pos, 1)) == 0, "chain: -0.0 against +0.0 is +0.0, never -0.0");
}

int main(int argc, char **argv) {
  if (argc >= 2 && std::strcmp(argv[1], "plan") == 0) {
    if (argc < 5) return 2;
    const double factor = std::atof(argv[2]);
    const uint64_t rmax = std::strtoull(argv[3], nullptr, 10), cap = std::strtoull(argv[4], nullptr, 10);
    std::vector<uint64_t> len;
    for (int i = 5; i < argc; ++i) len.push_back(std::strtoull(argv[i], nullptr, 10));
    for (const vi::RebalancePair &p : vi::rebalance_plan(len.data(), len.size(), factor, rmax, cap)) std::printf("%u %u\n", p.donor, p.receiver);
    return 0;
  }
  check_plan();
  check_keys();
  check_sides_and_chain();
  return failures ? 1 : 0;
}
