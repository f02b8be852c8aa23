// refine_rules_check.cpp — a host program over csrc/refine_rules.hpp alone: the functions vi_indexer_refine's kernels call,
// run on plain arrays.  Prints one line per failed check; exit status 1 if any failed.
//   * ordinal <-> slot over layouts with empty lists and lists of 1 / 63 / 64 / 65 / 4097 records
//   * the mean chain against a plain loop
//   * the fixed-point test
//   * the imbalance factor on known length vectors
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "refine_rules.hpp"

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
    }                               \
  } while (0)

// lists back to back, each padded to whole blocks of 64: the layout every index route plans
template <typename P>
static void check_layout(const std::vector<uint32_t> &len, const char *what) {
  const uint32_t nl = (uint32_t)len.size();
  std::vector<uint32_t> first(nl);
  std::vector<P> prefix(nl);
  uint64_t blocks = 0, n = 0;
  for (uint32_t l = 0; l < nl; ++l) {
    first[l] = (uint32_t)blocks;
    prefix[l] = (P)n;
    blocks += (len[l] + 63u) / 64u;
    n += len[l];
  }
  std::vector<uint8_t> used(blocks * 64 + 1, 0);
  uint64_t ord = 0;
  for (uint32_t l = 0; l < nl; ++l)
    for (uint32_t p = 0; p < len[l]; ++p, ++ord) {
      const uint32_t got_l = vi::refine_list_of_ordinal(prefix.data(), nl, ord);
      CHECK(got_l == l, "%s: ordinal %llu lies in list %u, not %u", what, (unsigned long long)ord, l, got_l);
      const uint64_t slot = vi::refine_slot_of_ordinal(prefix.data(), first.data(), nl, ord);
      CHECK(slot == (uint64_t)first[l] * 64 + p, "%s: ordinal %llu has slot %llu", what, (unsigned long long)ord, (unsigned long long)slot);
      CHECK(slot < blocks * 64, "%s: slot %llu lies outside the blocks", what, (unsigned long long)slot);
      if (slot < blocks * 64) {
        CHECK(!used[slot], "%s: slot %llu is the slot of two ordinals", what, (unsigned long long)slot);
        used[slot] = 1;
      }
      CHECK(vi::refine_slot(first[l], p) == slot, "%s: (list, position) and ordinal disagree at %llu", what, (unsigned long long)ord);
    }
  CHECK(ord == n, "%s: ordinals counted", what);
  // pad slots are no ordinal's slot
  uint64_t marked = 0;
  for (uint64_t s = 0; s < blocks * 64; ++s) marked += used[s];
  CHECK(marked == n, "%s: %llu slots carry a record, %llu records", what, (unsigned long long)marked, (unsigned long long)n);
}

static void check_means() {
  // values whose sum depends on the order: a chain is not a pairwise sum
  const uint32_t counts[] = {1, 2, 63, 64, 65, 1000, 4097};
  for (const uint32_t count : counts)
    for (const uint64_t stride : {(uint64_t)1, (uint64_t)3}) {
      std::vector<float> col(count * stride, -7.0f);
      uint32_t s = 12345u + count;
      for (uint32_t i = 0; i < count; ++i) {
        s = s * 1664525u + 1013904223u;
        col[i * stride] = ((float)(s >> 8) / 16777216.0f - 0.5f) * (i % 7 == 0 ? 1.0e4f : 1.0f) + 100.0f;
      }
      volatile float acc = 0.0f;  // (one rounded f32 add per member, whatever the optimiser would like)
      for (uint32_t i = 0; i < count; ++i) acc = acc + col[i * stride];
      const float want = acc / (float)count;
      const float got = vi::refine_chain_mean(col.data(), stride, count);
      CHECK(std::memcmp(&want, &got, 4) == 0, "mean of %u members at stride %llu: %a, the plain loop gives %a", count,
            (unsigned long long)stride, got, want);
      // the two steps a kernel takes, tile by tile
      float a2 = 0.0f;
      for (uint32_t base = 0; base < count; base += 64)
        for (uint32_t v = base; v < count && v < base + 64; ++v) a2 = vi::refine_chain_add(a2, col[v * stride]);
      const float got2 = vi::refine_mean(a2, count);
      CHECK(std::memcmp(&want, &got2, 4) == 0, "tiled chain of %u members: %a, the plain loop gives %a", count, got2, want);
    }
  // the chain starts from +0.0: a list of -0.0 rows has the mean +0.0
  const float negz[3] = {-0.0f, -0.0f, -0.0f};
  const float m = vi::refine_chain_mean(negz, 1, 3);
  CHECK(m == 0.0f && !std::signbit(m), "the mean of -0.0 rows is %a", m);
}

static void check_fixed_point() {
  const float a[4] = {1.0f, -0.0f, 3.5f, 0.0f}, b[4] = {1.0f, 0.0f, 3.5f, 0.0f};
  uint32_t wa[4], wb[4];
  std::memcpy(wa, a, 16);
  std::memcpy(wb, b, 16);
  CHECK(vi::refine_changed_words(wa, wa, 4) == 0, "a table equals itself");
  CHECK(vi::refine_changed_words(wa, wb, 4) == 1, "-0.0 and +0.0 are different bits");
  CHECK(vi::refine_fixed_point(0, 0), "nothing moved, nothing changed: a fixed point");
  CHECK(!vi::refine_fixed_point(1, 0), "a moved record is no fixed point");
  CHECK(!vi::refine_fixed_point(0, 1), "a changed word is no fixed point");
}

static void check_imbalance() {
  const std::vector<uint32_t> uniform(20, 137), empty(5, 0);
  CHECK(vi::refine_imbalance(uniform.data(), uniform.size()) == 1.0, "equal lengths: %f", vi::refine_imbalance(uniform.data(), 20));
  for (const uint32_t k : {1u, 2u, 20u, 4096u}) {
    std::vector<uint32_t> one(k, 0);
    one[k / 2] = 100000;
    CHECK(vi::refine_imbalance(one.data(), k) == (double)k, "everything in one list of %u: %f", k, vi::refine_imbalance(one.data(), k));
  }
  const std::vector<uint32_t> mixed = {1, 2, 3, 4};  // 4 * 30 / 100
  CHECK(vi::refine_imbalance(mixed.data(), 4) == 1.2, "lengths 1 2 3 4: %f", vi::refine_imbalance(mixed.data(), 4));
  CHECK(vi::refine_imbalance(empty.data(), 5) == 0.0, "no record: 0");
  CHECK(vi::refine_imbalance(nullptr, 0) == 0.0, "no list: 0");
  const std::vector<uint32_t> big(3, 0xFFFFFFF0u);  // squares past 2^64: the sums are doubles
  CHECK(std::fabs(vi::refine_imbalance(big.data(), 3) - 1.0) < 1e-12, "three lists of 2^32 - 16");
}

int main() {
  check_layout<uint64_t>({1, 63, 64, 65, 4097}, "1 63 64 65 4097");
  check_layout<uint64_t>({0, 0, 1, 0, 63, 64, 0, 0, 65, 4097, 0}, "with empty lists");
  check_layout<uint32_t>({4097, 0, 65, 64, 63, 1, 0}, "descending, u32 prefix");
  check_layout<uint64_t>({0, 0, 0, 5}, "leading empties");
  check_layout<uint64_t>({5, 0, 0, 0}, "trailing empties");
  check_layout<uint64_t>({7}, "one list");
  check_means();
  check_fixed_point();
  check_imbalance();
  return failures ? 1 : 0;
}
