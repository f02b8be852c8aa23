// list_layout_check.cpp — host checks of csrc/list_layout.hpp (compiled and run by test_list_layout_cpu.py): prints one
// line per failed check and exits non-zero if there was one.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "list_layout.hpp"

using namespace vi;

static int failures = 0;

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      ++failures;                   \
      std::printf("FAIL %s: ", #cond); \
      std::printf(__VA_ARGS__);     \
      std::printf("\n");            \
    }                               \
  } while (0)

// blocks b = rank, rank + world, ... of a list of n vectors, counted one by one; the last block holds n - 64 b vectors
static void brute_stripe(uint64_t n, uint32_t world, uint32_t rank, uint64_t *blocks, uint64_t *len) {
  const uint64_t nb = (n + 63) / 64;
  *blocks = *len = 0;
  for (uint64_t b = 0; b < nb; ++b)
    if (b % world == rank) {
      ++*blocks;
      *len += (b == nb - 1) ? n - 64 * b : 64;
    }
}

static void check_stripes() {
  const uint64_t ns[] = {0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 100000};
  for (uint64_t n : ns)
    for (uint32_t world = 1; world <= 8; ++world) {
      uint64_t sum_blocks = 0, sum_len = 0;
      for (uint32_t rank = 0; rank < world; ++rank) {
        uint64_t wb, wl;
        brute_stripe(n, world, rank, &wb, &wl);
        const uint64_t gb = local_blocks(n, world, rank), gl = local_len(n, world, rank);
        CHECK(gb == wb, "local_blocks(%llu, %u, %u) = %llu, counted %llu", (unsigned long long)n, world, rank,
              (unsigned long long)gb, (unsigned long long)wb);
        CHECK(gl == wl, "local_len(%llu, %u, %u) = %llu, counted %llu", (unsigned long long)n, world, rank,
              (unsigned long long)gl, (unsigned long long)wl);
        sum_blocks += gb;
        sum_len += gl;
      }
      CHECK(sum_len == n, "n %llu world %u: lengths sum to %llu", (unsigned long long)n, world, (unsigned long long)sum_len);
      CHECK(sum_blocks == (n + 63) / 64, "n %llu world %u: blocks sum to %llu", (unsigned long long)n, world,
            (unsigned long long)sum_blocks);
    }
  CHECK(kListBlock == 64u, "block width %u", kListBlock);
}

static void check_planner() {
  const std::vector<uint64_t> lens = {0, 1, 64, 65, 0, 130};
  {
    ListLayout lay;
    const LayoutError e = plan_list_layout(lens.data(), lens.size(), 1, 0, &lay);
    CHECK(e == LayoutError::none, "world 1: error %d", (int)e);
    const std::vector<uint32_t> first = {0, 0, 1, 2, 4, 4}, len = {0, 1, 64, 65, 0, 130};
    CHECK(lay.first == first, "world 1: first blocks differ");
    CHECK(lay.len == len, "world 1: lengths differ");
    CHECK(lay.total_blocks == 7, "world 1: total_blocks %llu", (unsigned long long)lay.total_blocks);
    CHECK(lay.total_vec == 260, "world 1: total_vec %llu", (unsigned long long)lay.total_vec);
  }
  for (uint32_t rank = 0; rank < 3; ++rank) {
    ListLayout lay;
    const LayoutError e = plan_list_layout(lens.data(), lens.size(), 3, rank, &lay);
    CHECK(e == LayoutError::none, "world 3 rank %u: error %d", rank, (int)e);
    CHECK(lay.first.size() == lens.size() && lay.len.size() == lens.size(), "world 3 rank %u: array sizes", rank);
    uint64_t blocks = 0, vec = 0;
    for (size_t l = 0; l < lens.size() && l < lay.first.size() && l < lay.len.size(); ++l) {
      CHECK(lay.first[l] == blocks, "world 3 rank %u list %zu: first %u, want %llu", rank, l, lay.first[l], (unsigned long long)blocks);
      CHECK(lay.len[l] == local_len(lens[l], 3, rank), "world 3 rank %u list %zu: len %u", rank, l, lay.len[l]);
      blocks += local_blocks(lens[l], 3, rank);
      vec += local_len(lens[l], 3, rank);
    }
    CHECK(lay.total_blocks == blocks, "world 3 rank %u: total_blocks %llu, want %llu", rank, (unsigned long long)lay.total_blocks,
          (unsigned long long)blocks);
    CHECK(lay.total_vec == vec, "world 3 rank %u: total_vec %llu, want %llu", rank, (unsigned long long)lay.total_vec,
          (unsigned long long)vec);
  }
  {  // an index without lists
    ListLayout lay;
    CHECK(plan_list_layout(nullptr, 0, 1, 0, &lay) == LayoutError::none && lay.total_blocks == 0 && lay.first.empty(), "no lists");
  }
}

static void check_limits() {
  {  // slot limit: 0xFFFFFFFF / 64 = 67108863 blocks are one too many
    const uint64_t ok[] = {67108861ull * 64, 64}, over[] = {67108861ull * 64, 65};
    ListLayout lay;
    LayoutError e = plan_list_layout(ok, 2, 1, 0, &lay);
    CHECK(e == LayoutError::none, "67108862 blocks: error %d", (int)e);
    CHECK(lay.total_blocks == 67108862ull, "67108862 blocks: total_blocks %llu", (unsigned long long)lay.total_blocks);
    CHECK(lay.first.size() == 2 && lay.first[1] == 67108861u, "67108862 blocks: first block of the second list");
    e = plan_list_layout(over, 2, 1, 0, &lay);
    CHECK(e == LayoutError::too_many_slots, "67108863 blocks: error %d", (int)e);
  }
  {  // length limit
    const uint64_t at = 0xFFFFFFFFull - 64, past = 0xFFFFFFFFull - 63, huge = 1ull << 40;
    ListLayout lay;
    LayoutError e = plan_list_layout(&at, 1, 1, 0, &lay);
    CHECK(e == LayoutError::too_many_slots, "list of 2^32 - 65: error %d", (int)e);
    e = plan_list_layout(&past, 1, 1, 0, &lay);
    CHECK(e == LayoutError::list_too_long, "list of 2^32 - 64: error %d", (int)e);
    e = plan_list_layout(&huge, 1, 1, 0, &lay);
    CHECK(e == LayoutError::list_too_long, "list of 2^40: error %d", (int)e);
  }
}

int main() {
  check_stripes();
  check_planner();
  check_limits();
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
