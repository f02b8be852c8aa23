// record_order_check.cpp — host checks of the two rules of csrc/list_layout.hpp that reading records back rests on
// (compiled and run by test_record_order_cpu.py): full_position, a rank's local position -> the position in the full
// list, and list_of_block, the list that owns a resident block.  Prints one line per failed check and exits non-zero if
// there was one.
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

// over the ranks of a world, the local positions of a list of n vectors map onto 0 .. n-1, each exactly once, ascending
// on every rank, and a position keeps its lane (p % 64)
static void check_positions() {
  for (uint32_t world = 1; world <= 5; ++world)
    for (uint64_t n = 0; n <= 400; ++n) {
      std::vector<uint32_t> seen(n, 0);
      uint64_t total = 0;
      for (uint32_t rank = 0; rank < world; ++rank) {
        const uint64_t ll = local_len(n, world, rank), lb = local_blocks(n, world, rank);
        CHECK(ll <= lb * 64 && (lb == 0 || ll > (lb - 1) * 64), "n %llu world %u rank %u: %llu vectors in %llu blocks",
              (unsigned long long)n, world, rank, (unsigned long long)ll, (unsigned long long)lb);
        uint64_t prev = 0;
        for (uint64_t p = 0; p < ll; ++p) {
          const uint64_t fp = full_position(p, world, rank);
          CHECK(fp < n, "n %llu world %u rank %u: local %llu -> %llu", (unsigned long long)n, world, rank, (unsigned long long)p,
                (unsigned long long)fp);
          CHECK(p == 0 || fp > prev, "n %llu world %u rank %u: local %llu -> %llu after %llu", (unsigned long long)n, world, rank,
                (unsigned long long)p, (unsigned long long)fp, (unsigned long long)prev);
          CHECK(fp % 64 == p % 64 && (fp / 64) % world == rank, "n %llu world %u rank %u: local %llu -> %llu: lane or owner",
                (unsigned long long)n, world, rank, (unsigned long long)p, (unsigned long long)fp);
          if (fp < n) ++seen[fp];
          prev = fp;
        }
        total += ll;
      }
      CHECK(total == n, "n %llu world %u: %llu local positions", (unsigned long long)n, world, (unsigned long long)total);
      for (uint64_t fp = 0; fp < n; ++fp)
        CHECK(seen[fp] == 1, "n %llu world %u: position %llu produced %u times", (unsigned long long)n, world,
              (unsigned long long)fp, seen[fp]);
    }
  CHECK(full_position(12345, 1, 0) == 12345, "world 1 is not the identity");
}

// every resident block of a layout is owned by the list whose span [first, first + blocks) holds it, whatever runs of
// empty lists lie before, between and behind
static void check_owner(const std::vector<uint64_t> &lens, uint32_t world, uint32_t rank, const char *what) {
  ListLayout lay;
  CHECK(plan_list_layout(lens.data(), lens.size(), world, rank, &lay) == LayoutError::none, "%s: layout error", what);
  uint64_t found = 0;
  for (uint64_t l = 0; l < lens.size(); ++l)
    for (uint64_t b = 0; b < local_blocks(lens[l], world, rank); ++b, ++found) {
      const uint32_t got = list_of_block(lay.first.data(), (uint32_t)lens.size(), lay.first[l] + (uint32_t)b);
      CHECK(got == l, "%s world %u rank %u: block %llu of list %llu is given to list %u", what, world, rank,
            (unsigned long long)b, (unsigned long long)l, got);
    }
  CHECK(found == lay.total_blocks, "%s world %u rank %u: %llu blocks visited of %llu", what, world, rank,
        (unsigned long long)found, (unsigned long long)lay.total_blocks);
}

static void check_owners() {
  const std::vector<std::vector<uint64_t>> layouts = {
      {1, 63, 64, 65, 0, 0, 200, 0, 129},
      {0, 0, 0, 5, 0, 0, 0},
      {0, 64},
      {64, 0},
      {1},
      {0, 0, 130, 0, 0, 0, 1, 0, 0, 700, 0},
      {400, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1},
  };
  for (const auto &lens : layouts)
    for (uint32_t world = 1; world <= 5; ++world)
      for (uint32_t rank = 0; rank < world; ++rank) check_owner(lens, world, rank, "layout");
  std::vector<uint64_t> many(1000);
  for (size_t l = 0; l < many.size(); ++l) many[l] = l % 7 == 3 ? 0 : (l * 37) % 300;
  for (uint32_t world = 1; world <= 3; ++world)
    for (uint32_t rank = 0; rank < world; ++rank) check_owner(many, world, rank, "1000 lists");
}

int main() {
  check_positions();
  check_owners();
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
