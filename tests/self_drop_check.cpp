// self_drop_check.cpp — the index, count and absent-row rules of csrc/self_drop.hpp against a brute-force "erase the
// record's own entry, then truncate to k": every input width 1 .. 130 (k = width - 1), every match position and none,
// every found count 0 .. width.  Includes only that header; prints one line per failed check, exit status 1 if any.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "self_drop.hpp"

int main() {
  int bad = 0;
  auto check = [&](bool ok, const char *what, uint32_t w, uint32_t s, uint32_t f) {
    if (!ok && ++bad <= 20) std::printf("FAIL %s: width %u match %d found %u\n", what, w, (int)s, f);
  };
  const uint32_t kPad = 0xFFFFFFFFu;
  for (uint32_t w = 1; w <= 130; ++w) {
    const uint32_t k = w - 1;
    for (uint32_t f = 0; f <= w; ++f) {                 // entries of the input row that hold a candidate
      for (uint32_t sm = 0; sm <= f; ++sm) {            // the match among them; sm == f: none
        const bool match = sm < f;
        const uint32_t s = match ? sm : vi::kSelfDropNoMatch;
        std::vector<uint32_t> in(w), want, got(k);
        for (uint32_t j = 0; j < w; ++j) in[j] = j < f ? 1000u + j : kPad;
        want = in;
        if (match) want.erase(want.begin() + sm);
        want.resize(k, kPad);
        uint32_t want_count = 0;
        for (uint32_t j = 0; j < k; ++j) want_count += want[j] != kPad;
        bool in_range = true;
        for (uint32_t j = 0; j < k; ++j) {
          const uint32_t src = vi::self_drop_src(j, s);
          if (src >= w) { in_range = false; break; }
          got[j] = in[src];
        }
        check(in_range, "source index inside the input row", w, s, f);
        if (in_range) check(got == want, "row", w, s, f);
        check(vi::self_drop_count(f, match, k) == want_count, "count", w, s, f);
      }
    }
  }
  for (uint32_t c = 0; c < 5; ++c) check(vi::self_drop_row_absent(c) == (c == 0), "absent row", 0, 0, c);
  check(vi::self_drop_row_absent(0xFFFFFFFFu) == false, "absent row", 0, 0, 0xFFFFFFFFu);
  return bad ? 1 : 0;
}
