// range_drop_check.cpp — the ragged rules of csrc/self_drop.hpp (range_drop_len, range_drop_src), applied to whole CSRs
// the way range_find_kernel / range_move_kernel apply them, against a brute-force "erase the record's own entry of every
// row, drop the rows of absent ids, concatenate": every row length 0 .. 130 with every match position and none, absent
// rows first, in the middle and last, CSRs of empty rows only, and a few thousand random CSRs.  Includes only that
// header; prints one line per failed check, exit status 1 if any.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "self_drop.hpp"

namespace {

struct Row {
  uint32_t len;
  uint32_t match;  // position of the own entry, or vi::kSelfDropNoMatch
  bool absent;
};

int bad = 0;

void fail_line(const char *what, const char *name, size_t row) {
  if (++bad <= 20) std::printf("FAIL %s: case %s row %zu\n", what, name, row);
}

// builds the input CSR of `rows` (distinct values everywhere), applies the rule as the two kernels do — lengths first,
// then an exclusive scan (range_result_place), then the move — and compares with erase-and-concatenate
void check_csr(const std::vector<Row> &rows, const char *name) {
  std::vector<uint64_t> in_lims(rows.size() + 1, 0);
  for (size_t q = 0; q < rows.size(); ++q) in_lims[q + 1] = in_lims[q] + rows[q].len;
  std::vector<uint64_t> in(in_lims.back());
  for (size_t e = 0; e < in.size(); ++e) in[e] = 0x100000000ull + e;

  std::vector<uint64_t> want;
  std::vector<uint64_t> want_lims(1, 0);
  for (size_t q = 0; q < rows.size(); ++q) {
    std::vector<uint64_t> r(in.begin() + in_lims[q], in.begin() + in_lims[q + 1]);
    if (rows[q].absent) r.clear();
    else if (rows[q].match != vi::kSelfDropNoMatch) r.erase(r.begin() + rows[q].match);
    want.insert(want.end(), r.begin(), r.end());
    want_lims.push_back(want.size());
  }

  std::vector<uint64_t> out_lims(rows.size() + 1, 0);
  for (size_t q = 0; q < rows.size(); ++q)
    out_lims[q + 1] = out_lims[q] + vi::range_drop_len(rows[q].len, rows[q].match != vi::kSelfDropNoMatch, rows[q].absent);
  if (out_lims != want_lims) { fail_line("lims", name, 0); return; }
  const uint64_t kUnwritten = ~0ull;
  std::vector<uint64_t> out(out_lims.back(), kUnwritten);
  for (size_t q = 0; q < rows.size(); ++q) {
    const uint32_t n = (uint32_t)(out_lims[q + 1] - out_lims[q]);
    for (uint32_t j = 0; j < n; ++j) {
      const uint64_t src = vi::range_drop_src(in_lims[q], j, rows[q].match);
      if (src < in_lims[q] || src >= in_lims[q + 1]) { fail_line("source index inside the input row", name, q); return; }
      out[out_lims[q] + j] = in[src];
    }
  }
  if (out != want) fail_line("entries", name, 0);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {  // xorshift64*, [0, n)
  rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
  return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

}  // namespace

int main() {
  const uint32_t none = vi::kSelfDropNoMatch;
  // every length with every match position and none, as a row between two others
  for (uint32_t len = 0; len <= 130; ++len)
    for (uint32_t sm = 0; sm <= len; ++sm) {
      const uint32_t s = sm < len ? sm : none;
      check_csr({{3, 1, false}, {len, s, false}, {2, none, false}}, "length x match");
      check_csr({{len, s, false}}, "single row");
      check_csr({{len, s, true}, {len, s, false}, {len, s, false}}, "absent first");
      check_csr({{len, s, false}, {len, s, true}, {len, s, false}}, "absent middle");
      check_csr({{len, s, false}, {len, s, false}, {len, s, true}}, "absent last");
    }
  // one CSR of all of them in a row
  {
    std::vector<Row> all;
    for (uint32_t len = 0; len <= 130; ++len)
      for (uint32_t sm = 0; sm <= len; ++sm) all.push_back({len, sm < len ? sm : none, false});
    check_csr(all, "all lengths and matches");
  }
  // nothing but empty rows, present and absent; no rows at all
  check_csr(std::vector<Row>(17, Row{0, none, false}), "all empty");
  check_csr(std::vector<Row>(17, Row{0, none, true}), "all empty and absent");
  check_csr({}, "no rows");
  // an absent row never has a match to report, but its (zero query's) search may have returned entries
  check_csr({{5, none, true}, {0, none, true}, {70, none, true}}, "all absent");
  // the rule itself at its corners
  if (vi::range_drop_len(0, false, false) != 0 || vi::range_drop_len(1, true, false) != 0 || vi::range_drop_len(1, false, false) != 1 ||
      vi::range_drop_len(7, true, true) != 0)
    fail_line("range_drop_len", "corners", 0);
  // random CSRs: up to 40 rows of up to 300 entries, a tenth of the rows absent, two thirds of the others with a match
  for (int c = 0; c < 4000; ++c) {
    std::vector<Row> rows(rnd(41));
    for (Row &r : rows) {
      r.len = rnd(4) == 0 ? 0 : rnd(301);
      r.absent = rnd(10) == 0;
      r.match = (!r.absent && r.len && rnd(3) != 0) ? rnd(r.len) : none;
    }
    check_csr(rows, "random");
  }
  return bad ? 1 : 0;
}
