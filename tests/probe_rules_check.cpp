// Stand-alone host check of csrc/probe_rules.hpp: the rule by which adaptive probing shortens a probe row, run on plain
// arrays against a brute-force restatement of the definition.  Prints one line per failed check and exits non-zero if
// there was one.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "probe_rules.hpp"

static int failures = 0;

static void fail(const char *what, const char *which, uint32_t a, uint32_t b) {
  std::printf("FAILED %s (%s): %u %u\n", what, which, a, b);
  ++failures;
}

struct Row {
  uint32_t P;
  std::vector<uint32_t> probes, order, len;  // probes: `found` real ones, then markers
  std::vector<float> d;
};

// the definition, restated: every count by its own formula, nothing shared with the header but the marker's value
struct Expected { uint32_t p; std::vector<uint32_t> probes, order; };
static Expected brute(const Row &row, const vi::ProbeRule &rule, uint32_t p_explicit) {
  uint32_t found = 0;
  for (uint32_t r = 0; r < row.P; ++r) found += row.probes[r] != 0xFFFFFFFFu ? 1u : 0u;
  uint32_t p_ratio = found, p_codes = found;
  if (rule.ratio2 != 0.0f && found) {
    const float t = (float)((double)rule.ratio2 * (double)row.d[0]);  // (a product of two f32 is exact in f64: one rounding)
    p_ratio = (uint32_t)std::count_if(row.d.begin(), row.d.begin() + found, [&](float d) { return d <= t; });
  }
  if (rule.max_codes != 0)
    for (uint32_t p = 1; p <= found; ++p)
      if (std::accumulate(row.len.begin(), row.len.begin() + p, (uint64_t)0) >= rule.max_codes) { p_codes = p; break; }
  const uint32_t lo = std::min(std::max(rule.min_probe, 1u), found);
  const uint32_t p = std::min(std::max(std::min({p_ratio, p_codes, p_explicit}), lo), found);
  Expected e{p, std::vector<uint32_t>(row.P, 0xFFFFFFFFu), std::vector<uint32_t>(row.P, 0xFFFFFFFFu)};
  for (uint32_t r = 0; r < p; ++r) {
    e.probes[r] = row.probes[r];
    uint32_t below = 0;
    for (uint32_t s = 0; s < p; ++s) below += row.order[s] < row.order[r] ? 1u : 0u;
    e.order[r] = below;
  }
  return e;
}

static uint32_t run(Row &row, const vi::ProbeRule &rule, uint32_t p_explicit) {
  std::vector<uint32_t> scratch(2 * ((row.P + 31u) / 32u) + 1, 0xDEADBEEFu);
  const uint32_t p = vi::prune_probe_row(row.P, row.probes.data(), row.order.data(), row.d.data(), row.len.data(), rule, p_explicit,
                                         scratch.data());
  if (scratch.back() != 0xDEADBEEFu) fail("scratch overrun", "", row.P, 0);
  return p;
}

static void check(const char *what, const Row &row0, const vi::ProbeRule &rule, uint32_t p_explicit) {
  const Expected want = brute(row0, rule, p_explicit);
  Row row = row0;
  const uint32_t p = run(row, rule, p_explicit);
  if (p != want.p) fail(what, "p", p, want.p);
  if (row.probes != want.probes) fail(what, "probes", p, want.p);
  if (row.order != want.order) fail(what, "order", p, want.p);
  // the kept orders are a permutation of 0 .. p-1 that keeps the relative order of the old ranks
  std::vector<uint32_t> seen(p, 0);
  for (uint32_t r = 0; r < p; ++r) {
    if (row.order[r] >= p || seen[row.order[r]]++) fail(what, "permutation", r, row.order[r]);
    for (uint32_t s = 0; s < p; ++s)
      if ((row0.order[r] < row0.order[s]) != (row.order[r] < row.order[s])) fail(what, "relative order", r, s);
  }
  for (uint32_t r = p; r < row.P; ++r)
    if (row.probes[r] != vi::kProbeMarker || row.order[r] != vi::kProbeMarker) fail(what, "tail", r, p);
  // idempotence: the pruned row pruned again (its markers are no probes) stays as it is
  Row again = row;
  const uint32_t p2 = run(again, rule, p_explicit);
  if (p2 != p || again.probes != row.probes || again.order != row.order) fail(what, "idempotence", p2, p);
  // a rule of zeros keeps the pruned row as it is, too
  Row zero = row;
  const uint32_t p0 = run(zero, vi::ProbeRule{0, 0.0f, 0}, vi::kProbeNoLimit);
  if (p0 != p || zero.probes != row.probes || zero.order != row.order) fail(what, "zero rule", p0, p);
}

static Row make_row(uint32_t P, uint32_t found, std::mt19937 &rng) {
  Row row{P, std::vector<uint32_t>(P, vi::kProbeMarker), std::vector<uint32_t>(P, vi::kProbeMarker), std::vector<uint32_t>(P, 0),
          std::vector<float>(P, 0.0f)};
  std::vector<uint32_t> lists(4 * P + 8), ord(found);
  std::iota(lists.begin(), lists.end(), 0u);
  std::shuffle(lists.begin(), lists.end(), rng);
  std::iota(ord.begin(), ord.end(), 0u);
  std::shuffle(ord.begin(), ord.end(), rng);
  std::uniform_real_distribution<float> step(0.0f, 0.5f);
  float d = 0.25f + step(rng);
  for (uint32_t r = 0; r < found; ++r) {
    row.probes[r] = lists[r];
    row.order[r] = ord[r];
    row.len[r] = rng() % 300u;
    row.d[r] = d;
    d += (rng() % 4u) ? step(rng) : 0.0f;  // ascending, with ties
  }
  return row;
}

int main() {
  std::mt19937 rng(12345);
  const uint32_t founds[] = {0, 1, 63, 64, 65, 200};
  const vi::ProbeRule zero{0, 0.0f, 0};
  for (uint32_t found : founds)
    for (uint32_t pad : {0u, 1u, 70u}) {
      const uint32_t P = found + pad;
      if (P == 0) continue;
      for (int trial = 0; trial < 20; ++trial) {
        const Row row = make_row(P, found, rng);
        const uint64_t total = std::accumulate(row.len.begin(), row.len.end(), (uint64_t)0);
        // a rule of zeros prunes nothing
        {
          Row r = row;
          const uint32_t p = run(r, zero, vi::kProbeNoLimit);
          if (p != found || r.probes != row.probes || r.order != row.order) fail("zero rule on a fresh row", "", p, found);
        }
        const float ratios[] = {1.0f, 1.0f + 1.0f / 8388608.0f, 1.5f, 2.0f, 7.25f, 1.0e30f};
        for (float ratio2 : ratios) check("ratio", row, vi::ProbeRule{0, ratio2, 0}, vi::kProbeNoLimit);
        for (uint64_t mc : {(uint64_t)1, total / 3 + 1, total, total + 1, (uint64_t)1 << 40}) check("max_codes", row, vi::ProbeRule{0, 0.0f, mc}, vi::kProbeNoLimit);
        for (uint32_t pe : {0u, 1u, found / 2, found, found + 1, found + 1000u}) check("explicit", row, zero, pe);
        for (uint32_t mp : {0u, 1u, 3u, found, found + 5u}) check("min_probe", row, vi::ProbeRule{mp, 1.0f, 1}, 0u);
        check("all three", row, vi::ProbeRule{2, 1.75f, total / 2 + 1}, found ? found - found / 3 : 0u);
        if (found == 0) continue;
        // t exactly equal to some d_r: ratio2 = 2, d_r = 2 d_0 is exact
        {
          Row r = row;
          const uint32_t at = found / 2;
          for (uint32_t i = 0; i < at; ++i) r.d[i] = std::min(r.d[i], 2.0f * r.d[0]);
          for (uint32_t i = at; i < found; ++i) r.d[i] = std::max(r.d[i], 2.0f * r.d[0]);
          r.d[at] = 2.0f * r.d[0];
          if (at + 1 < found) r.d[at + 1] = std::nextafter(2.0f * r.d[0], std::numeric_limits<float>::infinity());
          for (uint32_t i = at + 2; i < found; ++i) r.d[i] = std::max(r.d[i], r.d[at + 1]);
          check("t equals a distance", r, vi::ProbeRule{0, 2.0f, 0}, vi::kProbeNoLimit);
          Row pr = r;
          const uint32_t p = run(pr, vi::ProbeRule{0, 2.0f, 0}, vi::kProbeNoLimit);
          if (at > 0 && p != at + 1) fail("t equals a distance", "the equal one is kept, the next is not", p, at + 1);
        }
        // d_0 == 0: t == 0 keeps exactly the centroids at distance bits 0
        {
          Row r = row;
          const uint32_t zeros = 1 + rng() % std::min(found, 3u);
          for (uint32_t i = 0; i < zeros; ++i) r.d[i] = 0.0f;
          for (uint32_t i = zeros; i < found; ++i) r.d[i] = std::max(r.d[i], 1.0e-30f);
          check("d_0 == 0", r, vi::ProbeRule{0, 3.0f, 0}, vi::kProbeNoLimit);
          Row pr = r;
          const uint32_t p = run(pr, vi::ProbeRule{0, 3.0f, 0}, vi::kProbeNoLimit);
          if (p != zeros) fail("d_0 == 0", "count", p, zeros);
        }
        // all distances equal: the ratio keeps them all
        {
          Row r = row;
          for (uint32_t i = 0; i < found; ++i) r.d[i] = 3.5f;
          check("all distances equal", r, vi::ProbeRule{0, 1.0f, 0}, vi::kProbeNoLimit);
          Row pr = r;
          if (run(pr, vi::ProbeRule{0, 1.0f, 0}, vi::kProbeNoLimit) != found) fail("all distances equal", "count", 0, found);
        }
        // a budget reached exactly at a list boundary: that list is the last one kept; and one never reached
        {
          const uint32_t at = found / 2;
          const uint64_t upto = std::accumulate(row.len.begin(), row.len.begin() + at + 1, (uint64_t)0);
          if (upto) {
            check("budget at a boundary", row, vi::ProbeRule{0, 0.0f, upto}, vi::kProbeNoLimit);
            Row pr = row;
            const uint32_t p = run(pr, vi::ProbeRule{0, 0.0f, upto}, vi::kProbeNoLimit);
            uint32_t first = 0;
            for (uint64_t s = 0; first < found; ++first) { s += row.len[first]; if (s >= upto) break; }
            if (p != first + 1) fail("budget at a boundary", "count", p, first + 1);
          }
          Row pr = row;
          if (run(pr, vi::ProbeRule{0, 0.0f, total + 1}, vi::kProbeNoLimit) != found) fail("budget never reached", "count", 0, found);
        }
      }
    }
  // which ratios a rule may carry
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  if (!vi::probe_ratio_legal(0.0f) || !vi::probe_ratio_legal(1.0f) || !vi::probe_ratio_legal(3.0e38f)) fail("legal ratios", "", 0, 0);
  if (vi::probe_ratio_legal(nan) || vi::probe_ratio_legal(inf) || vi::probe_ratio_legal(-1.0f) || vi::probe_ratio_legal(0.5f) ||
      vi::probe_ratio_legal(-inf) || vi::probe_ratio_legal(std::nextafter(1.0f, 0.0f)))
    fail("illegal ratios", "", 0, 0);
  return failures ? 1 : 0;
}
