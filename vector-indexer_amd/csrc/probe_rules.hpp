// probe_rules.hpp — the rule by which adaptive probing (probe_prune.hip) shortens a query's probe row: how many of its
// probes stay, and the candidate-order ranks of those that do.  Nothing of HIP is included, so a host program can run the
// very same functions on plain arrays (tests/probe_rules_check.cpp); probe_prune_kernel calls the pieces with one lane
// per probe and wave-wide counts in place of the loops of prune_probe_row below.
//
// A row has `found` real probes l_0 .. l_{found-1} in coarse order (ascending (distance, index)), followed by the empty
// marker; d_r is the reference's coarse distance of probe r, len_r the full length of its list, order_r its
// candidate-order rank (a permutation of 0 .. found-1).  The probes kept are the prefix of length
//
//     p = clamp(min(p_ratio, p_codes, p_explicit),  lo = min(max(min_probe, 1), found),  hi = found)
//
//   p_ratio    = #{ r < found : d_r <= t },  t = fl32(ratio2 * d_0): one rounded multiply, compared in f32.  ratio2 == 0: off.
//   p_codes    = the smallest p >= 1 with len_0 + .. + len_{p-1} >= max_codes (the list that crosses the budget is still
//                scanned: Faiss's IndexIVF.max_codes), `found` if the sum never gets there.  max_codes == 0: off.
//   p_explicit = the caller's own count for this query.  kProbeNoLimit: off.
//
// A prefix of a probe row is the probe row of a smaller n_probe, and the shard visiting order restricted to a prefix is
// the prefix's own: the ranks of the kept probes are the old ranks closed up, order'_r = #{ r' < p : order_r' < order_r }.
// A rule of zeros keeps every probe and every rank; pruning a pruned row with the same rule changes nothing.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VI_PROBE_FN __host__ __device__ inline
#else
#define VI_PROBE_FN inline
#endif

namespace vi {

constexpr uint32_t kProbeMarker = 0xFFFFFFFFu;   // an empty place of a probe row, and the rank that goes with it
constexpr uint32_t kProbeNoLimit = 0xFFFFFFFFu;  // p_explicit of a query without a count of its own

struct ProbeRule {  // vi_probe_rule without the per-query counts
  uint32_t min_probe;  // 0 => 1
  float ratio2;        // 0 = off; else finite and >= 1
  uint64_t max_codes;  // 0 = off
};

// a ratio a rule may carry: 0, or finite and >= 1 (a NaN fails every comparison)
VI_PROBE_FN bool probe_ratio_legal(float ratio2) { return ratio2 == 0.0f || (ratio2 >= 1.0f && ratio2 <= 3.402823466e+38f); }

// t = fl32(ratio2 * d_0): exactly one rounding, never fused into a neighbour
VI_PROBE_FN float probe_threshold(float ratio2, float d0) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __fmul_rn(ratio2, d0);
#else
  volatile float t = ratio2 * d0;  // (rounded to f32 here whatever the host's evaluation method)
  return t;
#endif
}

// probe r counts towards p_ratio
VI_PROBE_FN bool probe_within_ratio(float d, float t) { return d <= t; }

// the lists up to and including this one (their lengths sum to `codes`) use the budget up
VI_PROBE_FN bool probe_budget_met(uint64_t codes, uint64_t max_codes) { return codes >= max_codes; }

// the number of probes kept, from the three counts (each `found` where its rule is off)
VI_PROBE_FN uint32_t probe_keep_count(uint32_t found, uint32_t p_ratio, uint32_t p_codes, uint32_t p_explicit, uint32_t min_probe) {
  uint32_t p = p_ratio < p_codes ? p_ratio : p_codes;
  if (p_explicit < p) p = p_explicit;
  uint32_t lo = min_probe > 1u ? min_probe : 1u;
  if (lo > found) lo = found;
  if (p < lo) p = lo;
  return p < found ? p : found;
}

// The closed-up rank of a kept probe whose old rank is g, from a bitmap of the kept probes' old ranks: seen[w] bit b is
// rank 32 w + b, before[w] the bits set in words below w.
VI_PROBE_FN uint32_t probe_popcount(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__popc(x);
#else
  uint32_t n = 0;
  for (; x; x &= x - 1u) ++n;
  return n;
#endif
}
VI_PROBE_FN uint32_t probe_closed_rank(const uint32_t *seen, const uint32_t *before, uint32_t g) {
  return before[g >> 5] + probe_popcount(seen[g >> 5] & ((1u << (g & 31u)) - 1u));
}

// One row, one thread: what probe_prune_kernel does with a wave.  probes / order: P words each, rewritten in place; d /
// len: per place of the row, read at real probes only (d where the ratio is on, len where the budget is).  scratch:
// 2 * ((P + 31) / 32) words.  Returns p.
VI_PROBE_FN uint32_t prune_probe_row(uint32_t P, uint32_t *probes, uint32_t *order, const float *d, const uint32_t *len,
                                     const ProbeRule &rule, uint32_t p_explicit, uint32_t *scratch) {
  const uint32_t words = (P + 31u) / 32u;
  uint32_t *seen = scratch, *before = scratch + words;
  uint32_t found = 0;
  while (found < P && probes[found] != kProbeMarker) ++found;
  uint32_t p_ratio = found, p_codes = found;
  if (rule.ratio2 != 0.0f && found) {
    const float t = probe_threshold(rule.ratio2, d[0]);
    p_ratio = 0;
    for (uint32_t r = 0; r < found; ++r) p_ratio += probe_within_ratio(d[r], t) ? 1u : 0u;
  }
  if (rule.max_codes != 0) {
    uint64_t codes = 0;
    for (uint32_t r = 0; r < found; ++r) {
      codes += len[r];
      if (probe_budget_met(codes, rule.max_codes)) { p_codes = r + 1u; break; }
    }
  }
  const uint32_t p = probe_keep_count(found, p_ratio, p_codes, p_explicit, rule.min_probe);
  for (uint32_t w = 0; w < words; ++w) seen[w] = 0u;
  for (uint32_t r = 0; r < p; ++r) seen[order[r] >> 5] |= 1u << (order[r] & 31u);
  for (uint32_t w = 0, run = 0; w < words; ++w) { before[w] = run; run += probe_popcount(seen[w]); }
  for (uint32_t r = 0; r < P; ++r) {
    const bool keep = r < p;
    order[r] = keep ? probe_closed_rank(seen, before, order[r]) : kProbeMarker;
    if (!keep) probes[r] = kProbeMarker;
  }
  return p;
}

}  // namespace vi
