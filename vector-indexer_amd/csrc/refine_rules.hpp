// refine_rules.hpp — the rules of vi_indexer_refine (list_refine.hip) that are plain arithmetic: where a list-order
// ordinal lies in the resident blocks, how one column of a list's centre is summed and divided, when an iteration is a
// fixed point, and the imbalance factor of a set of list lengths.  Nothing of HIP is included, so a host program runs the
// very same functions on plain arrays (tests/refine_rules_check.cpp); the kernels call them as they stand.
//
// Ordinals.  The records of an index in list order — lists ascending, positions ascending, pad slots skipped — are
// numbered 0..n-1.  prefix[l] is the ordinal of list l's first record (the exclusive prefix of the lengths; an empty list
// shares its prefix with the list behind it).  A list's blocks are consecutive, so
//   ordinal -> (list, position): list = the LAST l with prefix[l] <= ordinal, position = ordinal - prefix[list]
//   (list, position) -> slot:    64 * first_block[list] + position
// The last such l is the one that holds the record: the empty lists in front of it have the same prefix and a lower index.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VI_REFINE_FN __host__ __device__ inline
#else
#define VI_REFINE_FN inline
#endif

namespace vi {

// the list that holds `ordinal` (< the sum of the lengths): the last l in [0, nlists) with prefix[l] <= ordinal.
// prefix[0] == 0, so there always is one.  P: uint32_t or uint64_t words.
template <typename P>
VI_REFINE_FN uint32_t refine_list_of_ordinal(const P *prefix, uint32_t nlists, uint64_t ordinal) {
  uint32_t lo = 0, hi = nlists;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)prefix[mid] <= ordinal) lo = mid; else hi = mid;
  }
  return lo;
}

// slot of position `pos` of a list whose first block is first_block
VI_REFINE_FN uint64_t refine_slot(uint32_t first_block, uint64_t pos) { return (uint64_t)first_block * 64u + pos; }

// slot of a list-order ordinal
template <typename P>
VI_REFINE_FN uint64_t refine_slot_of_ordinal(const P *prefix, const uint32_t *first_block, uint32_t nlists, uint64_t ordinal) {
  const uint32_t l = refine_list_of_ordinal(prefix, nlists, ordinal);
  return refine_slot(first_block[l], ordinal - (uint64_t)prefix[l]);
}

// One column of a centre (update_centroids_parallel, src/kmeans.rs:690-703): a chain of f32 adds from +0.0 over the
// list's members in list order, then one f32 divide by the member count.  The two steps, so that a kernel that meets the
// members tile by tile runs the same chain: no pairwise sum, no fused multiply-add (there is no multiply to fuse).
VI_REFINE_FN float refine_chain_add(float acc, float x) { return acc + x; }
VI_REFINE_FN float refine_mean(float sum, uint32_t count) { return sum / (float)count; }
// ... and the chain over a strided column of `count` members, as a host reads it
VI_REFINE_FN float refine_chain_mean(const float *column, uint64_t stride, uint32_t count) {
  float acc = 0.0f;
  for (uint32_t i = 0; i < count; ++i) acc = refine_chain_add(acc, column[(uint64_t)i * stride]);
  return refine_mean(acc, count);
}

// An iteration is a fixed point when it moved no record and left every word of the table as it was: every later
// iteration would then compute the same centres from the same lists and the same labels from the same centres.
VI_REFINE_FN uint64_t refine_changed_words(const uint32_t *table_bits, const uint32_t *new_bits, uint64_t words) {
  uint64_t changed = 0;
  for (uint64_t i = 0; i < words; ++i) changed += table_bits[i] != new_bits[i];
  return changed;
}
VI_REFINE_FN bool refine_fixed_point(uint64_t moved, uint64_t changed_words) { return moved == 0 && changed_words == 0; }

// Faiss's imbalance factor of an inverted file: lists * sum(len^2) / sum(len)^2, in double.  1 for equal lengths, the
// number of lists when one list holds everything; 0 for an index without a record.
VI_REFINE_FN double refine_imbalance(const uint32_t *len, uint64_t nlists) {
  double tot = 0.0, sq = 0.0;
  for (uint64_t l = 0; l < nlists; ++l) {
    tot += (double)len[l];
    sq += (double)len[l] * (double)len[l];
  }
  return tot > 0.0 ? (double)nlists * sq / (tot * tot) : 0.0;
}

}  // namespace vi
