// self_drop.hpp — the rules by which a search by stored record (similar_search.hip) takes the (k + 1)-wide row its search
// produced to the caller's k-wide row: which input entry an output entry is, how many entries the row then holds, and
// when a row is padding altogether — and, further down, the same for the ragged rows of its radius form.  Nothing of HIP
// is included, so a host program can test the rules (tests/self_drop_check.cpp, tests/range_drop_check.cpp); the kernels
// call the very same functions.
//
// Why this is exact: the input row is the first k + 1 entries of the reference's stably sorted candidate sequence.  The
// record itself is one entry of that sequence (its slot is unique).  Deleting one entry of a sorted sequence leaves the
// others in their order, so the first k entries of the sequence without it are the first k + 1 entries with it, less that
// entry if it is among them — and the first k of them if it is not.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VI_SELF_DROP_FN __host__ __device__ inline
#else
#define VI_SELF_DROP_FN inline
#endif

namespace vi {

constexpr uint32_t kSelfDropNoMatch = 0xFFFFFFFFu;  // no entry of the row is the record itself

// output entry j (j < k) is input entry j + (j >= s); s: the position of the record's own entry, or kSelfDropNoMatch
VI_SELF_DROP_FN uint32_t self_drop_src(uint32_t j, uint32_t s) { return j + (j >= s ? 1u : 0u); }

// entries of the output row that hold a neighbour: found_in_row of the k + 1 input entries did
VI_SELF_DROP_FN uint32_t self_drop_count(uint32_t found_in_row, bool match, uint32_t k) {
  const uint32_t left = found_in_row - (match && found_in_row ? 1u : 0u);
  return left < k ? left : k;
}

// a row whose id no resident record carries is written as padding, whatever the search of its zero-filled query returned
VI_SELF_DROP_FN bool self_drop_row_absent(uint32_t records_carrying_id) { return records_carrying_id == 0u; }

// ---- the ragged form: a radius search by stored record (range_find_kernel / range_move_kernel) ----
// The input is a CSR row of `len` entries, the whole of the reference's stably sorted sequence up to the radius.  The
// record itself is at most one entry of it, and deleting one entry of a sorted sequence leaves the others in their order
// and on their side of the radius: the output row is the input row less that entry, nothing else moves in or out.

// entries of the output row; match: one of the len entries is the record itself; absent: no record carries the row's id
VI_SELF_DROP_FN uint32_t range_drop_len(uint32_t len, bool match, bool absent) {
  return absent ? 0u : len - (match && len ? 1u : 0u);
}

// where output entry j (j < range_drop_len) of a row is read: in0 is the row's first input entry, s as for self_drop_src
VI_SELF_DROP_FN uint64_t range_drop_src(uint64_t in0, uint32_t j, uint32_t s) { return in0 + self_drop_src(j, s); }

}  // namespace vi
