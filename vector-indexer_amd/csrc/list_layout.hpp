// list_layout.hpp — where the lists of a resident index lie, as plain host arithmetic (standard library only: the rule and
// its limits are tested without a GPU, tests/test_list_layout_cpu.py).
//
// Lists lie back to back in list order, each padded to whole blocks of 64 vectors (device_index.hpp).  A slot is named by
// 32 bits (64 * block + lane) and a position inside a list by 32 bits as well: the two limits below.  With stripes (an
// index partitioned over `world` ranks) block b of a list lives on rank b % world, and every rank lays its own blocks
// out by the same rule; a local position p maps back to the list position ((p / 64) * world + rank) * 64 + p % 64.
#pragma once
#include <cstdint>
#include <vector>

namespace vi {

constexpr uint32_t kListBlock = 64;  // vectors per block: one lane of a wave each

// rank `rank`'s blocks of a list of n vectors: b = rank, rank + world, ...
inline uint64_t local_blocks(uint64_t n, uint32_t world, uint32_t rank) {
  const uint64_t nb = (n + kListBlock - 1) / kListBlock;
  return nb > rank ? (nb - rank + world - 1) / world : 0;
}
// ... and the vectors in them: only the last block of the list may be partial
inline uint64_t local_len(uint64_t n, uint32_t world, uint32_t rank) {
  const uint64_t nb = (n + kListBlock - 1) / kListBlock, lb = local_blocks(n, world, rank);
  if (lb == 0) return 0;
  const uint64_t last = rank + (lb - 1) * world;  // this rank's last block
  return (lb - 1) * kListBlock + (last == nb - 1 ? n - last * kListBlock : kListBlock);
}

// ---- reading a layout back (record_fetch.hip and tests/record_order_check.cpp share these two) ----
#if defined(__HIP__) || defined(__HIPCC__)
#define VI_LAYOUT_HD __host__ __device__
#else
#define VI_LAYOUT_HD
#endif

// the list position of local position p on rank `rank` of `world` (1, 0: the identity).  Monotone in p: a rank's local
// order of a list is its order in the full list.
VI_LAYOUT_HD inline uint64_t full_position(uint64_t p, uint32_t world, uint32_t rank) {
  return ((p / kListBlock) * world + rank) * kListBlock + p % kListBlock;
}
// the list that owns resident block `block` (block < total_blocks, nlists >= 1): a list without blocks here shares its
// `first` with the next list, so the owner is the LAST list with first[l] <= block
VI_LAYOUT_HD inline uint32_t list_of_block(const uint32_t *first, uint32_t nlists, uint32_t block) {
  uint32_t lo = 0, hi = nlists;  // first[lo] <= block < first[hi], with first[nlists] read as +infinity
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= block) lo = mid; else hi = mid;
  }
  return lo;
}

#if defined(__HIP__) || defined(__HIPCC__)
// ---- one pass over every resident slot: what builds a filter (slot_filter.hip) and matches a get's ids (record_fetch.hip) ----
struct ResidentLists { const uint32_t *first_block, *list_len; uint32_t nlists; };  // (a list not resident here: length 0)
constexpr uint32_t kListSplit = 8;  // workgroups sharing the blocks of one list (long lists carry most of an index)
inline dim3 slot_walk_grid(uint32_t nlists) { return dim3(nlists, kListSplit); }
// One wave per 64-vector block, four waves per workgroup, lane = vector of the block: body(block, lane, resident, list,
// b) per wave and block, `block` counted over the whole index, resident = the lane's position is below the list length,
// b = the block's index within `list` (so the lane's position in its list is 64 b + lane; both are wave-uniform).
template <class Body>
__device__ __forceinline__ void for_each_resident_block(const ResidentLists &L, Body body) {
  const uint32_t l = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (l >= L.nlists) return;
  const uint32_t len = L.list_len[l], fb = L.first_block[l], nblk = (len + 63u) / 64u;
  for (uint32_t b = blockIdx.y * 4u + wave; b < nblk; b += gridDim.y * 4u)  // (wave-uniform)
    body(fb + b, lane, b * 64u + lane < len, l, b);
}
#endif

struct ListLayout {
  std::vector<uint32_t> first, len;  // per list: its first block, its local length
  uint64_t total_blocks = 0, total_vec = 0;
};
enum class LayoutError { none, list_too_long, too_many_slots };

// The layout of lists of full_len[l] vectors on rank `rank` of `world` (1, 0: the whole lists).  A list longer than
// 2^32 - 1 - 64 vectors has positions that do not fit 32 bits once padded; 2^32 / 64 - 1 blocks or more have slots that
// do not.  On an error `out` is not to be used.
inline LayoutError plan_list_layout(const uint64_t *full_len, uint64_t nlists, uint32_t world, uint32_t rank, ListLayout *out) {
  out->first.assign(nlists, 0);
  out->len.assign(nlists, 0);
  out->total_blocks = out->total_vec = 0;
  for (uint64_t l = 0; l < nlists; ++l) {
    if (full_len[l] > 0xFFFFFFFFull - kListBlock) return LayoutError::list_too_long;
    out->first[l] = (uint32_t)out->total_blocks;
    out->len[l] = (uint32_t)local_len(full_len[l], world, rank);
    out->total_blocks += local_blocks(full_len[l], world, rank);
    out->total_vec += out->len[l];
    if (out->total_blocks >= 0xFFFFFFFFull / kListBlock) return LayoutError::too_many_slots;
  }
  return LayoutError::none;
}

}  // namespace vi
