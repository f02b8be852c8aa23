// id_table.hpp — a set of u64 ids as an open-addressing table on the device: power-of-two capacity, linear probing,
// kEmptyKey = free word.  The id that equals kEmptyKey cannot be a key: whether the set holds it is a flag word of its
// own, and its entry number is `capacity`, one past the words.  Used by the id filters (slot_filter.hip) and by the
// record fetch (record_fetch.hip), which keeps value arrays of capacity + 1 entries beside the words.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.hpp"

namespace vi {

constexpr uint64_t kEmptyKey = ~0ull;
constexpr uint64_t kNoEntry = ~0ull;  // id_table_find: the set does not hold the id

__device__ __forceinline__ uint64_t mix_id(uint64_t x) {  // splitmix64's finalizer: every id bit reaches every index bit
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

struct IdTable {
  unsigned long long *words;  // [capacity]
  uint64_t mask;              // capacity - 1
  uint32_t *flags;            // [0]: the set holds kEmptyKey   [1]: an insert found no free word (cannot happen: load <= 0.5)
};

// power of two >= 2 max(n, 1): load factor <= 0.5
inline uint64_t id_table_capacity(uint64_t n) {
  uint64_t capacity = 2;
  while (capacity < 2 * n) capacity <<= 1;
  return capacity;
}

// One thread per id of the set.  A duplicate meets its own key and is done.  The probe loop ends after `capacity` words
// whatever the table holds.
static __global__ void __launch_bounds__(256) id_table_insert_kernel(IdTable t, const uint64_t *ids, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t id = ids[i];
    if (id == kEmptyKey) {
      t.flags[0] = 1u;
      continue;
    }
    uint64_t h = mix_id(id) & t.mask;
    bool done = false;
    for (uint64_t probe = 0; probe <= t.mask && !done; ++probe, h = (h + 1) & t.mask) {
      const unsigned long long prev = atomicCAS(&t.words[h], (unsigned long long)kEmptyKey, (unsigned long long)id);
      done = prev == kEmptyKey || prev == id;
    }
    if (!done) t.flags[1] = 1u;
  }
}

// the entry of `id` in a complete table (the insert kernel ran before on the stream): its word's index, `capacity` for
// kEmptyKey, kNoEntry when the set does not hold it
__device__ __forceinline__ uint64_t id_table_find(const IdTable &t, uint64_t id) {
  if (id == kEmptyKey) return t.flags[0] != 0u ? t.mask + 1 : kNoEntry;
  uint64_t h = mix_id(id) & t.mask;
  for (uint64_t probe = 0; probe <= t.mask; ++probe, h = (h + 1) & t.mask) {
    const uint64_t w = t.words[h];
    if (w == id) return h;
    if (w == kEmptyKey) break;
  }
  return kNoEntry;
}

// The set of ids[0 .. n) (host memory unless on_device; n == 0: none is read) as *out, complete on stream st: 2 +
// extra_flag_words cleared flag words, host ids in b.upload.  `uploaded` (or null) is recorded behind the upload.
inline vi_status id_set_build(IdSetBuffers &b, const uint64_t *ids, uint64_t n, bool on_device, uint32_t extra_flag_words,
                              hipStream_t st, IdTable *out, hipEvent_t uploaded = nullptr) {
  const uint64_t capacity = id_table_capacity(n);
  VI_TRY(b.words.reserve(capacity));
  VI_TRY(b.flags.reserve(2 + extra_flag_words));
  if (n && !on_device) {
    VI_TRY(b.upload.reserve(n));
    VI_HIP(hipMemcpyAsync(b.upload.p, ids, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    ids = b.upload.p;
  }
  if (uploaded) VI_HIP(hipEventRecord(uploaded, st));
  VI_HIP(hipMemsetAsync(b.words.p, 0xff, capacity * sizeof(unsigned long long), st));  // every word kEmptyKey
  VI_HIP(hipMemsetAsync(b.flags.p, 0, (2 + extra_flag_words) * sizeof(uint32_t), st));
  *out = IdTable{b.words.p, capacity - 1, b.flags.p};
  if (n) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, 65536);
    hipLaunchKernelGGL(id_table_insert_kernel, dim3(grid), dim3(256), 0, st, *out, ids, n);
    VI_HIP(hipGetLastError());
  }
  return VI_OK;
}

// the refusal of a table whose flag words, read back, report an insert that found no free word
inline vi_status id_set_check(const uint32_t *flags_host, const IdTable &t, uint64_t n, const char *what) {
  if (flags_host[1]) return fail(VI_ERR_DEVICE, "%s: the id table (capacity %llu for %llu ids) overflowed", what,
                                 (unsigned long long)(t.mask + 1), (unsigned long long)n);
  return VI_OK;
}

}  // namespace vi
