// flat_rows.hpp — from a pool of hits to sorted CSR rows: the last step of the exact radius search (flat_range.hip,
// DESIGN §4s), of the exact radius graph (flat_join.hip) and, up to the sort, of the exact k-NN graph
// (flat_knn.hip).  A pool entry is (key = distance bits << 32 |
// ordinal, row); flat_range_place_kernel scatters the pool into the rows, flat_range_sort_kernel sorts every row of up to
// kRangeSortLds keys in LDS, longer rows go through sort_rows_u64 on padded scratch (sort_csr_rows), and
// flat_range_output_kernel writes D / I / tie (the ordinal) / slot.  Each translation unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "flat_common.hpp"
#include "flat_range.hpp"
#include "search_internal.hpp"

namespace vi {
namespace {

constexpr uint64_t kNoKey = ~0ull;
constexpr uint64_t kPadKeys = 1ull << 25;  // keys of one batch of long rows on their padded scratch (256 MB)

// entry i of the pool to the next free place of its query's row; lims: the chunk's (global) row offsets, lims[0] = base
__global__ void __launch_bounds__(256) flat_range_place_kernel(const uint64_t *pool_key, const uint32_t *pool_q, uint64_t n,
                                                               const uint64_t *lims, uint32_t *fill, uint64_t *rows) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t q = pool_q[i];
  rows[(lims[q] - lims[0]) + atomicAdd(fill + q, 1u)] = pool_key[i];
}

// one wave per query: a row of 2 .. kRangeSortLds keys sorted in LDS (a bitonic network over the next power of two)
__global__ void __launch_bounds__(64) flat_range_sort_kernel(const uint64_t *lims, uint64_t *rows) {
  extern __shared__ __attribute__((aligned(16))) uint64_t s_keys[];
  const int lane = threadIdx.x;
  const uint64_t at = lims[blockIdx.x] - lims[0], n64 = lims[blockIdx.x + 1] - lims[blockIdx.x];
  if (n64 < 2 || n64 > kRangeSortLds) return;
  const uint32_t n = (uint32_t)n64;
  uint32_t P = kWave;
  while (P < n) P <<= 1;
  for (uint32_t i = lane; i < P; i += kWave) s_keys[i] = i < n ? rows[at + i] : kNoKey;
  wave_lds_sync();
  for (uint32_t k2 = 2; k2 <= P; k2 <<= 1)
    for (uint32_t j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      for (uint32_t t = lane; t < P / 2; t += kWave) {
        const uint32_t i = ((t & ~(j2 - 1u)) << 1) | (t & (j2 - 1u));
        const uint64_t x = s_keys[i], y = s_keys[i + j2];
        if ((x > y) == ((i & k2) == 0u)) { s_keys[i] = y; s_keys[i + j2] = x; }
      }
      wave_lds_sync();
    }
  for (uint32_t i = lane; i < n; i += kWave) rows[at + i] = s_keys[i];
}

// the rows of queries long[blockIdx.y] to (BACK false) or from (BACK true) rows of 2^logL keys padded with kNoKey
template <bool BACK>
__global__ void __launch_bounds__(256) flat_range_pad_kernel(const uint64_t *lims, const uint32_t *longq, uint32_t logL, uint64_t *rows,
                                                             uint64_t *pad) {
  const uint32_t q = longq[blockIdx.y];
  const uint64_t at = lims[q] - lims[0], n = lims[q + 1] - lims[q];
  uint64_t *row = pad + ((size_t)blockIdx.y << logL);
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < (1ull << logL); i += (uint64_t)gridDim.x * 256u) {
    if (BACK) { if (i < n) rows[at + i] = row[i]; }
    else row[i] = i < n ? rows[at + i] : kNoKey;
  }
}

struct RangeOutArgs {
  const uint64_t *rows;
  uint64_t n;
  const uint32_t *block_ord;
  const uint64_t *ext_ids;
  uint32_t nblocks;
  float *D;       // the chunk's first entry of the result
  int64_t *I;
  uint64_t *tie, *slots;
};

// sorted key i of the chunk -> entry i: the distance, the external id, the ordinal and the slot of the record
__global__ void __launch_bounds__(256) flat_range_output_kernel(RangeOutArgs o) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= o.n) return;
  const uint64_t key = o.rows[i];
  const uint32_t ordinal = (uint32_t)key, b = block_of_ordinal(o.block_ord, o.nblocks, ordinal);
  const uint64_t slot = (uint64_t)b * kWave + (ordinal - o.block_ord[b]);
  o.D[i] = __uint_as_float((uint32_t)(key >> 32));
  o.I[i] = (int64_t)o.ext_ids[slot];
  o.tie[i] = ordinal;
  o.slots[i] = slot;
}

// the sort kernel may be launched with rows of up to kRangeSortLds keys
inline vi_status reserve_csr_sort_lds() {
  if (hipFuncSetAttribute((const void *)flat_range_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(kRangeSortLds * sizeof(uint64_t))) != hipSuccess)
    return fail(VI_ERR_DEVICE, "cannot reserve LDS for the exact radius search's sort");
  return VI_OK;
}

// rows [0, m) of `rows` (bounds lims on the device, h_lims on the host, both from the first row on) sorted in place;
// longq / pad: scratch that grows.  Synchronises st where a row is too long for the LDS sort.
inline vi_status sort_csr_rows(const uint64_t *lims, const uint64_t *h_lims, uint64_t m, uint64_t *rows, DevBuf<uint32_t> &longq_buf,
                               DevBuf<uint64_t> &pad, hipStream_t st) {
  uint64_t longest = 0, lds_row = 0;  // the longest row, and the longest the LDS sort takes
  std::vector<uint32_t> longq;
  for (uint64_t q = 0; q < m; ++q) {
    const uint64_t n = h_lims[q + 1] - h_lims[q];
    longest = std::max(longest, n);
    if (n > kRangeSortLds) longq.push_back((uint32_t)q);
    else lds_row = std::max(lds_row, n);
  }
  if (lds_row >= 2) {
    uint64_t p2 = kWave;
    while (p2 < lds_row) p2 <<= 1;
    hipLaunchKernelGGL(flat_range_sort_kernel, dim3((uint32_t)m), dim3(64), p2 * sizeof(uint64_t), st, lims, rows);
    VI_HIP(hipGetLastError());
  }
  if (!longq.empty()) {
    uint32_t logL = 14;
    while ((1ull << logL) < longest) ++logL;
    const uint64_t per = std::max<uint64_t>(1, kPadKeys >> logL);
    VI_TRY(upload(longq_buf, longq.data(), longq.size(), st));
    VI_TRY(pad.reserve(std::min<uint64_t>(per, longq.size()) << logL));
    const uint32_t gx = (uint32_t)std::min<uint64_t>((1ull << logL) / 256u, 1024u);
    for (uint64_t r0 = 0; r0 < longq.size(); r0 += per) {
      const uint32_t nr = (uint32_t)std::min<uint64_t>(per, longq.size() - r0);
      hipLaunchKernelGGL(flat_range_pad_kernel<false>, dim3(gx, nr), dim3(256), 0, st, lims, longq_buf.p + r0, logL, rows, pad.p);
      VI_HIP(hipGetLastError());
      VI_TRY(sort_rows_u64(pad.p, nr, logL, st));
      hipLaunchKernelGGL(flat_range_pad_kernel<true>, dim3(gx, nr), dim3(256), 0, st, lims, longq_buf.p + r0, logL, rows, pad.p);
      VI_HIP(hipGetLastError());
    }
    VI_HIP(hipStreamSynchronize(st));  // (`longq` is read by its upload until here)
  }
  return VI_OK;
}

}  // namespace
}  // namespace vi
