// list_compact.hip — the resident half of vi_indexer_retain / vi_indexer_remove_ids: a new DeviceIndex holding the records
// of the old one that a SlotFilter admits, without re-reading a shard file.
//
//   keep.allow (one bit per old slot, pad slots 0)
//     -> kept_count_kernel: one wave per list.  Lanes stride over the list's old blocks; the popcount of each block's
//        allow word, scanned across the wave with a carry from stride to stride, is the number of kept records of the
//        list in front of the block (block_prefix) and, at the end, the list's new length.
//     -> on the host: the new layout from the new lengths, and the list of every new block (lay_out_from_old, the step
//        device_index_append takes)
//     -> compact_blocks_kernel: one wave per NEW block, lane = vector (gather form).  A full block of a list that lost
//        nothing is a straight copy of the old block.  Elsewhere new position p = 64 j + lane looks its source up: the old
//        block by binary search over the list's block_prefix, the lane inside it as the (p - prefix)-th set bit of the
//        block's allow word.  Sources inside a wave ascend and are mostly adjacent; the writes are whole rows.  Pad lanes
//        get what every index upload leaves there: zero vectors, external id ~0, timestamp 0.  Every word of the new
//        blocks / ext_ids / timestamps is written exactly once.
//     -> prepare_rank_images: norms, images and the rank mode's statistics, by the code a load runs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_index.hpp"
#include "search_internal.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;
constexpr int kCompactWaves = 4;  // waves per workgroup: lists of kept_count_kernel, new blocks of compact_blocks_kernel

struct CountArgs {
  const uint64_t *allow;                   // per old block
  const uint32_t *old_first, *old_len;     // per list
  uint32_t nlists;
  uint32_t *block_prefix;                  // per old block: kept records of its list in front of it
  uint32_t *new_len;                       // per list
};

__global__ void __launch_bounds__(kCompactWaves * kWave) kept_count_kernel(CountArgs a) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t l = blockIdx.x * kCompactWaves + (threadIdx.x >> 6);
  if (l >= a.nlists) return;
  const uint32_t first = a.old_first[l], nblk = (a.old_len[l] + kWave - 1) / kWave;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nblk; base += kWave) {  // (wave-uniform)
    const uint32_t b = base + lane;
    const uint32_t c = b < nblk ? (uint32_t)__popcll(a.allow[first + b]) : 0u;
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, kWave);
      if ((int)lane >= d) incl += up;
    }
    if (b < nblk) a.block_prefix[first + b] = carry + incl - c;
    carry += __shfl(incl, kWave - 1, kWave);
  }
  if (lane == 0) a.new_len[l] = carry;
}

struct CompactArgs {
  // the old index and what is kept of it
  const float4 *old_blocks;
  const uint64_t *old_ext, *old_ts;
  const uint32_t *old_first, *old_len;     // per list
  const uint64_t *allow;                   // per old block
  const uint32_t *block_prefix;            // per old block (kept_count_kernel)
  // the new layout
  const uint32_t *new_first, *new_len;     // per list
  const uint32_t *block_list;              // per new block: its list
  uint64_t nblocks;                        // new blocks
  uint32_t dq;
  float4 *blocks;
  uint64_t *ext, *ts;
};

// the r-th (from 0) set bit of w, which has more than r set bits: halve the word, step into the half that holds it
__device__ __forceinline__ uint32_t nth_set_bit(uint64_t w, uint32_t r) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t width = 32; width; width >>= 1) {
    const uint32_t c = (uint32_t)__popcll(w & ((1ull << width) - 1ull));
    if (r >= c) { r -= c; w >>= width; pos += width; }
  }
  return pos;
}

__global__ void __launch_bounds__(kCompactWaves * kWave) compact_blocks_kernel(CompactArgs a) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t b = (uint64_t)blockIdx.x * kCompactWaves + (threadIdx.x >> 6);
  if (b >= a.nblocks) return;
  const uint32_t l = a.block_list[b];
  const uint32_t j = (uint32_t)(b - a.new_first[l]);           // block of the list
  const uint32_t old_len = a.old_len[l], new_len = a.new_len[l], old_first = a.old_first[l];
  const uint32_t dq = a.dq;
  float4 *dst = a.blocks + (b * dq) * kWave + lane;
  const uint64_t slot = b * kWave + lane;
  const bool untouched = new_len == old_len;                   // (wave-uniform) positions are the old ones
  if (untouched && j * kWave + (kWave - 1) < new_len) {        // ... and all 64 are records: copy, four 1 KiB rows in flight
    const float4 *src = a.old_blocks + ((uint64_t)(old_first + j) * dq) * kWave + lane;
    const uint64_t old_slot = (uint64_t)(old_first + j) * kWave + lane;
    for (uint32_t qd = 0; qd < dq; qd += 4) {  // (dq is a multiple of 4: layout_dq)
      const float4 t0 = src[(size_t)(qd + 0) * kWave], t1 = src[(size_t)(qd + 1) * kWave];
      const float4 t2 = src[(size_t)(qd + 2) * kWave], t3 = src[(size_t)(qd + 3) * kWave];
      dst[(size_t)(qd + 0) * kWave] = t0;
      dst[(size_t)(qd + 1) * kWave] = t1;
      dst[(size_t)(qd + 2) * kWave] = t2;
      dst[(size_t)(qd + 3) * kWave] = t3;
    }
    a.ext[slot] = a.old_ext[old_slot];
    a.ts[slot] = a.old_ts[old_slot];
    return;
  }
  const uint32_t p = j * kWave + lane;                         // position inside the new list (new_len < 2^32 - 64)
  const bool valid = p < new_len;
  uint32_t sb = j, sl = lane;                                  // source block of the old list, lane inside it
  if (!untouched) {
    const uint32_t old_nblk = (old_len + kWave - 1) / kWave;   // >= 1: the list has a new block, so it had records
    const uint32_t ps = valid ? p : 0u;                        // (pad lanes search too, and read nothing afterwards)
    // the last old block whose prefix is <= ps: it holds kept record ps (blocks with nothing kept share the prefix of
    // the block behind them, so they are never the last).  The trip count depends on old_nblk alone: wave-uniform.
    uint32_t lo = 0, hi = old_nblk;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (a.block_prefix[old_first + mid] <= ps) lo = mid; else hi = mid;
    }
    sb = lo;
    sl = valid ? nth_set_bit(a.allow[old_first + sb], ps - a.block_prefix[old_first + sb]) : 0u;
  }
  const float4 *src = a.old_blocks + ((uint64_t)(old_first + sb) * dq) * kWave + sl;  // (read only where valid)
  const uint64_t old_slot = (uint64_t)(old_first + sb) * kWave + sl;
  for (uint32_t qd = 0; qd < dq; qd += 4) {  // four rows in flight here too
    float4 t0 = make_float4(0.f, 0.f, 0.f, 0.f), t1 = t0, t2 = t0, t3 = t0;
    if (valid) {
      t0 = src[(size_t)(qd + 0) * kWave];
      t1 = src[(size_t)(qd + 1) * kWave];
      t2 = src[(size_t)(qd + 2) * kWave];
      t3 = src[(size_t)(qd + 3) * kWave];
    }
    dst[(size_t)(qd + 0) * kWave] = t0;
    dst[(size_t)(qd + 1) * kWave] = t1;
    dst[(size_t)(qd + 2) * kWave] = t2;
    dst[(size_t)(qd + 3) * kWave] = t3;
  }
  a.ext[slot] = valid ? a.old_ext[old_slot] : ~0ull;
  a.ts[slot] = valid ? a.old_ts[old_slot] : 0ull;
}

struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

}  // namespace

// The index `old` without the records whose allow bit in `keep` is 0; the others close up in their old order.  Complete
// on return; `old` and `keep` are only read.
vi_status device_index_compact(const DeviceIndex &old, const SlotFilter &keep, DeviceIndex *ix, float *ms_kernel,
                               uint64_t *kernel_bytes) {
  const uint64_t nlists = old.nlists;
  if (old.stripe_world > 1) return fail(VI_ERR_INVALID_INPUT, "a partitioned index gives no records up");
  if (keep.owner_serial != old.serial) return fail(VI_ERR_INVALID_INPUT, "the filter was made from another index");
  if (!old.timestamps.p || !old.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "the index keeps no ids or timestamps");
  VI_TRY(init_device_index(ix, old.device, old.dim, nlists));
  ix->order = old.order;
  ix->timing = old.timing;
  hipStream_t st = ix->stream;
  if (ms_kernel) *ms_kernel = 0.0f;
  if (kernel_bytes) *kernel_bytes = 0;
  // ---- count pass: the new length of every list, the kept records in front of every old block ----
  DevBuf<uint32_t> block_prefix, d_new_len;
  VI_TRY(block_prefix.reserve(std::max<uint64_t>(1, old.lists.nblocks)));
  VI_TRY(d_new_len.reserve(std::max<uint64_t>(1, nlists)));
  std::vector<uint32_t> n_len(nlists);
  if (nlists) {
    CountArgs c{keep.allow.p, old.list_first_block.p, old.list_len.p, (uint32_t)nlists, block_prefix.p, d_new_len.p};
    hipLaunchKernelGGL(kept_count_kernel, dim3((uint32_t)((nlists + kCompactWaves - 1) / kCompactWaves)),
                       dim3(kCompactWaves * kWave), 0, st, c);
    VI_HIP(hipGetLastError());
    VI_HIP(hipMemcpyAsync(n_len.data(), d_new_len.p, nlists * 4, hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
  }
  std::vector<uint64_t> full_len(n_len.begin(), n_len.end());
  DevBuf<uint32_t> d_block_list;
  VI_TRY(lay_out_from_old(ix, old, full_len.data(), &d_block_list));
  const uint64_t total_blocks = ix->lists.nblocks;
  if (ix->nvec_resident != keep.num_allowed) return fail(VI_ERR_OTHER, "compact: the filter's count does not match its allow words");
  if (total_blocks) {
    CompactArgs a{};
    a.old_blocks = (const float4 *)old.lists.blocks.p;
    a.old_ext = old.ext_ids.p; a.old_ts = old.timestamps.p;
    a.old_first = old.list_first_block.p; a.old_len = old.list_len.p;
    a.allow = keep.allow.p; a.block_prefix = block_prefix.p;
    a.new_first = ix->list_first_block.p; a.new_len = ix->list_len.p;
    a.block_list = d_block_list.p; a.nblocks = total_blocks;
    a.dq = ix->dq;
    a.blocks = (float4 *)ix->lists.blocks.p; a.ext = ix->ext_ids.p; a.ts = ix->timestamps.p;
    EventPair ev;
    VI_HIP(hipEventCreate(&ev.a));
    VI_HIP(hipEventCreate(&ev.b));
    VI_HIP(hipEventRecord(ev.a, st));
    hipLaunchKernelGGL(compact_blocks_kernel, dim3((uint32_t)((total_blocks + kCompactWaves - 1) / kCompactWaves)),
                       dim3(kCompactWaves * kWave), 0, st, a);
    VI_HIP(hipGetLastError());
    VI_HIP(hipEventRecord(ev.b, st));
    VI_HIP(hipStreamSynchronize(st));  // (block_prefix and the block list are freed on return)
    if (ms_kernel) (void)hipEventElapsedTime(ms_kernel, ev.a, ev.b);
    // read + written: every new block once each way (blocks, ids, timestamps), less what pad lanes do not read
    if (kernel_bytes) *kernel_bytes = 2 * total_blocks * ((uint64_t)ix->dq * kWave * 16 + kWave * 16);
  }
  return prepare_rank_images(ix);
}

}  // namespace vi
