// list_blocks.hpp — what the two kernels that write the blocks of a new index from those of an old one have in common
// (update_blocks_kernel, list_update.hip; rehome_blocks_kernel, list_refine.hip), and the host frame around them.
//
// Both run one wave per NEW block, kBlockWaves blocks per workgroup, lane = vector of the block, and write every word of
// the new blocks / ext_ids / timestamps exactly once.  A lane's column of a block is dq quads, 1 KiB apart, filled four
// quads at a time (fill_block_column); a new block that is one whole old block in order is copied row by row
// (copy_old_block); a pad lane gets what every index upload leaves there.  Where a lane finds its source differs between
// the two kernels and stays with them.
#pragma once
#include <hip/hip_runtime.h>

#include "device_index.hpp"

namespace vi {

constexpr int kBlockWaves = 4;  // waves per workgroup: one new block each (kept_count_kernel: one list each)

struct OldBlocks { const float4 *blocks; const uint64_t *ext, *ts; };  // the index that is read
struct NewBlocks { float4 *blocks; uint64_t *ext, *ts; };              // ... and the one that is written
inline OldBlocks old_blocks_of(const DeviceIndex &ix) { return {(const float4 *)ix.lists.blocks.p, ix.ext_ids.p, ix.timestamps.p}; }
inline NewBlocks new_blocks_of(DeviceIndex *ix) { return {(float4 *)ix->lists.blocks.p, ix->ext_ids.p, ix->timestamps.p}; }

// read + written by a block kernel: every new block once each way (blocks, ids, timestamps), less what pad lanes (and
// the lanes of new rows) do not read
inline uint64_t block_bytes_moved(uint64_t nblocks, uint32_t dq) { return 2 * nblocks * ((uint64_t)dq * 64 * 16 + 64 * 16); }

constexpr uint64_t kPadExtId = ~0ull, kPadTimestamp = 0ull;
__device__ __forceinline__ float4 pad_quad() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// The lane's column of a new block (dst: its first quad), four quads at a time: load(qd, t) puts the lane's quads qd ..
// qd + 3 into t[0 .. 3] — all four loads under one test of where the lane reads from, so that they are in flight together
// — and leaves t alone on a pad lane.
template <typename LoadQuads>
__device__ __forceinline__ void fill_block_column(float4 *dst, uint32_t dq, LoadQuads load) {
  for (uint32_t qd = 0; qd < dq; qd += 4) {  // (dq is a multiple of 4: layout_dq)
    float4 t[4] = {pad_quad(), pad_quad(), pad_quad(), pad_quad()};
    load(qd, t);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) dst[(size_t)(qd + i) * 64] = t[i];
  }
}
// the four loads where the lane's column starts at src in the blocks of an index
__device__ __forceinline__ void load_block_quads(const float4 *src, uint32_t qd, float4 (&t)[4]) {
#pragma unroll
  for (uint32_t i = 0; i < 4; ++i) t[i] = src[(size_t)(qd + i) * 64];
}

// New block `nb` is old block `ob`, vectors, ids and timestamps: every load and store of the wave is one 1 KiB row.
__device__ __forceinline__ void copy_old_block(const OldBlocks &o, const NewBlocks &n, uint32_t dq, uint64_t ob, uint64_t nb, uint32_t lane) {
  const float4 *src = o.blocks + (ob * dq) * 64 + lane;
  fill_block_column(n.blocks + (nb * dq) * 64 + lane, dq, [&](uint32_t qd, float4 (&t)[4]) { load_block_quads(src, qd, t); });
  n.ext[nb * 64 + lane] = o.ext[ob * 64 + lane];
  n.ts[nb * 64 + lane] = o.ts[ob * 64 + lane];
}

// What every route from an old index begins with (list_update.hip): the refusals (`refusal`: the call's own words for a
// partitioned index), then — behind the route's own refusals, before any device call — a fresh index on old's device
// with old's summation order and timing.
vi_status refuse_update(const DeviceIndex &old, const char *refusal);
vi_status begin_update(const DeviceIndex &old, DeviceIndex *ix);

// `kernel` over `nblocks` new blocks, one wave each, between two HIP events; synchronised on return (the caller's scratch
// may go).  ms (optional): the time between the events.
template <typename Args>
vi_status launch_block_kernel(void (*kernel)(Args), const Args &a, uint64_t nblocks, hipStream_t st, float *ms) {
  EventSpans<1> ev;
  VI_TRY(ev.create(true));
  VI_TRY(ev.begin(0, st));
  hipLaunchKernelGGL(kernel, dim3(ceil_div_u32(nblocks, kBlockWaves)), dim3(kBlockWaves * 64), 0, st, a);
  VI_HIP(hipGetLastError());
  VI_TRY(ev.end(0, st));
  VI_HIP(hipStreamSynchronize(st));
  if (ms) *ms = ev.ms(0);
  return VI_OK;
}

}  // namespace vi
