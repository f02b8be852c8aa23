// slot_filter.hpp — a subset of an index's resident vectors that a search may be restricted to (slot_filter.hip).
//
// The search engines already ignore some slots: the pad lanes at the tail of every list.  The matrix-core ranking never
// ranks them because their squared norm is kBig (kI8PadNorm in the int8 frame), the exact evaluations mask them by
// `pos < len`.  A filter makes the excluded slots look the same way: a copy of the norm arrays in which they hold the pad
// value, and one allow bit per slot for the places where exact distances are offered.  The coarse step, the grouping, the
// work items, the records and the tie keys of a filtered search are those of the unfiltered one.
#pragma once
#include <cstdint>

#include "common.hpp"

namespace vi {

struct DeviceIndex;

constexpr float kBig = 3.0e38f;  // norm of pad slots inside the rank kernels (finite: low bits are reused)

// Column of vector v (0..63 of its block) in the bf16 / int8 images.  A lane of lane half h ends an MFMA holding rows
// (e&3) + 8(e>>2) + 4h (e = 0..15) of each 32-row tile: a SUB-BLOCK, the unit the select re-evaluates exactly.  The image
// places vectors so that sub-block (tile t, half h) is the 16 CONSECUTIVE vectors 32t + 16h .. + 15 of the block: their
// f32 quads are 256 contiguous bytes, two whole cache lines, where the identity placement touched half of four.
__host__ __device__ inline uint32_t image_column(uint32_t v) {
  const uint32_t t = v >> 5, h = (v >> 4) & 1u, e = v & 15u;
  return 32u * t + (e & 3u) + 8u * (e >> 2) + 4u * h;
}

// Immutable once built: any number of concurrent searches of its index may share it.  12 bytes per resident slot
// (16 with an int8 image) + 1 bit.  The one exception: slot_filter_compose overwrites a filter the caller hands it as
// `reuse`, and the caller guarantees that no search is using it meanwhile.
struct SlotFilter {
  uint64_t owner_serial = 0;      // DeviceIndex::serial of the index whose slots it describes
  DevBuf<uint64_t> allow;         // [lists.nblocks] bit = lane of the block; pad slots 0
  DevBuf<float> xnorm;            // the index's xnorm / xnorm_img / i8_norm_img with kBig / kI8PadNorm on every slot
  DevBuf<float> xnorm_img;        //   whose allow bit is 0
  DevBuf<int> i8_norm_img;        // (only when the index has an int8 image)
  DevBuf<unsigned long long> count;  // the writer's counter (one word): kept, so that writing a filter again allocates nothing
  uint64_t num_allowed = 0;       // resident vectors with allow bit 1
};

// allow = stored timestamp within [ts_min, ts_max] (both inclusive)
vi_status slot_filter_timestamps(const DeviceIndex &ix, uint64_t ts_min, uint64_t ts_max, SlotFilter *out);

// allow = (external id is one of ids[0..n)) != exclude.  The set needs no order and may repeat ids; any u64 is an id.  It
// becomes a hash table on the device (host ids are uploaded once, device ids are read in place); the table and the upload
// are freed before the call returns, so the finished filter costs what a timestamp filter costs.
vi_status slot_filter_ids(const DeviceIndex &ix, const uint64_t *ids, uint64_t n, bool ids_on_device, bool exclude,
                          SlotFilter *out);

// allow = a.allow & b.allow; both must be filters of ix (VI_ERR_INVALID_INPUT otherwise)
vi_status slot_filter_intersect(const DeviceIndex &ix, const SlotFilter &a, const SlotFilter &b, SlotFilter *out);

// allow = the AND (any == false) or the OR (any == true) of n = 1..VI_FILTER_MAX_TERMS terms (vi_filter_term, include/vi_amd.h),
// each flipped first where it says negate — and `resident`, whatever the expression: one launch of the writer for the
// whole expression.  filters[i]: the operand of term i where its kind is VI_TERM_FILTER (checked by the caller to be a
// filter of ix and not *out), else not read.  Kinds, bounds, null pointers and negate are checked by the caller
// (api.cpp); what depends on the index is checked here, before any device work: a timestamp term without timestamps, an
// id / id-range / mask term without external ids, a mask whose length is not ix.nvec_resident, an id set past 2^40.
// Every id term gets a table of its own (one IdSetBuffers each), all inserted on the index's stream before the launch and
// freed before the call returns.  A mask is one byte per resident record in list order (record_fetch.hpp), non-zero
// admits; a host mask is uploaded once.  *out may be a finished filter of ix: it is overwritten in place and, its
// buffers being large enough already, nothing is allocated for it.
vi_status slot_filter_compose(const DeviceIndex &ix, bool any, const vi_filter_term *terms, uint32_t n,
                              const SlotFilter *const *filters, SlotFilter *out);

}  // namespace vi
