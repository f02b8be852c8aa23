// slot_filter.hip — builds a SlotFilter (slot_filter.hpp): from the resident timestamps of an index, from a set of
// external ids, or as the intersection of two filters of one index.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_index.hpp"
#include "id_table.hpp"
#include "list_layout.hpp"
#include "rank_stream.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;

// what every filter is made of: the index's norm arrays, the filter's masked copies of them, its allow words, its count
struct FilterOut {
  const float *xnorm, *xnorm_img;
  const int *i8_norm_img;  // or null
  uint64_t *allow;
  float *xnorm_out, *xnorm_img_out;
  int *i8_out;
  unsigned long long *count;
};

// The one writer of a filter, called by a whole wave for 64-vector block `block` with lane = vector of the block and
// ok = "this slot is allowed" (false on every pad slot): lane 0 stores the wave's ballot as the block's allow word; the
// masked norms: natural order as they are, image order through image_column — the one definition of that permutation —
// with kBig / kI8PadNorm on the slots that are not allowed.  Returns the number of allowed slots of the block.
__device__ __forceinline__ uint32_t write_filter_block(const FilterOut &o, uint32_t block, uint32_t lane, bool ok) {
  const size_t base = (size_t)block * kWave;
  const uint32_t col = image_column(lane);
  const uint64_t word = __ballot(ok);
  if (lane == 0) o.allow[block] = word;
  o.xnorm_out[base + lane] = ok ? o.xnorm[base + lane] : kBig;
  o.xnorm_img_out[base + col] = ok ? o.xnorm_img[base + col] : kBig;
  if (o.i8_norm_img) o.i8_out[base + col] = ok ? o.i8_norm_img[base + col] : kI8PadNorm;
  return (uint32_t)__popcll(word);
}

// allow = stored timestamp within [ts_min, ts_max]
struct TimestampPred {
  const uint64_t *timestamps;
  uint64_t ts_min, ts_max;
  __device__ bool operator()(uint32_t block, uint32_t lane, bool resident) const {
    const uint64_t ts = timestamps[(size_t)block * kWave + lane];
    return resident && ts >= ts_min && ts <= ts_max;
  }
};

// allow = (external id is in the table, id_table.hpp) != exclude; the table is complete (the insert kernel ran before on the stream)
struct IdPred {
  const uint64_t *ext_ids;
  IdTable t;
  bool exclude;
  __device__ bool operator()(uint32_t block, uint32_t lane, bool resident) const {
    const bool member = id_table_find(t, ext_ids[(size_t)block * kWave + lane]) != kNoEntry;
    return resident && member != exclude;  // (resident first in both modes: a deny filter never allows a pad slot)
  }
};

// allow = a.allow & b.allow
struct IntersectPred {
  const uint64_t *a, *b;
  __device__ bool operator()(uint32_t block, uint32_t lane, bool resident) const {
    return resident && (((a[block] & b[block]) >> lane) & 1ull) != 0;
  }
};

// The walk of list_layout.hpp: a slot's allow bit is the predicate AND `position below the list length`.
template <class Pred>
__global__ void __launch_bounds__(256) slot_filter_kernel(ResidentLists L, FilterOut o, Pred pred) {
  uint32_t n = 0;
  for_each_resident_block(L, [&](uint32_t block, uint32_t lane, bool resident) {
    n += write_filter_block(o, block, lane, pred(block, lane, resident));
  });
  if ((threadIdx.x & 63u) == 0 && n) atomicAdd(o.count, (unsigned long long)n);
}

// The part every filter shares: the buffers of *f, the zeroed count, one launch of the kernel with `pred`, the count.
// The index's own statistics — xmax2, rho2_max, the centring mu, mean_* — are left as they are and keep setting the rank
// margins and the rank mode of a filtered search: a filter only removes candidates, it never widens a bound, so the
// margins of the full index remain valid upper bounds for every subset of it — whatever predicate chose the subset.
template <class Pred>
vi_status build_filter(const DeviceIndex &ix, const Pred &pred, SlotFilter *f, const uint32_t *flags_dev = nullptr,
                       uint32_t *flags_host = nullptr) {
  const uint64_t nb = ix.lists.nblocks, nslots = nb * kWave;
  f->owner_serial = ix.serial;
  VI_TRY(f->allow.reserve(std::max<uint64_t>(1, nb)));
  VI_TRY(f->xnorm.reserve(std::max<uint64_t>(1, nslots)));
  VI_TRY(f->xnorm_img.reserve(std::max<uint64_t>(1, nslots)));
  if (ix.i8_norm_img.p) VI_TRY(f->i8_norm_img.reserve(std::max<uint64_t>(1, nslots)));
  DevBuf<unsigned long long> cnt;
  VI_TRY(cnt.reserve(1));
  hipStream_t st = ix.stream;
  VI_HIP(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), st));
  VI_HIP(hipMemsetAsync(f->allow.p, 0, std::max<uint64_t>(1, nb) * sizeof(uint64_t), st));
  if (nb && ix.nlists) {
    ResidentLists L{ix.list_first_block.p, ix.list_len.p, (uint32_t)ix.nlists};
    FilterOut o{ix.xnorm.p, ix.xnorm_img.p, ix.i8_norm_img.p, f->allow.p, f->xnorm.p, f->xnorm_img.p, f->i8_norm_img.p, cnt.p};
    hipLaunchKernelGGL(slot_filter_kernel<Pred>, slot_walk_grid((uint32_t)ix.nlists), dim3(256), 0, st, L, o, pred);
    VI_HIP(hipGetLastError());
  }
  unsigned long long n = 0;
  VI_HIP(hipMemcpyAsync(&n, cnt.p, sizeof(n), hipMemcpyDeviceToHost, st));
  if (flags_dev) VI_HIP(hipMemcpyAsync(flags_host, flags_dev, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  f->num_allowed = n;
  return VI_OK;
}

}  // namespace

vi_status slot_filter_timestamps(const DeviceIndex &ix, uint64_t ts_min, uint64_t ts_max, SlotFilter *f) {
  if (!ix.timestamps.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no timestamps");
  VI_HIP(hipSetDevice(ix.device));
  return build_filter(ix, TimestampPred{ix.timestamps.p, ts_min, ts_max}, f);
}

vi_status slot_filter_ids(const DeviceIndex &ix, const uint64_t *ids, uint64_t n, bool ids_on_device, bool exclude,
                          SlotFilter *f) {
  if (!ix.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no external ids");
  if (n > (1ull << 40)) return fail(VI_ERR_INVALID_INPUT, "id set of %llu ids is too large", (unsigned long long)n);
  VI_HIP(hipSetDevice(ix.device));
  IdSetBuffers set;  // lives until this function returns
  IdTable t;
  VI_TRY(id_set_build(set, ids, n, ids_on_device, 0, ix.stream, &t));
  uint32_t fl[2] = {0, 0};
  VI_TRY(build_filter(ix, IdPred{ix.ext_ids.p, t, exclude}, f, set.flags.p, fl));
  return id_set_check(fl, t, n, "id filter");
}

vi_status slot_filter_intersect(const DeviceIndex &ix, const SlotFilter &a, const SlotFilter &b, SlotFilter *f) {
  if (a.owner_serial != ix.serial || b.owner_serial != ix.serial)
    return fail(VI_ERR_INVALID_INPUT, "the filter was made from another indexer (or before this one was rebuilt)");
  VI_HIP(hipSetDevice(ix.device));
  return build_filter(ix, IntersectPred{a.allow.p, b.allow.p}, f);
}

}  // namespace vi
