// slot_filter.hip — builds a SlotFilter (slot_filter.hpp) from the resident timestamps of an index.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_index.hpp"
#include "rank_stream.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;
constexpr uint32_t kListSplit = 8;  // workgroups sharing the blocks of one list (long lists carry most of an index)

struct FilterBuildArgs {
  const uint32_t *first_block, *list_len;
  uint32_t nlists;
  const uint64_t *timestamps;
  uint64_t ts_min, ts_max;
  const float *xnorm, *xnorm_img;
  const int *i8_norm_img;  // or null
  uint64_t *allow;
  float *xnorm_out, *xnorm_img_out;
  int *i8_out;
  unsigned long long *count;
};

// One wave per 64-vector block, the list layout taken as pad_norms_kernel takes it (first block and length of every
// list; lists that are not resident here have length 0).  Lane = vector of the block: its allow bit is `timestamp in the
// window` AND `position below the list length`; lane 0 stores the wave's ballot as the block's allow word.  The masked
// norms: natural order as they are, image order through image_column — the one definition of that permutation.
__global__ void __launch_bounds__(256) slot_filter_kernel(FilterBuildArgs a) {
  const uint32_t l = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (l >= a.nlists) return;
  const uint32_t len = a.list_len[l], fb = a.first_block[l], nblk = (len + 63u) / 64u;
  const uint32_t col = image_column(lane);
  uint32_t n = 0;
  for (uint32_t b = blockIdx.y * 4u + wave; b < nblk; b += gridDim.y * 4u) {  // (wave-uniform)
    const size_t base = (size_t)(fb + b) * kWave;
    const uint64_t ts = a.timestamps[base + lane];
    const bool ok = b * 64u + lane < len && ts >= a.ts_min && ts <= a.ts_max;
    const uint64_t word = __ballot(ok);
    if (lane == 0) a.allow[fb + b] = word;
    a.xnorm_out[base + lane] = ok ? a.xnorm[base + lane] : kBig;
    a.xnorm_img_out[base + col] = ok ? a.xnorm_img[base + col] : kBig;
    if (a.i8_norm_img) a.i8_out[base + col] = ok ? a.i8_norm_img[base + col] : kI8PadNorm;
    n += (uint32_t)__popcll(word);
  }
  if (lane == 0 && n) atomicAdd(a.count, (unsigned long long)n);
}

}  // namespace

// The index's own statistics — xmax2, rho2_max, the centring mu, mean_* — are left as they are and keep setting the rank
// margins and the rank mode of a filtered search: a filter only removes candidates, it never widens a bound, so the
// margins of the full index remain valid upper bounds for every subset of it.
vi_status slot_filter_timestamps(const DeviceIndex &ix, uint64_t ts_min, uint64_t ts_max, SlotFilter *f) {
  if (!ix.timestamps.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no timestamps");
  VI_HIP(hipSetDevice(ix.device));
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
    FilterBuildArgs a{ix.list_first_block.p, ix.list_len.p, (uint32_t)ix.nlists, ix.timestamps.p, ts_min, ts_max,
                      ix.xnorm.p, ix.xnorm_img.p, ix.i8_norm_img.p, f->allow.p, f->xnorm.p, f->xnorm_img.p,
                      f->i8_norm_img.p, cnt.p};
    hipLaunchKernelGGL(slot_filter_kernel, dim3((uint32_t)ix.nlists, kListSplit), dim3(256), 0, st, a);
    VI_HIP(hipGetLastError());
  }
  unsigned long long n = 0;
  VI_HIP(hipMemcpyAsync(&n, cnt.p, sizeof(n), hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  f->num_allowed = n;
  return VI_OK;
}

}  // namespace vi
