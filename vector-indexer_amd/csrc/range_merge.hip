// range_merge.hip — merging the radius results of the ranks of a partitioned index into the unpartitioned result.
//
// Every part is a CSR radius result of the same nq queries (lims u64[nq + 1]; D f32, I i64, tie u64 of lims[nq] entries),
// each row sorted by the key (bits(D), tie) — distances are >= +0, so their bit patterns order as they do; the rule of
// merge_partials_kernel (search_kernels.hip).  The output is one CSR result in that order: lims[q] = sum over parts of
// lims_p[q].
//
// Merge by rank, parallel over ENTRIES: a radius row is ragged and can hold every probed vector, and one query can own
// most of a batch, so a wave-per-query loop (merge_partials_kernel: two wave reductions per emitted result) would
// serialise exactly the case that costs most.  Here every input entry finds its own destination:
//   dest = lims_out[q] + (its position in its row) + sum over the other parts p' of #{entries of row q of p' before it}
// where an entry of p' is before it if its key is smaller, or equal and p' < p: one binary search per other part.
//
// The part pointers (<= 64 x 4) travel in a small DEVICE TABLE (MergeTable below), not in a kernel-argument struct: a
// lane picks its part at run time, and a kernel-argument array indexed per lane would be copied to scratch.  Every
// workgroup of the place kernel copies the table to LDS once.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "device_index.hpp"

namespace vi {

namespace {

constexpr uint32_t kMergeThreads = 256;

// u64 words on the device: row r, part p at [r * kRangeMergeMaxParts + p]
enum : uint32_t { kRowLims = 0, kRowD = 1, kRowI = 2, kRowTie = 3, kRowBase = 4, kTableRows = 5 };
constexpr uint32_t kBaseWords = kRangeMergeMaxParts + 1;  // base[p] = entries of the parts before p; base[parts] = all
constexpr uint32_t kTableWords = kRowBase * kRangeMergeMaxParts + kBaseWords;

// one thread per q in 0..nq: lims_out[q] = sum_p lims_p[q].  The thread of q == nq also leaves the running sums — where
// each part's entries start in the flat entry numbering of the place kernel — in the table's base row.
__global__ void __launch_bounds__(kMergeThreads) range_merge_lims_kernel(uint64_t nq, uint32_t parts, uint64_t *table,
                                                                          uint64_t *lims_out) {
  const uint64_t q = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (q > nq) return;
  uint64_t sum = 0;
  for (uint32_t p = 0; p < parts; ++p) {
    const uint64_t *lims = reinterpret_cast<const uint64_t *>(table[kRowLims * kRangeMergeMaxParts + p]);
    if (q == nq) table[kRowBase * kRangeMergeMaxParts + p] = sum;
    sum += lims[q];
  }
  if (q == nq) table[kRowBase * kRangeMergeMaxParts + parts] = sum;
  lims_out[q] = sum;
}

// Flat over the `total` = sum_p lims_p[nq] input entries, one thread per entry.
//
// Memory safety does not depend on the rows being sorted.  For lims that are non-decreasing: entry e of part p lands in
// the row q with lims_p[q] <= e < lims_p[q + 1] (the guard below drops an entry that has no such row, as under
// lims_p[0] > 0), so its position in the row is < len_p(q); every count taken from another part p' is the end point of
// a binary search confined to [lims_p'[q], lims_p'[q + 1]), so it is <= len_p'(q), sorted or not.  Hence
//   lims_out[q] <= dest <= lims_out[q] + len_p(q) - 1 + sum_{p' != p} len_p'(q) = lims_out[q + 1] - 1 < total:
// inside the row's output range, inside the output buffers.  (Reads stay below lims_p'[nq], each part's length.)  On
// sorted rows the destinations of a row are a permutation of it even when two parts carry equal keys — a caller error,
// the same rank passed twice — because the part index breaks the tie.  `dest < total` is checked all the same.
__global__ void __launch_bounds__(kMergeThreads) range_merge_place_kernel(uint64_t nq, uint32_t parts, uint64_t total,
                                                                           const uint64_t *__restrict__ table,
                                                                           const uint64_t *__restrict__ lims_out,
                                                                           float *__restrict__ D_out, int64_t *__restrict__ I_out,
                                                                           uint64_t *__restrict__ tie_out) {
  __shared__ uint64_t tb[kTableWords];
  for (uint32_t i = threadIdx.x; i < kTableWords; i += kMergeThreads) tb[i] = table[i];  // (unused columns are zero)
  __syncthreads();
  const uint64_t t = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
  if (t >= total || nq == 0) return;
  const uint64_t *base = tb + kRowBase * kRangeMergeMaxParts;
  // the part: the last p with base[p] <= t (parts without entries share their base with the next part and are passed)
  uint32_t p = 0;
  {
    uint32_t lo = 0, hi = parts - 1;
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (base[mid] <= t) lo = mid; else hi = mid - 1;
    }
    p = lo;
  }
  const uint64_t e = t - base[p];
  const uint64_t *lims_p = reinterpret_cast<const uint64_t *>(tb[kRowLims * kRangeMergeMaxParts + p]);
  // the row: the last q with lims_p[q] <= e (upper bound - 1: empty rows share their lims with the next row and are passed)
  uint64_t q = 0;
  {
    uint64_t lo = 0, hi = nq - 1;
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo + 1) >> 1);
      if (lims_p[mid] <= e) lo = mid; else hi = mid - 1;
    }
    q = lo;
  }
  const uint64_t row0 = lims_p[q];
  if (e < row0 || e >= lims_p[q + 1]) return;  // (only on lims that are no CSR offsets)
  const float d = reinterpret_cast<const float *>(tb[kRowD * kRangeMergeMaxParts + p])[e];
  const int64_t id = reinterpret_cast<const int64_t *>(tb[kRowI * kRangeMergeMaxParts + p])[e];
  const uint64_t tie = reinterpret_cast<const uint64_t *>(tb[kRowTie * kRangeMergeMaxParts + p])[e];
  const uint32_t dk = __float_as_uint(d);
  uint64_t dest = lims_out[q] + (e - row0);
  for (uint32_t o = 0; o < parts; ++o) {
    if (o == p) continue;
    const uint64_t *lims_o = reinterpret_cast<const uint64_t *>(tb[kRowLims * kRangeMergeMaxParts + o]);
    const uint64_t a = lims_o[q], b = lims_o[q + 1];
    if (b <= a) continue;
    const float *D_o = reinterpret_cast<const float *>(tb[kRowD * kRangeMergeMaxParts + o]);
    const uint64_t *tie_o = reinterpret_cast<const uint64_t *>(tb[kRowTie * kRangeMergeMaxParts + o]);
    const bool equal_first = o < p;  // an equal key of a lower part comes first
    uint64_t lo = a, hi = b;
    while (lo < hi) {
      const uint64_t mid = lo + ((hi - lo) >> 1);
      const uint32_t md = __float_as_uint(D_o[mid]);
      bool before = md < dk;
      if (md == dk) {
        const uint64_t mt = tie_o[mid];
        before = mt < tie || (mt == tie && equal_first);
      }
      if (before) lo = mid + 1; else hi = mid;
    }
    dest += lo - a;
  }
  if (dest >= total) return;
  D_out[dest] = d;
  I_out[dest] = id;
  tie_out[dest] = tie;
}

thread_local RangeMergeTimes g_last_times{};

}  // namespace

RangeMergeTimes range_merge_last_times() { return g_last_times; }

vi_status range_merge_device(int device, uint64_t nq, uint32_t parts, const uint64_t *const *lims_dev, const float *const *D_dev,
                             const int64_t *const *I_dev, const uint64_t *const *tie_dev, RangeResult *out) {
  if (parts == 0 || parts > kRangeMergeMaxParts) return fail(VI_ERR_INVALID_INPUT, "parts must be 1..64");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(VI_ERR_DEVICE, "no HIP device visible: libvi_amd never falls back to the CPU");
  if (device < 0 || device >= ndev) return fail(VI_ERR_DEVICE, "device %d out of range (%d visible)", device, ndev);
  if (nq >= (1ull << 31) * kMergeThreads - 1) return fail(VI_ERR_INVALID_INPUT, "more than 2^39 queries");
  VI_HIP(hipSetDevice(device));
  const char *timing_env = getenv("VI_RANGE_MERGE_TIMING");
  const bool timing = timing_env && *timing_env && *timing_env != '0';
  StreamEvents<4> se;  // one stream; the events only under VI_RANGE_MERGE_TIMING
  if (timing) VI_TRY(se.create());
  else if (hipStreamCreateWithFlags(&se.stream, hipStreamDefault) != hipSuccess)
    return fail(VI_ERR_DEVICE, "hipStreamCreate failed: %s", hipGetErrorString(hipGetLastError()));
  hipStream_t st = se.stream;

  out->ix = nullptr;
  out->device = device;
  out->nq = nq;
  out->total = 0;
  out->h_lims.assign(nq + 1, 0);
  VI_TRY(out->lims.reserve(nq + 1));
  std::vector<uint64_t> h_table(kTableWords, 0);
  for (uint32_t p = 0; p < parts; ++p) {
    h_table[kRowLims * kRangeMergeMaxParts + p] = reinterpret_cast<uint64_t>(lims_dev[p]);
    h_table[kRowD * kRangeMergeMaxParts + p] = reinterpret_cast<uint64_t>(D_dev[p]);
    h_table[kRowI * kRangeMergeMaxParts + p] = reinterpret_cast<uint64_t>(I_dev[p]);
    h_table[kRowTie * kRangeMergeMaxParts + p] = reinterpret_cast<uint64_t>(tie_dev[p]);
  }
  DevBuf<uint64_t> table;
  VI_TRY(table.reserve(kTableWords));
  VI_HIP(hipMemcpyAsync(table.p, h_table.data(), kTableWords * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  if (timing) VI_HIP(hipEventRecord(se.ev[0], st));
  hipLaunchKernelGGL(range_merge_lims_kernel, dim3(ceil_div_u32(nq + 1, kMergeThreads)), dim3(kMergeThreads), 0, st, nq, parts,
                     table.p, out->lims.p);
  VI_HIP(hipGetLastError());
  if (timing) VI_HIP(hipEventRecord(se.ev[1], st));
  // the one synchronisation before the output exists: the grand total sizes D / I / tie
  VI_HIP(hipMemcpyAsync(out->h_lims.data(), out->lims.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  const uint64_t total = out->h_lims[nq];
  if (total >= (1ull << 31) * kMergeThreads) return fail(VI_ERR_INVALID_INPUT, "more than 2^39 entries to merge");
  out->cap = std::max<uint64_t>(1, total);
  VI_TRY(out->D.reserve(out->cap));
  VI_TRY(out->I.reserve(out->cap));
  VI_TRY(out->tie.reserve(out->cap));
  out->total = total;
  if (timing) VI_HIP(hipEventRecord(se.ev[2], st));
  if (total && nq) {
    hipLaunchKernelGGL(range_merge_place_kernel, dim3(ceil_div_u32(total, kMergeThreads)), dim3(kMergeThreads), 0, st, nq, parts,
                       total, table.p, out->lims.p, out->D.p, out->I.p, out->tie.p);
    VI_HIP(hipGetLastError());
  }
  if (timing) VI_HIP(hipEventRecord(se.ev[3], st));
  VI_HIP(hipStreamSynchronize(st));  // (the parts may go once the call returns)
  g_last_times = RangeMergeTimes{};
  if (timing) {
    g_last_times.ms_lims = elapsed_ms(se.ev[0], se.ev[1]);
    g_last_times.ms_alloc = elapsed_ms(se.ev[1], se.ev[2]);
    g_last_times.ms_place = elapsed_ms(se.ev[2], se.ev[3]);
  }
  return VI_OK;
}

}  // namespace vi
