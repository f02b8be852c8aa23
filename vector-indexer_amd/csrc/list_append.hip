// list_append.hip — the resident half of vi_indexer_add_records: a new DeviceIndex from the old one's blocks and a batch of
// new rows, without re-reading a shard file.
//
//   new rows (device, row-major, uploaded once)
//     -> label of every row: the coarse step of the old index with n_probe = 1 (device_index_search, probes_out), in
//        chunks — the first probe of the reference's coarse step (ivf_index.rs:205-220), whatever engine ranks it
//     -> rows grouped by label, ascending call index inside a label (group_ids_by_label_device)
//     -> on the host: the new length and first block of every list, and the list of every new block
//     -> append_blocks_kernel: one wave per NEW block.  Positions inside a list are kept, so a block whose 64 positions
//        are all old is a straight copy of the old block (dq coalesced 16-byte loads and stores per lane: lane = vector);
//        the one block of a list where old records end takes its old lanes from the old block and the others from the
//        row-major upload (as repack_rows_kernel reads it); blocks behind it are new rows only.  Pad lanes get what every
//        index upload leaves there: zero vectors, external id ~0, timestamp 0.
//     -> prepare_rank_images: norms, images and the rank mode's statistics, by the code a load runs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "device_index.hpp"
#include "search_internal.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;
constexpr int kAppendWaves = 4;            // waves (= blocks of 64 vectors) per workgroup
constexpr uint64_t kLabelChunk = 65536;    // rows per coarse step

struct AppendArgs {
  // the old index
  const float4 *old_blocks;
  const uint64_t *old_ext, *old_ts;
  const uint32_t *old_first, *old_len;     // per list
  // the new layout
  const uint32_t *new_first, *new_len;     // per list
  const uint32_t *block_list;              // per new block: its list
  uint64_t nblocks;                        // new blocks
  // the new rows, grouped by list: list l receives rows order[seg[l] .. seg[l + 1]) in that order
  const float *rows;                       // n x dim
  const uint64_t *row_ext, *row_ts;        // per row, resolved on the host (never null)
  const uint32_t *order, *seg;
  uint32_t dim, dq;
  float4 *blocks;
  uint64_t *ext, *ts;
};

__global__ void __launch_bounds__(kAppendWaves * kWave) append_blocks_kernel(AppendArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t b = (uint64_t)blockIdx.x * kAppendWaves + (threadIdx.x >> 6);
  if (b >= a.nblocks) return;
  const uint32_t l = a.block_list[b];
  const uint32_t j = (uint32_t)(b - a.new_first[l]);           // block of the list
  const uint32_t old_len = a.old_len[l], new_len = a.new_len[l];
  const uint32_t pos = j * kWave + lane;                       // position inside the list (new_len < 2^32 - 64)
  const uint32_t dq = a.dq;
  float4 *dst = a.blocks + (b * dq) * kWave + lane;
  const uint64_t slot = b * kWave + lane;
  const float4 *src = a.old_blocks + ((uint64_t)(a.old_first[l] + j) * dq) * kWave + lane;  // (read only where pos < old_len)
  const uint64_t old_slot = (uint64_t)(a.old_first[l] + j) * kWave + lane;
  if (j * kWave + (kWave - 1) < old_len) {  // all 64 positions old (wave-uniform): copy, four 1 KiB rows in flight
    for (uint32_t qd = 0; qd < dq; qd += 4) {  // (dq is a multiple of 4: layout_dq)
      float4 t[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) t[u] = src[(size_t)(qd + u) * kWave];
#pragma unroll
      for (int u = 0; u < 4; ++u) dst[(size_t)(qd + u) * kWave] = t[u];
    }
    a.ext[slot] = a.old_ext[old_slot];
    a.ts[slot] = a.old_ts[old_slot];
    return;
  }
  const bool is_old = pos < old_len, is_new = !is_old && pos < new_len;
  uint32_t row = 0;
  if (is_new) row = a.order[a.seg[l] + (pos - old_len)];
  const float *v = a.rows + (size_t)row * a.dim;
  for (uint32_t qd = 0; qd < dq; ++qd) {
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t e = qd * 4;
    if (is_old) {
      x = src[(size_t)qd * kWave];
    } else if (is_new) {
      if (e + 0 < a.dim) x.x = v[e + 0];
      if (e + 1 < a.dim) x.y = v[e + 1];
      if (e + 2 < a.dim) x.z = v[e + 2];
      if (e + 3 < a.dim) x.w = v[e + 3];
    }
    dst[(size_t)qd * kWave] = x;
  }
  a.ext[slot] = is_old ? a.old_ext[old_slot] : is_new ? a.row_ext[row] : ~0ull;
  a.ts[slot] = is_old ? a.old_ts[old_slot] : is_new ? a.row_ts[row] : 0ull;
}

struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

}  // namespace

// labels_dev[i] = the list the reference's coarse step probes first for row i: the old index's own coarse step, n_probe 1
vi_status device_index_label_rows(const DeviceIndex &ix, const float *rows_dev, uint64_t n, uint32_t *labels_dev) {
  if (n == 0) return VI_OK;
  if (ix.nlists == 0) return fail(VI_ERR_INVALID_INPUT, "the index has no list to add to");
  VI_HIP(hipSetDevice(ix.device));
  DevBuf<uint32_t> order_scratch;  // (the coarse step writes the candidate-order ranks too: all zero at one probe)
  VI_TRY(order_scratch.reserve(std::min(n, kLabelChunk)));
  for (uint64_t at = 0; at < n; at += kLabelChunk) {
    SearchIO io;
    io.queries = rows_dev + at * ix.dim;
    io.on_device = true;
    io.nq = std::min(kLabelChunk, n - at);
    io.k = 1;
    io.n_probe = 1;
    io.probes_out = labels_dev + at;
    io.order_out = order_scratch.p;
    VI_TRY(device_index_search(ix, io));
  }
  return VI_OK;
}

// The index `old` with rows appended: list l receives rows order_dev[seg_host[l] .. seg_host[l + 1]) of rows_dev behind its
// old records.  Complete on return; `old` is only read.
vi_status device_index_append(const DeviceIndex &old, const float *rows_dev, uint64_t n, const uint32_t *order_dev,
                              const uint32_t *seg_dev, const std::vector<uint64_t> &seg_host, const uint64_t *row_ext_dev,
                              const uint64_t *row_ts_dev, DeviceIndex *ix, float *ms_kernel, uint64_t *kernel_bytes) {
  const uint64_t nlists = old.nlists;
  if (old.stripe_world > 1) return fail(VI_ERR_INVALID_INPUT, "a partitioned index takes no records");
  if (seg_host.size() != nlists + 1 || seg_host[nlists] != n) return fail(VI_ERR_OTHER, "append: grouping does not match the index");
  VI_TRY(init_device_index(ix, old.device, old.dim, nlists));
  ix->order = old.order;
  ix->timing = old.timing;
  const uint32_t dq = ix->dq;
  hipStream_t st = ix->stream;
  // the new layout from the old lengths: lists back to back in list order, each padded to whole blocks (as a load lays them)
  std::vector<uint32_t> o_len(nlists);
  if (nlists) {
    VI_HIP(hipMemcpyAsync(o_len.data(), old.list_len.p, nlists * 4, hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
  }
  std::vector<uint64_t> full_len(nlists);
  for (uint64_t l = 0; l < nlists; ++l) full_len[l] = (uint64_t)o_len[l] + (seg_host[l + 1] - seg_host[l]);
  DevBuf<uint32_t> d_block_list;
  VI_TRY(lay_out_from_old(ix, old, full_len.data(), &d_block_list));  // (the new first / len are in place for the kernel below)
  const uint64_t total_blocks = ix->lists.nblocks;
  if (ms_kernel) *ms_kernel = 0.0f;
  if (kernel_bytes) *kernel_bytes = 0;
  if (total_blocks) {
    if (!old.timestamps.p || !old.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "the index keeps no ids or timestamps");
    AppendArgs a{};
    a.old_blocks = (const float4 *)old.lists.blocks.p;
    a.old_ext = old.ext_ids.p; a.old_ts = old.timestamps.p;
    a.old_first = old.list_first_block.p; a.old_len = old.list_len.p;
    a.new_first = ix->list_first_block.p; a.new_len = ix->list_len.p;
    a.block_list = d_block_list.p; a.nblocks = total_blocks;
    a.rows = rows_dev; a.row_ext = row_ext_dev; a.row_ts = row_ts_dev;
    a.order = order_dev; a.seg = seg_dev;
    a.dim = ix->dim; a.dq = dq;
    a.blocks = (float4 *)ix->lists.blocks.p; a.ext = ix->ext_ids.p; a.ts = ix->timestamps.p;
    EventPair ev;
    VI_HIP(hipEventCreate(&ev.a));
    VI_HIP(hipEventCreate(&ev.b));
    VI_HIP(hipEventRecord(ev.a, st));
    hipLaunchKernelGGL(append_blocks_kernel, dim3((uint32_t)((total_blocks + kAppendWaves - 1) / kAppendWaves)),
                       dim3(kAppendWaves * kWave), 0, st, a);
    VI_HIP(hipGetLastError());
    VI_HIP(hipEventRecord(ev.b, st));
    VI_HIP(hipStreamSynchronize(st));  // (block_list is freed on return)
    if (ms_kernel) (void)hipEventElapsedTime(ms_kernel, ev.a, ev.b);
    // read + written: every new block once each way (blocks, ids, timestamps), less what pad and new lanes do not read
    if (kernel_bytes) *kernel_bytes = 2 * total_blocks * ((uint64_t)dq * kWave * 16 + kWave * 16);
  } else {
    VI_HIP(hipStreamSynchronize(st));
  }
  return prepare_rank_images(ix);
}

}  // namespace vi
