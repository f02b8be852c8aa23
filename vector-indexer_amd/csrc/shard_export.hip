// shard_export.hip — one shard_<id>.bin from records that are in HBM, byte-identical to shard_save_to (shards.cpp: the
// frame is laid down by the routines it uses).
//
// One kernel lays the records (24 B meta + D f32 + pad) out in file order in a staging image, one copy brings the image
// to pinned host memory, the host patches header, index and centroid vectors in (shard_frame_write), one write(2).  The
// kernel runs one wave per record — its list by binary search over the shard's lists with records, then 32-bit words of
// {id, external_id, timestamp, D x f32, pad} — and is a template over where a record comes from: RowSource, a row of a
// row-major matrix through `order` (a build: shard_export_device), or BlockSource, a slot of a resident index (a refine:
// shard_export_blocks).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "device_index.hpp"
#include "record_fetch.hpp"
#include "refine_rules.hpp"
#include "search_internal.hpp"
#include "shards.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;

// where the records of a shard go, per list of the shard with records
struct ExportFrame {
  const uint32_t *rec_first;     // index of its first record among the shard's records
  const uint64_t *rec_dst;       // byte offset of its first record inside the staging image
  uint32_t nlists, dim, stride;  // stride = bytes per record
  uint64_t nrec;                 // records of the shard
  uint8_t *image;
};

struct ExportRecord { uint64_t id, ext, ts; const uint32_t *values; };  // values: what Source::value reads dimension e from

struct RowSource {
  const float *X;
  const uint32_t *order;         // ids grouped by list
  const uint64_t *ext_ids;       // per point, or null: the id itself (bindings/python/src/lib.rs:236-243)
  const uint64_t *timestamps;    // per point (0 => now), or null: now (vector_store.rs:36-40)
  uint64_t now;
  uint32_t dim;
  const uint64_t *rec_src;       // per list: offset into order
  void bind(const uint64_t *src0, const uint64_t *) { rec_src = src0; }  // (no id0: the id is the row)
  __device__ ExportRecord record(uint32_t l, uint64_t j) const {
    const uint32_t id = order[rec_src[l] + j];  // internal id = position (vector_store.rs:33), high word 0
    uint64_t ts = timestamps ? timestamps[id] : 0ull;
    if (ts == 0) ts = now;
    return {id, ext_ids ? ext_ids[id] : (uint64_t)id, ts, reinterpret_cast<const uint32_t *>(X + (size_t)id * dim)};
  }
  __device__ uint32_t value(const ExportRecord &r, uint32_t e) const { return r.values[e]; }
};

struct BlockSource {
  const float *blocks;           // the index's blocks as floats
  const uint64_t *ext_ids, *timestamps;
  uint32_t dq;
  const uint64_t *rec_slot0;     // per list: slot of its first record
  const uint64_t *rec_id0;       // per list: ordinal of its first record
  void bind(const uint64_t *src0, const uint64_t *id0) { rec_slot0 = src0; rec_id0 = id0; }
  __device__ ExportRecord record(uint32_t l, uint64_t j) const {
    const uint64_t slot = rec_slot0[l] + j;
    return {rec_id0[l] + j, ext_ids[slot], timestamps[slot],
            reinterpret_cast<const uint32_t *>(blocks) + ((slot >> 6) * dq) * (kWave * 4) + (slot & 63u) * 4};
  }
  __device__ uint32_t value(const ExportRecord &r, uint32_t e) const { return r.values[(size_t)(e >> 2) * (kWave * 4) + (e & 3u)]; }
};

template <class Source>
__global__ void __launch_bounds__(256) export_records_kernel(ExportFrame a, Source s) {
  const int lane = threadIdx.x & 63;
  const uint64_t rec = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rec >= a.nrec) return;
  uint32_t lo = 0, hi = a.nlists;  // largest l with rec_first[l] <= rec (only lists with records take part)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.rec_first[mid] <= rec) lo = mid; else hi = mid;
  }
  const uint64_t j = rec - a.rec_first[lo];
  const ExportRecord r = s.record(lo, j);
  uint32_t *dst = reinterpret_cast<uint32_t *>(a.image + a.rec_dst[lo] + j * a.stride);
  const uint32_t words = a.stride / 4;
  for (uint32_t w = lane; w < words; w += kWave) {
    uint32_t v = 0;
    if (w == 0) v = (uint32_t)r.id;
    else if (w == 1) v = (uint32_t)(r.id >> 32);
    else if (w == 2) v = (uint32_t)r.ext;
    else if (w == 3) v = (uint32_t)(r.ext >> 32);
    else if (w == 4) v = (uint32_t)r.ts;
    else if (w == 5) v = (uint32_t)(r.ts >> 32);
    else if (w >= 6 && w < 6 + a.dim) v = s.value(r, w - 6);
    dst[w] = v;
  }
}

// The shard's lists in file order: centroid ids, centroid vectors (host, cids.size() x dim) and, per list, its records
// and where `src` finds the first of them (src0; id0 where the source wants one, else empty).  The file goes to `path`.
template <class Source>
vi_status export_shard(Source src, const std::string &path, bool unlink_on_failure, uint64_t shard_id, uint32_t dim,
                       const std::vector<uint64_t> &cids, const float *cvecs_host, const std::vector<uint64_t> &count,
                       const std::vector<uint64_t> &src0, const std::vector<uint64_t> &id0, ShardExportWs &ws, hipStream_t st,
                       uint64_t *bytes_out) {
  const uint32_t nl = (uint32_t)cids.size();
  uint64_t nrec = 0;
  for (uint32_t i = 0; i < nl; ++i) nrec += count[i];
  if (nrec >= 0xFFFFFFFFull) return fail(VI_ERR_OTHER, "shard with more than 2^32 records");
  const ShardPlan pl(dim, count);
  const uint64_t data_off = pl.data_off, total = pl.total;
  // staging image on the device (records only; header, index and centroid vectors are patched in on the host)
  VI_TRY(ws.image.reserve(total + 16));
  if (ws.host_cap < total) {
    if (ws.host) (void)hipHostFree(ws.host);
    ws.host = nullptr;
    ws.host_cap = 0;
    VI_HIP(hipHostMalloc((void **)&ws.host, total + 16));
    ws.host_cap = total;
  }
  // only lists with records take part in the kernel's search table
  std::vector<uint64_t> k_src, k_id0, k_dst;
  std::vector<uint32_t> k_first;
  for (uint32_t i = 0, first = 0; i < nl; ++i) {
    if (count[i]) { k_src.push_back(src0[i]); k_dst.push_back(pl.records(i)); k_first.push_back(first); }
    if (count[i] && !id0.empty()) k_id0.push_back(id0[i]);
    first += (uint32_t)count[i];
  }
  if (nrec) {
    VI_TRY(upload(ws.d_src, k_src.data(), k_src.size(), st));
    VI_TRY(upload(ws.d_id0, k_id0.data(), k_id0.size(), st));
    VI_TRY(upload(ws.d_dst, k_dst.data(), k_dst.size(), st));
    VI_TRY(upload(ws.d_first, k_first.data(), k_first.size(), st));
    src.bind(ws.d_src.p, ws.d_id0.p);
    const ExportFrame a{ws.d_first.p, ws.d_dst.p, (uint32_t)k_src.size(), dim, (uint32_t)pl.stride, nrec, ws.image.p};
    hipLaunchKernelGGL(export_records_kernel<Source>, dim3((uint32_t)((nrec + 3) / 4)), dim3(256), 0, st, a, src);
    VI_HIP(hipGetLastError());
    VI_HIP(hipMemcpyAsync(ws.host + data_off, ws.image.p + data_off, total - data_off, hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));  // (k_* are read by the copies above)
  }
  std::vector<const void *> cvecs(nl);
  for (uint32_t i = 0; i < nl; ++i) cvecs[i] = cvecs_host + (uint64_t)i * dim;
  shard_frame_write(ws.host, pl, shard_id, cids.data(), cvecs.data());
  if (bytes_out) *bytes_out = total;
  return shard_image_write(path, ws.host, total, unlink_on_failure);
}

}  // namespace

// (device_index.hpp)  The file takes its final name, the old one removed first (shards.rs:73).
vi_status shard_export_device(const std::string &shards_dir, uint64_t shard_id, uint32_t dim, const std::vector<uint64_t> &cids,
                              const float *cvecs_host, const std::vector<uint64_t> &src_off, const std::vector<uint32_t> &len,
                              const float *X_dev, const uint32_t *order_dev, const uint64_t *ext_dev, const uint64_t *ts_dev,
                              uint64_t now, ShardExportWs &ws, hipStream_t st) {
  VI_TRY(make_dirs(shards_dir));
  const std::string path = shard_file_path(shards_dir, shard_id);
  ::remove(path.c_str());
  const RowSource src{X_dev, order_dev, ext_dev, ts_dev, now, dim, nullptr};
  return export_shard(src, path, false, shard_id, dim, cids, cvecs_host, std::vector<uint64_t>(len.begin(), len.end()), src_off, {}, ws, st,
                      nullptr);
}

// (device_index.hpp)  `path` is a temporary name of the caller's; a file left short by a failed write is removed.
vi_status shard_export_blocks(const DeviceIndex &ix, const std::string &path, uint64_t shard_id, const std::vector<uint64_t> &cids,
                              const float *cvecs_host, ShardExportWs &ws, uint64_t *bytes_out) {
  hipStream_t st = ix.stream;
  VI_HIP(hipSetDevice(ix.device));
  VI_TRY(ensure_fetch_layout(ix, st));
  const FetchState &lay = ix.fetch;
  std::vector<uint64_t> count, slot0, id0;
  for (const uint64_t l : cids) {
    if (l >= ix.nlists) return fail(VI_ERR_INVALID_DATA, "shard %llu names a list the index does not hold", (unsigned long long)shard_id);
    count.push_back(lay.h_len[l]);
    slot0.push_back(refine_slot(lay.h_first[l], 0));
    id0.push_back(lay.h_prefix[l]);
  }
  const BlockSource src{ix.lists.blocks.p, ix.ext_ids.p, ix.timestamps.p, ix.dq, nullptr, nullptr};
  return export_shard(src, path, true, shard_id, ix.dim, cids, cvecs_host, count, slot0, id0, ws, st, bytes_out);
}

ShardExportWs::~ShardExportWs() {
  if (host) (void)hipHostFree(host);
}

}  // namespace vi
