// device_index.hip — where a resident index (DeviceIndex, device_index.hpp) is constructed.
//
// Four routes build one (device_index.hpp names them and their callers): device_index_load and device_index_from_rows
// here, device_index_from_order in list_build.hip, device_index_update in list_update.hip.  The steps they share:
//   layout        plan_list_layout (list_layout.hpp): first block and local length of every list, the two 32-bit limits
//   storage       alloc_list_storage: blocks, ids, timestamps and the per-list arrays, sized and uploaded from the layout
//   coarse table  coarse_table_from_rows / repack_table: rows 0..n-1 into lane-interleaved blocks
//   (layout, storage and a copied coarse table at once for the route that starts from an older index: lay_out_from_old)
//   ending        prepare_rank_images (rank_images.hip)
// What fills the list blocks is each route's own: repack_kernel (shard records), repack_rows_kernel (rows of a matrix),
// update_blocks_kernel (the kept records of an older index and new rows).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>

#include "device_index.hpp"
#include "list_layout.hpp"
#include "scan.hpp"
#include "search_internal.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBlockThreads = kWave * kWavesPerBlock;
static_assert(kWave == (int)kListBlock, "a block of the layout is one wave of vectors");

// ------------------------------------------------------------------------------------------
// repack: AoS records (or row-major rows) -> lane-interleaved blocks (+ external ids)
// ------------------------------------------------------------------------------------------
struct RepackArgs {
  const uint8_t *src;           // device image of a shard file / row-major matrix
  const uint64_t *blk_src;      // [nb] byte offset of the first record of each destination block
  const uint32_t *blk_nv;       // [nb] valid vectors in the block (1..64)
  const uint32_t *blk_dst;      // [nb] destination block index
  uint32_t nb, dim, dq;
  uint32_t stride;              // bytes between consecutive records
  uint32_t vec_off;             // byte offset of the f32 payload inside a record
  int32_t id_off;               // byte offset of the u64 external id, or -1
  float *blocks;
  uint64_t *ext_ids;            // may be null
  int32_t ts_off;               // byte offset of the u64 timestamp, or -1
  uint64_t *timestamps;         // may be null
};

__global__ void __launch_bounds__(kBlockThreads) repack_kernel(RepackArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t b = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (b >= a.nb) return;
  const uint32_t nv = a.blk_nv[b], dst = a.blk_dst[b];
  const uint8_t *rec = a.src + a.blk_src[b] + (size_t)lane * a.stride;
  const bool valid = (uint32_t)lane < nv;
  const float *v = reinterpret_cast<const float *>(rec + a.vec_off);
  float4 *out = reinterpret_cast<float4 *>(a.blocks) + ((size_t)dst * a.dq) * kWave + lane;
  for (uint32_t qd = 0; qd < a.dq; ++qd) {
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t e = qd * 4;
    if (valid) {
      if (e + 0 < a.dim) x.x = v[e + 0];
      if (e + 1 < a.dim) x.y = v[e + 1];
      if (e + 2 < a.dim) x.z = v[e + 2];
      if (e + 3 < a.dim) x.w = v[e + 3];
    }
    out[(size_t)qd * kWave] = x;
  }
  if (a.ext_ids) {
    uint64_t id = ~0ull;
    if (valid && a.id_off >= 0) id = *reinterpret_cast<const uint64_t *>(rec + a.id_off);
    a.ext_ids[(size_t)dst * kWave + lane] = id;
  }
  if (a.timestamps) {
    uint64_t ts = 0ull;
    if (valid && a.ts_off >= 0) ts = *reinterpret_cast<const uint64_t *>(rec + a.ts_off);
    a.timestamps[(size_t)dst * kWave + lane] = ts;
  }
}

// rows of a row-major matrix -> lane-interleaved blocks (one lane per destination slot)
__global__ void __launch_bounds__(kBlockThreads) repack_rows_kernel(const float *src, uint32_t dim, uint32_t dq,
                                                                   const uint32_t *row_of_slot, uint64_t nslots,
                                                                   const uint64_t *id_of_row, float *blocks,
                                                                   uint64_t *ids_out) {
  const uint64_t s = (uint64_t)blockIdx.x * kBlockThreads + threadIdx.x;
  if (s >= nslots) return;
  const uint32_t row = row_of_slot[s];
  const bool valid = row != kNoPos;
  const float *v = src + (size_t)row * dim;
  float4 *out = reinterpret_cast<float4 *>(blocks) + ((s / kWave) * dq) * kWave + (s % kWave);
  for (uint32_t qd = 0; qd < dq; ++qd) {
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint32_t e = qd * 4;
    if (valid) {
      if (e + 0 < dim) x.x = v[e + 0];
      if (e + 1 < dim) x.y = v[e + 1];
      if (e + 2 < dim) x.z = v[e + 2];
      if (e + 3 < dim) x.w = v[e + 3];
    }
    out[(size_t)qd * kWave] = x;
  }
  if (ids_out) ids_out[s] = valid ? (id_of_row ? id_of_row[row] : (uint64_t)row) : ~0ull;
}

}  // namespace

vi_status launch_repack_rows(const float *src, uint32_t dim, uint32_t dq, const uint32_t *row_of_slot,
                             uint64_t nslots, const uint64_t *id_of_row, float *blocks, uint64_t *ids_out,
                             hipStream_t st) {
  if (nslots == 0) return VI_OK;
  hipLaunchKernelGGL(repack_rows_kernel, dim3((uint32_t)((nslots + kBlockThreads - 1) / kBlockThreads)),
                     dim3(kBlockThreads), 0, st, src, dim, dq, row_of_slot, nslots, id_of_row, blocks, ids_out);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

DeviceIndex::~DeviceIndex() {
  if (stream) (void)hipStreamDestroy(stream);
}

vi_status init_device_index(DeviceIndex *ix, int device, uint32_t dim, uint64_t nlists) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(VI_ERR_DEVICE, "no HIP device visible: libvi_amd never falls back to the CPU");
  if (device < 0 || device >= ndev) return fail(VI_ERR_DEVICE, "device %d out of range (%d visible)", device, ndev);
  VI_HIP(hipSetDevice(device));
  ix->device = device;
  ix->dim = dim;
  ix->dq = layout_dq(dim);
  ix->nlists = nlists;
  if (!ix->stream) VI_HIP(hipStreamCreateWithFlags(&ix->stream, hipStreamDefault));
  return VI_OK;
}

// ------------------------------------------------------------------------------------------
// what every route shares
// ------------------------------------------------------------------------------------------
vi_status alloc_list_storage(DeviceIndex *ix, const ListLayout &lay, const uint32_t *shard_host, const DeviceIndex *shard_from,
                             bool with_timestamps) {
  const uint64_t nlists = ix->nlists, slots = std::max<uint64_t>(1, lay.total_blocks) * kWave;
  hipStream_t st = ix->stream;
  ix->nvec_resident = lay.total_vec;
  ix->lists.dq = ix->dq;
  ix->lists.nblocks = lay.total_blocks;
  VI_TRY(ix->lists.blocks.reserve(slots * ix->dq * 4));
  VI_TRY(ix->ext_ids.reserve(slots));
  if (with_timestamps) VI_TRY(ix->timestamps.reserve(slots));
  VI_TRY(upload(ix->list_first_block, lay.first.data(), nlists, st));
  VI_TRY(upload(ix->list_len, lay.len.data(), nlists, st));
  if (shard_from) {
    ix->nshards = shard_from->nshards;
    VI_TRY(ix->list_shard.reserve(std::max<uint64_t>(1, nlists)));
    if (nlists) VI_HIP(hipMemcpyAsync(ix->list_shard.p, shard_from->list_shard.p, nlists * 4, hipMemcpyDeviceToDevice, st));
  } else {
    ix->nshards = 0;
    for (uint64_t l = 0; l < nlists; ++l) ix->nshards = std::max<uint64_t>(ix->nshards, (uint64_t)shard_host[l] + 1);
    VI_TRY(upload(ix->list_shard, shard_host, nlists, st));
  }
  return VI_OK;
}

vi_status lay_out_from_old(DeviceIndex *ix, const DeviceIndex &old, const uint64_t *full_len, DevBuf<uint32_t> *block_list_dev) {
  const uint64_t nlists = ix->nlists;
  const uint32_t dq = ix->dq;
  hipStream_t st = ix->stream;
  // lists back to back in list order, each padded to whole blocks (as a load lays them)
  ListLayout lay;
  switch (plan_list_layout(full_len, nlists, 1, 0, &lay)) {
    case LayoutError::list_too_long: return fail(VI_ERR_INVALID_INPUT, "a list would pass the 32-bit position limit");
    case LayoutError::too_many_slots: return fail(VI_ERR_INVALID_INPUT, "index too large for 32-bit slot ids");
    case LayoutError::none: break;
  }
  std::vector<uint32_t> block_list(lay.total_blocks);
  for (uint64_t l = 0; l < nlists; ++l) {
    const uint64_t nb = ((uint64_t)lay.len[l] + kWave - 1) / kWave;
    std::fill(block_list.begin() + lay.first[l], block_list.begin() + lay.first[l] + nb, (uint32_t)l);
  }
  // coarse table and shard of every list: unchanged
  ix->centroids.dq = dq;
  ix->centroids.nblocks = old.centroids.nblocks;
  const uint64_t cwords = std::max<uint64_t>(1, old.centroids.nblocks) * dq * kWave * 4;
  VI_TRY(ix->centroids.blocks.reserve(cwords));
  if (old.centroids.nblocks)
    VI_HIP(hipMemcpyAsync(ix->centroids.blocks.p, old.centroids.blocks.p, old.centroids.nblocks * dq * kWave * 4 * sizeof(float),
                          hipMemcpyDeviceToDevice, st));
  VI_TRY(alloc_list_storage(ix, lay, nullptr, &old, true));
  VI_TRY(upload(*block_list_dev, block_list.data(), block_list.size(), st));
  VI_HIP(hipStreamSynchronize(st));  // (lay and block_list are read by the copies queued above)
  return VI_OK;
}

vi_status repack_table(const float *rows_dev, uint64_t n, uint32_t dim, uint32_t dq, float *blocks, hipStream_t st,
                       DevBuf<uint32_t> *ros_keep) {
  std::vector<uint32_t> ros((n + kWave - 1) / kWave * kWave, kNoPos);
  for (uint64_t i = 0; i < n; ++i) ros[i] = (uint32_t)i;
  DevBuf<uint32_t> own;
  DevBuf<uint32_t> &dros = ros_keep ? *ros_keep : own;
  VI_TRY(upload(dros, ros.data(), ros.size(), st));
  VI_TRY(launch_repack_rows(rows_dev, dim, dq, dros.p, ros.size(), nullptr, blocks, nullptr, st));
  VI_HIP(hipStreamSynchronize(st));  // ros (host vector) must outlive the copy
  return VI_OK;
}

vi_status coarse_table_from_rows(DeviceIndex *ix, const float *rows_dev) {
  const uint64_t nb = (ix->nlists + kWave - 1) / kWave;
  ix->centroids.dq = ix->dq;
  ix->centroids.nblocks = nb;
  VI_TRY(ix->centroids.blocks.reserve(std::max<uint64_t>(1, nb) * ix->dq * kWave * 4));
  return repack_table(rows_dev, ix->nlists, ix->dim, ix->dq, ix->centroids.blocks.p, ix->stream);
}

// ------------------------------------------------------------------------------------------
// upload
// ------------------------------------------------------------------------------------------
static vi_status repack_upload(const uint8_t *host_src, size_t src_bytes, const std::vector<uint64_t> &blk_src,
                               const std::vector<uint32_t> &blk_nv, const std::vector<uint32_t> &blk_dst,
                               uint32_t dim, uint32_t dq, uint32_t stride, uint32_t vec_off, int32_t id_off,
                               float *blocks, uint64_t *ext_ids, int32_t ts_off, uint64_t *timestamps, hipStream_t st) {
  const uint32_t nb = (uint32_t)blk_src.size();
  if (nb == 0) return VI_OK;
  DevBuf<uint8_t> img;
  DevBuf<uint64_t> dsrc;
  DevBuf<uint32_t> dnv, ddst;
  VI_TRY(img.reserve(src_bytes + 16));
  VI_TRY(dsrc.reserve(nb));
  VI_TRY(dnv.reserve(nb));
  VI_TRY(ddst.reserve(nb));
  VI_HIP(hipMemcpyAsync(img.p, host_src, src_bytes, hipMemcpyHostToDevice, st));
  VI_HIP(hipMemcpyAsync(dsrc.p, blk_src.data(), nb * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  VI_HIP(hipMemcpyAsync(dnv.p, blk_nv.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  VI_HIP(hipMemcpyAsync(ddst.p, blk_dst.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  RepackArgs a{img.p, dsrc.p, dnv.p, ddst.p, nb, dim, dq, stride, vec_off, id_off, blocks, ext_ids, ts_off, timestamps};
  hipLaunchKernelGGL(repack_kernel, dim3((nb + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlockThreads), 0, st, a);
  VI_HIP(hipGetLastError());
  VI_HIP(hipStreamSynchronize(st));  // img is freed on return
  return VI_OK;
}

std::vector<uint32_t> shard_owners(const std::vector<uint64_t> &shard_bytes, uint32_t world) {
  const size_t ns = shard_bytes.size();
  std::vector<uint32_t> order(ns), owner(ns, 0);
  for (size_t i = 0; i < ns; ++i) order[i] = (uint32_t)i;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return shard_bytes[a] > shard_bytes[b]; });
  std::vector<uint64_t> load(std::max<uint32_t>(world, 1), 0);
  for (uint32_t s : order) {
    uint32_t best = 0;
    for (uint32_t r = 1; r < load.size(); ++r)
      if (load[r] < load[best]) best = r;
    owner[s] = best;
    load[best] += shard_bytes[s];
  }
  return owner;
}

vi_status device_index_load(const IndexMeta &meta, const std::string &shards_dir, int device, int rank, int world,
                            int placement, DeviceIndex *ix) {
  VI_TRY(init_device_index(ix, device, meta.dimension, meta.k()));
  const uint32_t dim = ix->dim, dq = ix->dq;
  const uint64_t k = ix->nlists;

  // ---- centroid table ----
  {
    DevBuf<float> dtab;
    VI_TRY(upload(dtab, meta.centroids.data(), k * dim, ix->stream));
    VI_TRY(coarse_table_from_rows(ix, dtab.p));
  }

  // ---- lists: every rank maps all shard files and keeps a STRIPE of every list resident: block b (64 vectors)
  //      of a list lives on rank b % world.  Placement of whole lists (or whole shard files, the reference's
  //      grouping) cannot balance: on the bench workload two lists carry 52 % of the scan work, and the
  //      reference's super-k-means puts neighbouring lists into one shard (92 % / 8 % of the work at world 2).
  //      With stripes every rank scans 1/world of every probed list whatever the skew.  A local position p maps
  //      back to the list position ((p / 64) * world + rank) * 64 + p % 64 (tie keys, stripe_tie_kernel). ----
  uint64_t nshards = 0;
  for (uint64_t c = 0; c < k; ++c) nshards = std::max(nshards, meta.c2s[c] + 1);
  std::vector<uint32_t> h_shard(k, 0);
  for (uint64_t c = 0; c < k; ++c) h_shard[c] = (uint32_t)meta.c2s[c];
  std::vector<std::unique_ptr<ShardFile>> files(nshards);
  const bool part = world > 1;
  for (uint64_t s = 0; s < nshards; ++s) {
    auto f = std::make_unique<ShardFile>();
    // a missing/corrupt shard is skipped, as search does (`if let Ok`, ivf_index.rs:253-254)
    if (f->open(shards_dir, s) != VI_OK || f->dim() != dim) continue;
    files[s] = std::move(f);
  }
  for (uint64_t c = 0; c < k; ++c) {
    const uint64_t s = meta.c2s[c];
    if (s >= nshards || !files[s]) continue;
    const ShardListView *lv = files[s]->find(c);
    if (!lv) { files[s].reset(); continue; }  // NotFound fails the whole shard read (shards.rs:257-265)
  }
  // placement 1 (north_star's rule): whole shard files to ranks, greedy by bytes; this rank then holds every block of
  // the lists of its shards (W = 1 below) and nothing of the others
  std::vector<uint32_t> owner;
  const bool by_shard = part && placement == 1;
  if (by_shard) {
    std::vector<uint64_t> bytes(nshards, 0);
    for (uint64_t c = 0; c < k; ++c) {
      const uint64_t s = meta.c2s[c];
      if (s >= nshards || !files[s]) continue;
      if (const ShardListView *lv = files[s]->find(c)) bytes[s] += (uint64_t)lv->num_vectors * record_stride(dim);
    }
    owner = shard_owners(bytes, (uint32_t)world);
    for (uint64_t s = 0; s < nshards; ++s)
      if (owner[s] != (uint32_t)rank) files[s].reset();  // (as if the file were not there: its lists stay empty here)
  }
  const uint32_t W = (part && !by_shard) ? (uint32_t)world : 1u, R = (part && !by_shard) ? (uint32_t)rank : 0u;
  ix->stripe_world = W;
  ix->stripe_rank = R;
  // this rank's blocks of every list (list_layout.hpp: b = R, R+W, ... ; the last block of a list may be partial)
  std::vector<uint64_t> full_len(k, 0);
  for (uint64_t c = 0; c < k; ++c) {
    const uint64_t s = meta.c2s[c];
    if (s >= nshards || !files[s]) continue;
    full_len[c] = files[s]->find(c)->num_vectors;
  }
  ListLayout lay;
  if (plan_list_layout(full_len.data(), k, W, R, &lay) != LayoutError::none)
    return fail(VI_ERR_OTHER, "index too large for 32-bit slot ids");
  VI_TRY(alloc_list_storage(ix, lay, h_shard.data(), nullptr, true));
  const uint32_t stride = (uint32_t)record_stride(dim);
  for (uint64_t s = 0; s < nshards; ++s) {
    if (!files[s]) continue;
    const ShardFile &f = *files[s];
    std::vector<uint64_t> src;
    std::vector<uint32_t> nv, dst;
    const uint8_t *lo = nullptr, *hi = nullptr;
    for (uint32_t i = 0; i < f.num_lists(); ++i) {
      const ShardListView &lv = f.list(i);
      // (a file with duplicate centroid ids: only the first entry exists for the reference's linear find,
      // shards.rs:257-265 — a later one must not be uploaded over the blocks sized from the first)
      if (lv.centroid_id >= k || meta.c2s[lv.centroid_id] != s || lv.num_vectors == 0 || f.find(lv.centroid_id) != &lv) continue;
      if (!lo || lv.records < lo) lo = lv.records;
      const uint8_t *end = lv.records + (uint64_t)lv.num_vectors * stride;
      if (!hi || end > hi) hi = end;
    }
    if (!lo) continue;
    for (uint32_t i = 0; i < f.num_lists(); ++i) {
      const ShardListView &lv = f.list(i);
      if (lv.centroid_id >= k || meta.c2s[lv.centroid_id] != s || lv.num_vectors == 0 || f.find(lv.centroid_id) != &lv) continue;
      const uint32_t nb = (lv.num_vectors + kWave - 1) / kWave;
      for (uint32_t b = R; b < nb; b += W) {
        src.push_back((uint64_t)(lv.records - lo) + (uint64_t)b * kWave * stride);
        nv.push_back(std::min<uint32_t>(kWave, lv.num_vectors - b * kWave));
        dst.push_back(lay.first[lv.centroid_id] + (b - R) / W);
        if (dst.back() >= lay.total_blocks) return fail(VI_ERR_INVALID_DATA, "shard_%llu.bin: list blocks exceed the index layout", (unsigned long long)s);
      }
    }
    // VectorMeta {id, external_id, timestamp} (shards.rs:45-51): the timestamp stays resident for vi_indexer_filter_timestamps
    VI_TRY(repack_upload(lo, (size_t)(hi - lo), src, nv, dst, dim, dq, stride, (uint32_t)kVectorMetaBytes, 8,
                         ix->lists.blocks.p, ix->ext_ids.p, 16, ix->timestamps.p, ix->stream));
  }
  VI_HIP(hipStreamSynchronize(ix->stream));  // (lay and h_shard are read by the copies of alloc_list_storage)
  return prepare_rank_images(ix);
}

vi_status device_index_from_rows(int device, int order, uint32_t dim, const float *table_dev, uint64_t ntable,
                                 const float *rows_dev, const std::vector<uint64_t> &list_off,
                                 const std::vector<uint32_t> &member_rows, const uint64_t *ids_dev,
                                 const std::vector<uint32_t> *list_shard, DeviceIndex *ix) {
  const uint64_t nlists = list_off.size() - 1;
  if (nlists != ntable) return fail(VI_ERR_INVALID_INPUT, "table rows must equal list count");
  VI_TRY(init_device_index(ix, device, dim, nlists));
  ix->order = order;
  const uint32_t dq = ix->dq;
  hipStream_t st = ix->stream;
  VI_TRY(coarse_table_from_rows(ix, table_dev));
  std::vector<uint64_t> full_len(nlists);
  std::vector<uint32_t> h_shard(nlists, 0);
  for (uint64_t l = 0; l < nlists; ++l) {
    full_len[l] = list_off[l + 1] - list_off[l];
    h_shard[l] = list_shard ? (*list_shard)[l] : (uint32_t)l;
  }
  ListLayout lay;
  if (plan_list_layout(full_len.data(), nlists, 1, 0, &lay) != LayoutError::none)
    return fail(VI_ERR_OTHER, "index too large for 32-bit slot ids");
  VI_TRY(alloc_list_storage(ix, lay, h_shard.data(), nullptr, false));  // (no timestamps: the k-means hierarchy has none)
  {
    std::vector<uint32_t> ros(lay.total_blocks * kWave, kNoPos);
    for (uint64_t l = 0; l < nlists; ++l)
      for (uint64_t e = list_off[l]; e < list_off[l + 1]; ++e)
        ros[(uint64_t)lay.first[l] * kWave + (e - list_off[l])] = member_rows[e];
    DevBuf<uint32_t> dros;
    VI_TRY(upload(dros, ros.data(), ros.size(), st));
    VI_TRY(launch_repack_rows(rows_dev, dim, dq, dros.p, ros.size(), ids_dev, ix->lists.blocks.p, ix->ext_ids.p, st));
    VI_HIP(hipStreamSynchronize(st));  // (ros, lay and h_shard are read by the copies queued above)
  }
  return prepare_rank_images(ix);
}

}  // namespace vi
