// list_refine.hip — the resident half of vi_indexer_refine: Lloyd iterations warm-started from the table an index has,
// over the records it holds, without a row-major copy of them and without touching the old blocks until the end.
//
// The assignment is carried as arrays over POSITIONS of the current list order (position j of iteration t is the j-th
// record of the lists as iteration t - 1 left them; before the first iteration positions are the old index's list-order
// ordinals):
//   cur[j]      the old ordinal of the record at position j (null = the identity: the first iteration)
//   cur_lab[j]  its list
//   seg[l]      first position of list l
// One iteration (device_index_refine):
//   centres  list_means_kernel: per (list, column) one sequential f32 chain over the list's members in position order,
//            then one divide (refine_rules.hpp) — update_centroids_parallel's order (src/kmeans.rs:690-703).  A list
//            without a member keeps its centroid bits (the reference writes zeros there; a zero centroid would attract
//            records, so this is a deliberate deviation).
//   labels   a coarse-only index of the new table (device_index_from_rows, whose one list holds one row of the table, so
//            that every launch of prepare_rank_images has work) and the walk over stored records (StoredRowsWalk):
//            chunks of stored rows of the OLD index, in ordinal order, through that index's coarse step at n_probe 1 —
//            the labeller of an add (device_index_label_rows).  The search kernels are the ones every search runs.
//   lists    relabel_kernel brings the labels into position order and counts the moved records; the stable grouping of
//            positions by label (group_ids_by_label_device) gives the next order; compose_kernel maps it back to old
//            ordinals.
// After the last iteration, once: the new layout from the new lengths (lay_out_from_old), rehome_blocks_kernel — one wave
// per NEW block, lane = new position, source = the old slot of ordinal cur[seg[l] + p] — the new table
// (coarse_table_from_rows) and prepare_rank_images, the load's own code.
//
// Device memory beside the old and the new index: eight u32 words per record (the old and the new labels by ordinal, the
// new labels by position, cur and cur_lab twice each, the grouping's output) plus the grouping's scratch, one chunk of
// rows in the walk's search context, two tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "device_index.hpp"
#include "record_fetch.hpp"
#include "refine_rules.hpp"
#include "search_internal.hpp"
#include "shards.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;
constexpr int kRehomeWaves = 4;                       // new blocks per workgroup of rehome_blocks_kernel
constexpr uint32_t kMeanCols = 64;                    // columns of one list_means_kernel wave: lane = column on the way out
constexpr uint32_t kMeanQuads = kMeanCols / 4;
constexpr uint32_t kMeanStride = kMeanCols + 4;       // dwords; the pad keeps 16-byte alignment and spreads the rows over the banks

struct MeansArgs {
  const float4 *blocks;                    // the old index
  uint32_t dq, dim, nlists;
  const uint32_t *first_block, *old_len;   // per list
  const uint64_t *prefix;                  // per list: ordinal of its first record (FetchState::prefix)
  // the members of list l: ordinals cur[seg[l] .. seg[l + 1]).  cur == nullptr: the list's own records in their own order,
  // and seg is not read
  const uint32_t *cur, *seg;
  const float *table;                      // C: nlists x dim
  float *out;                              // C'
};

// One wave per (list, 64 columns).  64 members at a time: lane = member on the way in — its quads of the 64 columns into
// an LDS tile of 64 rows — lane = column on the way out: the column's chain takes the tile's rows in member order.  Where
// cur is null (the first iteration) the 64 members are one old block and every load instruction is one contiguous 1 KiB
// row of it; otherwise each lane reads its member's 16 bytes of every quad where the old index keeps them.  The chain of a
// (list, column) is sequential either way: the parallelism is lists x columns, never members.
__global__ void __launch_bounds__(kWave) list_means_kernel(MeansArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[kWave * kMeanStride];
  const uint32_t lane = threadIdx.x, l = blockIdx.x, q0 = blockIdx.y * kMeanQuads, col = blockIdx.y * kMeanCols + lane;
  const uint32_t seg0 = a.cur ? a.seg[l] : 0u;
  const uint32_t count = a.cur ? a.seg[l + 1] - seg0 : a.old_len[l];
  if (count == 0) {  // an empty list keeps its centroid, bit for bit
    if (col < a.dim) a.out[(size_t)l * a.dim + col] = a.table[(size_t)l * a.dim + col];
    return;
  }
  float acc = 0.0f;
  for (uint32_t base = 0; base < count; base += kWave) {  // (wave-uniform)
    const uint32_t m = min((uint32_t)kWave, count - base);
    const bool valid = lane < m;
    uint64_t slot = 0;
    if (valid)
      slot = a.cur ? refine_slot_of_ordinal(a.prefix, a.first_block, a.nlists, a.cur[seg0 + base + lane])
                   : refine_slot(a.first_block[l], (uint64_t)base + lane);
    const float4 *src = a.blocks + ((slot >> 6) * a.dq) * kWave + (slot & 63u);
#pragma unroll
    for (uint32_t c = 0; c < kMeanQuads; ++c)
      if (q0 + c < a.dq) {  // (uniform; the blocks are zero padded up to dq)
        const float4 v = valid ? src[(size_t)(q0 + c) * kWave] : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(&tile[lane * kMeanStride + 4u * c]) = v;
      }
    __syncthreads();
    if (col < a.dim)
      for (uint32_t v = 0; v < m; ++v) acc = refine_chain_add(acc, tile[v * kMeanStride + lane]);
    __syncthreads();  // the tile has been read out before the next members are laid in
  }
  if (col < a.dim) a.out[(size_t)l * a.dim + col] = refine_mean(acc, count);
}

// lab[j] = the list that holds ordinal j
__global__ void __launch_bounds__(256) position_lists_kernel(const uint64_t *prefix, uint32_t nlists, uint64_t n, uint32_t *lab) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) lab[j] = refine_list_of_ordinal(prefix, nlists, j);
}

// new_lab[j] (optional) = lab_ord[cur[j]] (cur null: lab_ord[j]); *moved += positions whose label differs from old_lab[j]
__global__ void __launch_bounds__(256) relabel_kernel(const uint32_t *lab_ord, const uint32_t *cur, const uint32_t *old_lab, uint64_t n,
                                                      uint32_t *new_lab, unsigned long long *moved) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool differs = false;
  if (j < n) {
    const uint32_t lab = lab_ord[cur ? cur[j] : j];
    if (new_lab) new_lab[j] = lab;
    differs = lab != old_lab[j];
  }
  const uint64_t m = __ballot(differs);
  if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(moved, (unsigned long long)__popcll(m));
}

// the grouping's order (new position -> previous position) mapped back to old ordinals, and the label of every new position
__global__ void __launch_bounds__(256) compose_kernel(const uint32_t *order, const uint32_t *cur, const uint32_t *lab_pos, uint64_t n,
                                                      uint32_t *new_cur, uint32_t *new_cur_lab) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t prev = order[j];
  new_cur[j] = cur ? cur[prev] : prev;
  new_cur_lab[j] = lab_pos[prev];
}

struct RehomeArgs {
  // the old index
  const float4 *old_blocks;
  const uint64_t *old_ext, *old_ts;
  const uint32_t *old_first;               // per list
  const uint64_t *old_prefix;              // per list
  uint32_t nlists, dq;
  // the assignment: list l holds the records of old ordinals cur[seg[l] .. seg[l + 1]), in that order
  const uint32_t *cur, *seg;
  // the new layout
  const uint32_t *new_first, *new_len;     // per list
  const uint32_t *block_list;              // per new block: its list
  uint64_t nblocks;
  float4 *blocks;
  uint64_t *ext, *ts;
};

// One wave per NEW block, lane = new position.  Vector, external id and timestamp of position p of list l come from the
// old slot of ordinal cur[seg[l] + p]; a pad lane gets what every upload leaves there: a zero vector, id ~0, timestamp 0.
// Every word of the new blocks / ext / ts is written exactly once.  A block whose 64 sources are one whole old block in
// order — every block of a list nothing joined and nothing left, but its last — is a straight copy of it: four 1 KiB rows
// in flight, as update_blocks_kernel copies (list_update.hip: copy_old_block).
__global__ void __launch_bounds__(kRehomeWaves * kWave) rehome_blocks_kernel(RehomeArgs a) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t b = (uint64_t)blockIdx.x * kRehomeWaves + (threadIdx.x >> 6);
  if (b >= a.nblocks) return;
  const uint32_t l = a.block_list[b];
  const uint32_t p = (uint32_t)(b - a.new_first[l]) * kWave + lane;
  const bool valid = p < a.new_len[l];
  uint64_t src_slot = 0;
  if (valid) src_slot = refine_slot_of_ordinal(a.old_prefix, a.old_first, a.nlists, a.cur[a.seg[l] + p]);
  const uint32_t dq = a.dq;
  float4 *dst = a.blocks + (b * dq) * kWave + lane;
  const uint64_t slot = b * kWave + lane;
  const uint64_t slot0 = __shfl(src_slot, 0, kWave);
  if (__all(valid && src_slot == slot0 + lane) && (slot0 & 63u) == 0) {  // (wave-uniform) one whole old block, in order
    const float4 *src = a.old_blocks + ((slot0 >> 6) * dq) * kWave + lane;
    for (uint32_t qd = 0; qd < dq; qd += 4) {  // (dq is a multiple of 4: layout_dq)
      const float4 t0 = src[(size_t)(qd + 0) * kWave], t1 = src[(size_t)(qd + 1) * kWave];
      const float4 t2 = src[(size_t)(qd + 2) * kWave], t3 = src[(size_t)(qd + 3) * kWave];
      dst[(size_t)(qd + 0) * kWave] = t0;
      dst[(size_t)(qd + 1) * kWave] = t1;
      dst[(size_t)(qd + 2) * kWave] = t2;
      dst[(size_t)(qd + 3) * kWave] = t3;
    }
    a.ext[slot] = a.old_ext[slot0 + lane];
    a.ts[slot] = a.old_ts[slot0 + lane];
    return;
  }
  const float4 *src = a.old_blocks + ((src_slot >> 6) * dq) * kWave + (src_slot & 63u);  // (read only where valid)
  for (uint32_t qd = 0; qd < dq; qd += 4) {
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
  a.ext[slot] = valid ? a.old_ext[src_slot] : ~0ull;
  a.ts[slot] = valid ? a.old_ts[src_slot] : 0ull;
}

// records of one shard in file order, read from the blocks of a resident index.  One wave per record: 32-bit words of
// {id, external_id, timestamp, D x f32, pad} (list_build.hip: export_records_kernel reads a row-major matrix instead).
// VectorMeta.id is the record's list-order ordinal.
struct BlockExportArgs {
  const float *blocks;           // the index's blocks as floats
  const uint64_t *ext_ids, *timestamps;
  const uint64_t *rec_slot0;     // per list of the shard with records: slot of its first record
  const uint64_t *rec_id0;       // per list: ordinal of its first record
  const uint64_t *rec_dst;       // per list: byte offset of its first record inside the staging image
  const uint32_t *rec_first;     // per list: index of its first record among the shard's records
  uint32_t nlists, dim, dq, stride;
  uint64_t nrec;
  uint8_t *image;
};

__global__ void __launch_bounds__(256) export_block_records_kernel(BlockExportArgs a) {
  const int lane = threadIdx.x & 63;
  const uint64_t rec = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (rec >= a.nrec) return;
  uint32_t lo = 0, hi = a.nlists;  // largest l with rec_first[l] <= rec (only lists with records take part)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.rec_first[mid] <= rec) lo = mid; else hi = mid;
  }
  const uint64_t j = rec - a.rec_first[lo];
  const uint64_t slot = a.rec_slot0[lo] + j, id = a.rec_id0[lo] + j;
  uint32_t *dst = reinterpret_cast<uint32_t *>(a.image + a.rec_dst[lo] + j * a.stride);
  const uint64_t ext = a.ext_ids[slot], ts = a.timestamps[slot];
  const uint32_t *src = reinterpret_cast<const uint32_t *>(a.blocks) + ((slot >> 6) * a.dq) * (kWave * 4) + (slot & 63u) * 4;
  const uint32_t words = a.stride / 4;
  for (uint32_t w = lane; w < words; w += kWave) {
    uint32_t v = 0;
    if (w == 0) v = (uint32_t)id;
    else if (w == 1) v = (uint32_t)(id >> 32);
    else if (w == 2) v = (uint32_t)ext;
    else if (w == 3) v = (uint32_t)(ext >> 32);
    else if (w == 4) v = (uint32_t)ts;
    else if (w == 5) v = (uint32_t)(ts >> 32);
    else if (w >= 6 && w < 6 + a.dim) {
      const uint32_t e = w - 6;
      v = src[(size_t)(e >> 2) * (kWave * 4) + (e & 3u)];
    }
    dst[w] = v;
  }
}

struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  vi_status create() {
    VI_HIP(hipEventCreate(&a));
    VI_HIP(hipEventCreate(&b));
    return VI_OK;
  }
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

inline dim3 grid_1d(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

}  // namespace

vi_status device_index_refine(const DeviceIndex &old, const float *table_host, uint64_t iters, DeviceIndex *ix, RefineResult *res) {
  *res = RefineResult{};
  const uint64_t nlists = old.nlists, n = old.nvec_resident;
  const uint32_t dim = old.dim, dq = old.dq;
  if (old.stripe_world > 1) return fail(VI_ERR_INVALID_INPUT, "a partitioned index is not refined");
  if (!old.timestamps.p || !old.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "the index keeps no ids or timestamps");
  if (iters == 0 || n == 0 || nlists == 0) return fail(VI_ERR_OTHER, "refine: nothing to do");
  VI_TRY(init_device_index(ix, old.device, dim, nlists));
  ix->order = old.order;
  ix->timing = old.timing;
  hipStream_t st = ix->stream;
  VI_TRY(ensure_fetch_layout(old, st));
  const FetchState &lay = old.fetch;
  res->old_len = lay.h_len;

  DevBuf<float> table[2];                                 // C and C', swapped from iteration to iteration
  DevBuf<uint32_t> lab0, lab_ord, lab_pos, cur_lab[2], cur[2], order, seg, order_scratch;
  DevBuf<unsigned long long> d_moved;
  VI_TRY(upload(table[0], table_host, nlists * dim, st));
  VI_TRY(table[1].reserve(nlists * dim));
  VI_TRY(lab0.reserve(n));
  VI_TRY(lab_ord.reserve(n));
  VI_TRY(lab_pos.reserve(n));
  VI_TRY(cur_lab[0].reserve(n));
  VI_TRY(cur_lab[1].reserve(n));
  VI_TRY(cur[0].reserve(n));
  VI_TRY(cur[1].reserve(n));
  VI_TRY(d_moved.reserve(1));
  hipLaunchKernelGGL(position_lists_kernel, grid_1d(n), dim3(256), 0, st, lay.prefix.p, (uint32_t)nlists, n, lab0.p);
  VI_HIP(hipGetLastError());
  VI_HIP(hipMemcpyAsync(cur_lab[0].p, lab0.p, n * 4, hipMemcpyDeviceToDevice, st));
  VI_HIP(hipStreamSynchronize(st));

  EventPair ev;
  VI_TRY(ev.create());
  std::vector<float> h_table(table_host, table_host + nlists * dim), h_new(nlists * dim);
  std::vector<uint64_t> seg_host;
  const uint32_t *cur_p = nullptr;  // identity before the first iteration
  int tc = 0, cc = 0;               // which of table[] / cur[] / cur_lab[] is current
  const StoredRows all_rows{nullptr, 0, n, true};
  for (uint64_t it = 0; it < iters; ++it) {
    // ---- centres ----
    const double t0 = now_ms();
    {
      MeansArgs a{(const float4 *)old.lists.blocks.p, dq, dim, (uint32_t)nlists, old.list_first_block.p, old.list_len.p, lay.prefix.p,
                  cur_p, seg.p, table[tc].p, table[tc ^ 1].p};
      VI_HIP(hipEventRecord(ev.a, st));
      hipLaunchKernelGGL(list_means_kernel, dim3((uint32_t)nlists, (dim + kMeanCols - 1) / kMeanCols), dim3(kWave), 0, st, a);
      VI_HIP(hipGetLastError());
      VI_HIP(hipEventRecord(ev.b, st));
      VI_HIP(hipMemcpyAsync(h_new.data(), table[tc ^ 1].p, nlists * dim * sizeof(float), hipMemcpyDeviceToHost, st));
      VI_HIP(hipStreamSynchronize(st));
      res->ms_means_kernel += elapsed_ms(ev.a, ev.b);
      // read: every record's values (and its ordinal on the gather path) and the old table; written: the new table
      res->means_bytes += n * (uint64_t)dim * 4 + (cur_p ? n * 4 : 0) + 2 * nlists * (uint64_t)dim * 4;
    }
    const uint64_t changed = refine_changed_words((const uint32_t *)h_table.data(), (const uint32_t *)h_new.data(), nlists * dim);
    const double t1 = now_ms();
    res->ms_means += (float)(t1 - t0);
    // ---- labels: the coarse step of C' over every stored row, in ordinal order ----
    {
      DeviceIndex coarse;  // the table, and one list that holds its first row
      std::vector<uint64_t> list_off(nlists + 1, 1);
      list_off[0] = 0;
      const std::vector<uint32_t> member_rows(1, 0u);
      VI_TRY(device_index_from_rows(old.device, old.order, dim, table[tc ^ 1].p, nlists, table[tc ^ 1].p, list_off, member_rows, nullptr,
                                    nullptr, &coarse));
      const vi_status s = with_search_context(old, [&](SearchContext &ctx) -> vi_status {
        StoredRowsWalk walk(64);
        VI_TRY(order_scratch.reserve(std::min(n, walk.chunk_rows)));
        return walk.run(old, ctx, all_rows, [&](const RowChunk &c) -> vi_status {
          SearchIO io;
          io.queries = ctx.ws.q.p;
          io.on_device = true;
          io.nq = c.m;
          io.k = 1;
          io.n_probe = 1;
          io.probes_out = lab_ord.p + c.q0;
          io.order_out = order_scratch.p;
          return device_index_search(coarse, io);
        });
      });
      if (s != VI_OK) { (void)hipGetLastError(); return s; }
      VI_HIP(hipSetDevice(old.device));
    }
    // ---- lists: labels by position, the moved records, the stable grouping, the next order ----
    unsigned long long moved = 0;
    VI_HIP(hipMemsetAsync(d_moved.p, 0, 8, st));
    hipLaunchKernelGGL(relabel_kernel, grid_1d(n), dim3(256), 0, st, lab_ord.p, cur_p, cur_lab[cc].p, n, lab_pos.p, d_moved.p);
    VI_HIP(hipGetLastError());
    VI_HIP(hipMemcpyAsync(&moved, d_moved.p, 8, hipMemcpyDeviceToHost, st));
    VI_TRY(group_ids_by_label_device(lab_pos.p, n, nlists, order, seg, &seg_host, st));  // (synchronises st)
    if (seg_host.size() != nlists + 1 || seg_host[nlists] != n) return fail(VI_ERR_OTHER, "refine: a record was assigned to no list");
    hipLaunchKernelGGL(compose_kernel, grid_1d(n), dim3(256), 0, st, order.p, cur_p, lab_pos.p, n, cur[cc ^ 1].p, cur_lab[cc ^ 1].p);
    VI_HIP(hipGetLastError());
    VI_HIP(hipStreamSynchronize(st));
    cc ^= 1;
    cur_p = cur[cc].p;
    tc ^= 1;
    h_table.swap(h_new);
    res->ms_label += (float)(now_ms() - t1);
    res->iterations_run = it + 1;
    if (refine_fixed_point(moved, changed)) break;  // every later iteration would be the identity
  }
  {  // records whose list after the call differs from their list before it
    unsigned long long moved = 0;
    VI_HIP(hipMemsetAsync(d_moved.p, 0, 8, st));
    hipLaunchKernelGGL(relabel_kernel, grid_1d(n), dim3(256), 0, st, lab_ord.p, (const uint32_t *)nullptr, lab0.p, n, (uint32_t *)nullptr,
                       d_moved.p);
    VI_HIP(hipGetLastError());
    VI_HIP(hipMemcpyAsync(&moved, d_moved.p, 8, hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
    res->moved = moved;
  }
  // ---- the new index: layout, re-home, table, images ----
  const double t2 = now_ms();
  std::vector<uint64_t> full_len(nlists);
  res->new_len.resize(nlists);
  for (uint64_t l = 0; l < nlists; ++l) {
    full_len[l] = seg_host[l + 1] - seg_host[l];
    res->new_len[l] = (uint32_t)full_len[l];
    res->lists_emptied += res->old_len[l] != 0 && full_len[l] == 0;
  }
  DevBuf<uint32_t> block_list;
  VI_TRY(lay_out_from_old(ix, old, full_len.data(), &block_list));
  if (ix->nvec_resident != n) return fail(VI_ERR_OTHER, "refine: the new layout does not hold every record");
  const uint64_t total_blocks = ix->lists.nblocks;
  {
    RehomeArgs a{(const float4 *)old.lists.blocks.p, old.ext_ids.p, old.timestamps.p, old.list_first_block.p, lay.prefix.p, (uint32_t)nlists,
                 dq, cur_p, seg.p, ix->list_first_block.p, ix->list_len.p, block_list.p, total_blocks, (float4 *)ix->lists.blocks.p,
                 ix->ext_ids.p, ix->timestamps.p};
    VI_HIP(hipEventRecord(ev.a, st));
    hipLaunchKernelGGL(rehome_blocks_kernel, dim3((uint32_t)((total_blocks + kRehomeWaves - 1) / kRehomeWaves)), dim3(kRehomeWaves * kWave),
                       0, st, a);
    VI_HIP(hipGetLastError());
    VI_HIP(hipEventRecord(ev.b, st));
    VI_HIP(hipStreamSynchronize(st));
    res->ms_rehome_kernel = elapsed_ms(ev.a, ev.b);
    // read + written: every new block once each way (blocks, ids, timestamps), less what pad lanes do not read; the order
    res->rehome_bytes = 2 * total_blocks * ((uint64_t)dq * kWave * 16 + kWave * 16) + n * 4;
  }
  VI_TRY(coarse_table_from_rows(ix, table[tc].p));
  const double t3 = now_ms();
  res->ms_rehome = (float)(t3 - t2);
  VI_TRY(prepare_rank_images(ix));
  res->ms_images = (float)(now_ms() - t3);
  res->table.swap(h_table);
  return VI_OK;
}

// One shard file from the blocks of a resident index, the frame by the routines shard_save_to uses (shards.cpp:
// byte-identical): cids = the shard's lists in file order, their centroid vectors cvecs_host (cids.size() x dim).  The
// file goes to `path` (a temporary name of the caller's); a file left short by a failed write is removed.
vi_status shard_export_blocks(const DeviceIndex &ix, const std::string &path, uint64_t shard_id, const std::vector<uint64_t> &cids,
                              const float *cvecs_host, ShardExportWs &ws, DevBuf<uint64_t> &id0_buf, uint64_t *bytes_out) {
  hipStream_t st = ix.stream;
  VI_HIP(hipSetDevice(ix.device));
  VI_TRY(ensure_fetch_layout(ix, st));
  const FetchState &lay = ix.fetch;
  const uint32_t nl = (uint32_t)cids.size(), dim = ix.dim;
  std::vector<uint64_t> counts(nl);
  uint64_t nrec = 0;
  for (uint32_t i = 0; i < nl; ++i) {
    if (cids[i] >= ix.nlists) return fail(VI_ERR_INVALID_DATA, "shard %llu names a list the index does not hold", (unsigned long long)shard_id);
    counts[i] = lay.h_len[cids[i]];
    nrec += counts[i];
  }
  if (nrec >= 0xFFFFFFFFull) return fail(VI_ERR_OTHER, "shard with more than 2^32 records");
  const ShardPlan pl(dim, counts);
  const uint64_t data_off = pl.data_off, total = pl.total;
  VI_TRY(ws.image.reserve(total + 16));
  if (ws.host_cap < total) {
    if (ws.host) (void)hipHostFree(ws.host);
    ws.host = nullptr;
    ws.host_cap = 0;
    VI_HIP(hipHostMalloc((void **)&ws.host, total + 16));
    ws.host_cap = total;
  }
  std::vector<uint64_t> k_slot0, k_id0, k_dst;
  std::vector<uint32_t> k_first;
  for (uint32_t i = 0, first = 0; i < nl; ++i) {
    if (counts[i]) {
      k_slot0.push_back(refine_slot(lay.h_first[cids[i]], 0));
      k_id0.push_back(lay.h_prefix[cids[i]]);
      k_dst.push_back(pl.records(i));
      k_first.push_back(first);
    }
    first += (uint32_t)counts[i];
  }
  if (nrec) {
    VI_TRY(upload(ws.d_src, k_slot0.data(), k_slot0.size(), st));
    VI_TRY(upload(id0_buf, k_id0.data(), k_id0.size(), st));
    VI_TRY(upload(ws.d_dst, k_dst.data(), k_dst.size(), st));
    VI_TRY(upload(ws.d_first, k_first.data(), k_first.size(), st));
    BlockExportArgs a{ix.lists.blocks.p, ix.ext_ids.p, ix.timestamps.p, ws.d_src.p, id0_buf.p, ws.d_dst.p, ws.d_first.p,
                      (uint32_t)k_slot0.size(), dim, ix.dq, (uint32_t)pl.stride, nrec, ws.image.p};
    hipLaunchKernelGGL(export_block_records_kernel, dim3((uint32_t)((nrec + 3) / 4)), dim3(256), 0, st, a);
    VI_HIP(hipGetLastError());
    VI_HIP(hipMemcpyAsync(ws.host + data_off, ws.image.p + data_off, total - data_off, hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));  // (k_* are read by the copies above)
  }
  std::vector<const void *> cvecs(nl);
  for (uint32_t i = 0; i < nl; ++i) cvecs[i] = cvecs_host + (uint64_t)i * dim;
  shard_frame_write(ws.host, pl, shard_id, cids.data(), cvecs.data());
  if (bytes_out) *bytes_out = total;
  return shard_image_write(path, ws.host, total, true);
}

}  // namespace vi
