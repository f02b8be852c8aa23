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
//   split    only with a rule (vi_indexer_rebalance), in its first split_rounds iterations: the plan over the lengths the
//            iteration starts with (rebalance_rules.hpp), the pairs' two-means over the old blocks (list_split.hip), the
//            two centres of every split pair into C' — the table the labels are made against and the fixed-point test sees
//   labels   a coarse-only index of the new table (device_index_from_rows, whose one list holds one row of the table, so
//            that every launch of prepare_rank_images has work) and the walk over stored records (StoredRowsWalk):
//            chunks of stored rows of the OLD index, in ordinal order, through that index's coarse step at n_probe 1 —
//            the labeller of an add, chunk for chunk (device_index_label_chunk).  The search kernels are the ones every
//            search runs.
//   lists    relabel_kernel brings the labels into position order and counts the moved records; the stable grouping of
//            positions by label (group_ids_by_label_device) gives the next order; compose_kernel maps it back to old
//            ordinals.
// After the last iteration, once: the new layout from the new lengths (lay_out_from_old), rehome_blocks_kernel — one wave
// per NEW block, lane = new position, source = the old slot of ordinal cur[seg[l] + p]; what it shares with an update's
// block kernel is list_blocks.hpp, as are the frame it starts in (refuse_update, begin_update) and its launch — the new table
// (coarse_table_from_rows) and prepare_rank_images, the load's own code.  The shard files of the new index are written by
// shard_export.hip.
//
// Device memory beside the old and the new index: eight u32 words per record (the old and the new labels by ordinal, the
// new labels by position, cur and cur_lab twice each, the grouping's output) plus the grouping's scratch, one chunk of
// rows in the walk's search context, two tables.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_index.hpp"
#include "list_blocks.hpp"
#include "record_fetch.hpp"
#include "refine_rules.hpp"
#include "search_internal.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;
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
  OldBlocks old;                           // the old index
  const uint32_t *old_first;               // per list
  const uint64_t *old_prefix;              // per list
  uint32_t nlists, dq;
  // the assignment: list l holds the records of old ordinals cur[seg[l] .. seg[l + 1]), in that order
  const uint32_t *cur, *seg;
  // the new layout
  const uint32_t *new_first, *new_len;     // per list
  const uint32_t *block_list;              // per new block: its list
  uint64_t nblocks;
  NewBlocks out;
};

// One wave per NEW block, lane = new position.  Vector, external id and timestamp of position p of list l come from the
// old slot of ordinal cur[seg[l] + p]; the rest is list_blocks.hpp: a pad lane's values, the fill of the lane's column,
// and the straight copy of a block whose 64 sources are one whole old block in order — every block of a list nothing
// joined and nothing left, but its last.
__global__ void __launch_bounds__(kBlockWaves * kWave) rehome_blocks_kernel(RehomeArgs a) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t b = (uint64_t)blockIdx.x * kBlockWaves + (threadIdx.x >> 6);
  if (b >= a.nblocks) return;
  const uint32_t l = a.block_list[b];
  const uint32_t p = (uint32_t)(b - a.new_first[l]) * kWave + lane;
  const bool valid = p < a.new_len[l];
  uint64_t src_slot = 0;
  if (valid) src_slot = refine_slot_of_ordinal(a.old_prefix, a.old_first, a.nlists, a.cur[a.seg[l] + p]);
  const uint32_t dq = a.dq;
  const uint64_t slot0 = __shfl(src_slot, 0, kWave);
  if (__all(valid && src_slot == slot0 + lane) && (slot0 & 63u) == 0) {  // (wave-uniform) one whole old block, in order
    copy_old_block(a.old, a.out, dq, slot0 >> 6, b, lane);
    return;
  }
  const float4 *src = a.old.blocks + ((src_slot >> 6) * dq) * kWave + (src_slot & 63u);  // (read only where valid)
  fill_block_column(a.out.blocks + (b * dq) * kWave + lane, dq, [&](uint32_t qd, float4 (&t)[4]) {
    if (valid) load_block_quads(src, qd, t);
  });
  const uint64_t slot = b * kWave + lane;
  a.out.ext[slot] = valid ? a.old.ext[src_slot] : kPadExtId;
  a.out.ts[slot] = valid ? a.old.ts[src_slot] : kPadTimestamp;
}

inline dim3 grid_1d(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

}  // namespace

vi_status device_index_refine(const DeviceIndex &old, const float *table_host, uint64_t iters, DeviceIndex *ix, RefineResult *res,
                              const SplitRule *rule, SplitStats *split) {
  *res = RefineResult{};
  if (rule && !split) return fail(VI_ERR_OTHER, "refine: a split rule without a place for its counts");
  if (split) *split = SplitStats{};
  const uint64_t nlists = old.nlists, n = old.nvec_resident;
  const uint32_t dim = old.dim, dq = old.dq;
  VI_TRY(refuse_update(old, "a partitioned index is not refined"));
  if (iters == 0 || n == 0 || nlists == 0) return fail(VI_ERR_OTHER, "refine: nothing to do");
  VI_TRY(begin_update(old, ix));
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

  EventSpans<1> ev;  // list_means_kernel
  VI_TRY(ev.create(true));
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
      VI_TRY(ev.begin(0, st));
      hipLaunchKernelGGL(list_means_kernel, dim3((uint32_t)nlists, (dim + kMeanCols - 1) / kMeanCols), dim3(kWave), 0, st, a);
      VI_HIP(hipGetLastError());
      VI_TRY(ev.end(0, st));
      VI_HIP(hipMemcpyAsync(h_new.data(), table[tc ^ 1].p, nlists * dim * sizeof(float), hipMemcpyDeviceToHost, st));
      VI_HIP(hipStreamSynchronize(st));
      res->ms_means_kernel += ev.ms(0);
      // read: every record's values (and its ordinal on the gather path) and the old table; written: the new table
      res->means_bytes += n * (uint64_t)dim * 4 + (cur_p ? n * 4 : 0) + 2 * nlists * (uint64_t)dim * 4;
    }
    uint64_t changed = refine_changed_words((const uint32_t *)h_table.data(), (const uint32_t *)h_new.data(), nlists * dim);
    double t1 = now_ms();
    res->ms_means += (float)(t1 - t0);
    if (rule && it < rule->split_rounds) {
      // ---- split (a rebalance): the plan from the lengths this iteration starts with, the pairs' centres into C' ----
      std::vector<uint64_t> len(nlists);
      for (uint64_t l = 0; l < nlists; ++l) len[l] = cur_p ? seg_host[l + 1] - seg_host[l] : (uint64_t)lay.h_len[l];
      const std::vector<RebalancePair> pairs = rebalance_plan(len.data(), nlists, rule->split_factor, rule->receiver_max_len, rule->max_splits);
      if (!pairs.empty()) {
        const ListMembers members{(const float4 *)old.lists.blocks.p, dq, dim, (uint32_t)nlists, old.list_first_block.p, old.list_len.p,
                                  lay.prefix.p, cur_p, seg.p};
        VI_TRY(device_split_lists(members, pairs, len.data(), rule->split_iters, h_new.data(), st, split));
        // the table the labels are made against, and the one the fixed-point test sees
        VI_HIP(hipMemcpyAsync(table[tc ^ 1].p, h_new.data(), nlists * dim * sizeof(float), hipMemcpyHostToDevice, st));
        VI_HIP(hipStreamSynchronize(st));
        changed = refine_changed_words((const uint32_t *)h_table.data(), (const uint32_t *)h_new.data(), nlists * dim);
      }
      const double ts = now_ms();
      split->ms += (float)(ts - t1);
      t1 = ts;
    }
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
          return device_index_label_chunk(coarse, ctx.ws.q.p, c.m, lab_ord.p + c.q0, order_scratch.p);
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
    const RehomeArgs a{old_blocks_of(old), old.list_first_block.p, lay.prefix.p, (uint32_t)nlists, dq, cur_p, seg.p,
                       ix->list_first_block.p, ix->list_len.p, block_list.p, total_blocks, new_blocks_of(ix)};
    VI_TRY(launch_block_kernel(rehome_blocks_kernel, a, total_blocks, st, &res->ms_rehome_kernel));
    res->rehome_bytes = block_bytes_moved(total_blocks, dq) + n * 4;  // (... and the order)
  }
  VI_TRY(coarse_table_from_rows(ix, table[tc].p));
  const double t3 = now_ms();
  res->ms_rehome = (float)(t3 - t2);
  VI_TRY(prepare_rank_images(ix));
  res->ms_images = (float)(now_ms() - t3);
  res->table.swap(h_table);
  return VI_OK;
}

}  // namespace vi
