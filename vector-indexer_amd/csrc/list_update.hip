// list_update.hip — the resident half of vi_indexer_add_records, of vi_indexer_retain / vi_indexer_remove_ids and of
// vi_indexer_upsert_records: a new DeviceIndex from the blocks of the old one, without re-reading a shard file.  One
// route, device_index_update, with two optional halves — what goes (a keep filter) and what joins (rows):
//
//   refuse_update, begin_update (list_blocks.hpp; defined here): the refusals, a fresh index on the old one's device
//     -> the records every list keeps: with a filter, kept_count_kernel and one read-back; without, the old lengths the
//        caller read (nothing is launched)
//     -> on the host: new length = kept + rows received, the new layout from the new lengths, and the list of every new
//        block (lay_out_from_old)
//     -> one wave per NEW block, lane = vector (update_blocks_kernel).  A block whose 64 positions are the records of one
//        old block is a straight copy of it.  Pad lanes get what every index upload leaves there: zero vectors, external
//        id ~0, timestamp 0.  Every word of the new blocks / ext_ids / timestamps is written exactly once.  The copy, the
//        fill of a lane's column and the pad values are list_blocks.hpp's, shared with a refine's rehome_blocks_kernel.
//     -> finish_update: the launch between two events (launch_block_kernel), then prepare_rank_images: norms, images and
//        the rank mode's statistics, by the code a load runs.
//
// What goes.  keep.allow holds one bit per old slot, pad slots 0.  kept_count_kernel, one wave per list: lanes stride over
// the list's old blocks; the popcount of each block's allow word, scanned across the wave with a carry from stride to
// stride, is the number of kept records of the list in front of the block (block_prefix) and, at the end, kept[l].  New
// position p < kept[l] is a gather: it looks its source up, the old block by binary search over the list's block_prefix,
// the lane inside it as the (p - prefix)-th set bit of the block's allow word.  Sources inside a wave ascend and are
// mostly adjacent; the writes are whole rows.  No filter: kept[l] is the old length, every old record keeps its position,
// and allow, block_prefix and kept are never read.
//
// What joins.  The new rows (device, row-major, uploaded once) get their label from the coarse step of the old index with
// n_probe = 1 (device_index_label_rows: device_index_label_chunk, a search with probes_out, chunk by chunk) — the first probe of the
// reference's coarse step (ivf_index.rs:205-220), whatever engine ranks it — and are grouped by label, ascending call
// index inside a label (group_ids_by_label_device).  Position kept[l] <= p < new_len[l] reads its row from the row-major
// upload (as repack_rows_kernel reads it).  No rows: new_len == kept everywhere, no lane is new, and rows, order, seg,
// row_ext and row_ts are never read.
//
// A straight copy needs a list that lost nothing AND a block of old records only: equal lengths do not mean equal
// positions (one record out, one in).  A list may have no old block at all (an emptied list that receives rows): it never
// searches block_prefix.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_index.hpp"
#include "list_blocks.hpp"
#include "search_internal.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;
constexpr uint64_t kLabelChunk = 65536;    // rows per coarse step

struct CountArgs {
  const uint64_t *allow;                   // per old block
  const uint32_t *old_first, *old_len;     // per list
  uint32_t nlists;
  uint32_t *block_prefix;                  // per old block: kept records of its list in front of it
  uint32_t *kept;                          // per list
};

__global__ void __launch_bounds__(kBlockWaves * kWave) kept_count_kernel(CountArgs a) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint32_t l = blockIdx.x * kBlockWaves + (threadIdx.x >> 6);
  if (l >= a.nlists) return;
  const uint32_t first = a.old_first[l], nblk = (a.old_len[l] + kWave - 1) / kWave;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nblk; base += kWave) {  // (wave-uniform)
    const uint32_t b = base + lane;
    const uint32_t c = b < nblk ? (uint32_t)__popcll(a.allow[first + b]) : 0u;
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d, kWave);
      if ((int)lane >= d) incl += up;
    }
    if (b < nblk) a.block_prefix[first + b] = carry + incl - c;
    carry += __shfl(incl, kWave - 1, kWave);
  }
  if (lane == 0) a.kept[l] = carry;
}

struct UpdateArgs {
  OldBlocks old;                           // the old index
  const uint32_t *old_first, *old_len;     // per list
  // what is kept of it.  allow == nullptr: everything, and none of the three is read
  const uint64_t *allow;                   // per old block
  const uint32_t *block_prefix;            // per old block (kept_count_kernel)
  const uint32_t *kept;                    // per list: kept records (kept_count_kernel)
  // the new layout
  const uint32_t *new_first, *new_len;     // per list: new_len = kept + rows received
  const uint32_t *block_list;              // per new block: its list
  uint64_t nblocks;                        // new blocks
  // the new rows, grouped by list: list l receives rows order[seg[l] .. seg[l + 1]) in that order, behind its kept records.
  // No rows: new_len == kept, and none of the five is read
  const float *rows;                       // n x dim
  const uint64_t *row_ext, *row_ts;        // per row, resolved on the host
  const uint32_t *order, *seg;
  uint32_t dim, dq;
  NewBlocks out;
};

// the r-th (from 0) set bit of w, which has more than r set bits: halve the word, step into the half that holds it
__device__ __forceinline__ uint32_t nth_set_bit(uint64_t w, uint32_t r) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t width = 32; width; width >>= 1) {
    const uint32_t c = (uint32_t)__popcll(w & ((1ull << width) - 1ull));
    if (r >= c) { r -= c; w >>= width; pos += width; }
  }
  return pos;
}

// quad qd of a row-major row of `dim` values, zero beyond dim (as repack_rows_kernel reads an upload)
__device__ __forceinline__ float4 row_quad(const float *v, uint32_t qd, uint32_t dim) {
  float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
  const uint32_t e = qd * 4;
  if (e + 0 < dim) x.x = v[e + 0];
  if (e + 1 < dim) x.y = v[e + 1];
  if (e + 2 < dim) x.z = v[e + 2];
  if (e + 3 < dim) x.w = v[e + 3];
  return x;
}

// New position p = 64 j + lane of list l is kept record p of the old list where p < kept (a gather where the list lost
// records, the old position where it lost none), row order[seg[l] + p - kept] of the upload where kept <= p < new_len, a
// pad lane behind that.  kDrops: there is a filter (else kept == old_len and allow / block_prefix / kept are not read);
// kRows: there may be rows (else kept == new_len and rows / order / seg / row_ext / row_ts are not read).  One body, the
// three instantiations finish_update chooses from: the two tests cost the remove route 1 % as kernel arguments (r14).
template <bool kDrops, bool kRows>
__global__ void __launch_bounds__(kBlockWaves * kWave) update_blocks_kernel(UpdateArgs a) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  const uint64_t b = (uint64_t)blockIdx.x * kBlockWaves + (threadIdx.x >> 6);
  if (b >= a.nblocks) return;
  const uint32_t l = a.block_list[b];
  const uint32_t j = (uint32_t)(b - a.new_first[l]);           // block of the list
  const uint32_t old_len = a.old_len[l], new_len = a.new_len[l], old_first = a.old_first[l];
  const uint32_t kept = !kDrops ? old_len : !kRows ? new_len : a.kept[l];
  const uint32_t dq = a.dq;
  const bool lost_nothing = kept == old_len;                   // (wave-uniform) kept positions are the old ones
  // a straight copy needs both: a list that loses one record and receives one keeps its length and moves every position
  if (lost_nothing && j * kWave + (kWave - 1) < old_len) {     // ... and all 64 are old records
    copy_old_block(a.old, a.out, dq, old_first + j, b, lane);
    return;
  }
  const uint32_t p = j * kWave + lane;                         // position inside the new list (new_len < 2^32 - 64)
  const bool is_old = p < kept, is_new = kRows && !is_old && p < new_len;
  uint32_t sb = j, sl = lane;                                  // source block of the old list, lane inside it
  if (kDrops && !lost_nothing && j * kWave < kept) {           // (wave-uniform) the block holds kept records that moved
    // kept < old_len here, so there is a filter and the list had records: old_nblk >= 1.  A list without old blocks (an
    // emptied list that receives rows) has kept == old_len == 0 and never searches; a block of new rows only does not either.
    const uint32_t old_nblk = (old_len + kWave - 1) / kWave;
    const uint32_t ps = is_old ? p : 0u;                       // (the other lanes search too, and read nothing afterwards)
    // the last old block whose prefix is <= ps: it holds kept record ps (blocks with nothing kept share the prefix of
    // the block behind them, so they are never the last).  The trip count depends on old_nblk alone: wave-uniform.
    uint32_t lo = 0, hi = old_nblk;
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (a.block_prefix[old_first + mid] <= ps) lo = mid; else hi = mid;
    }
    sb = lo;
    sl = is_old ? nth_set_bit(a.allow[old_first + sb], ps - a.block_prefix[old_first + sb]) : 0u;
  }
  const float4 *src = a.old.blocks + ((uint64_t)(old_first + sb) * dq) * kWave + sl;  // (read only where is_old)
  const uint64_t old_slot = (uint64_t)(old_first + sb) * kWave + sl;
  uint32_t row = 0;
  if (is_new) row = a.order[a.seg[l] + (p - kept)];
  const float *v = a.rows + (size_t)row * a.dim;               // (read only where is_new)
  fill_block_column(a.out.blocks + (b * dq) * kWave + lane, dq, [&](uint32_t qd, float4 (&t)[4]) {
    if (is_old) {
      load_block_quads(src, qd, t);
    } else if (is_new) {
#pragma unroll
      for (uint32_t i = 0; i < 4; ++i) t[i] = row_quad(v, qd + i, a.dim);
    }
  });
  const uint64_t slot = b * kWave + lane;
  a.out.ext[slot] = is_old ? a.old.ext[old_slot] : is_new ? a.row_ext[row] : kPadExtId;
  a.out.ts[slot] = is_old ? a.old.ts[old_slot] : is_new ? a.row_ts[row] : kPadTimestamp;
}

// ... and an update ends with, once lay_out_from_old has run: the old index, the new layout and the new storage filled
// in, the block kernel timed between two events (one wave per new block), prepare_rank_images.
vi_status finish_update(const DeviceIndex &old, DeviceIndex *ix, const DevBuf<uint32_t> &block_list, UpdateArgs a, float *ms_kernel,
                        uint64_t *kernel_bytes) {
  const uint64_t total_blocks = ix->lists.nblocks;
  if (total_blocks) {
    a.old = old_blocks_of(old);
    a.old_first = old.list_first_block.p; a.old_len = old.list_len.p;
    a.new_first = ix->list_first_block.p; a.new_len = ix->list_len.p;
    a.block_list = block_list.p; a.nblocks = total_blocks;
    a.dim = ix->dim; a.dq = ix->dq;
    a.out = new_blocks_of(ix);
    // (rows without a filter, a filter without rows, both; neither — nothing changes — runs as the first: no lane is new)
    void (*kernel)(UpdateArgs) = !a.allow ? update_blocks_kernel<false, true> : !a.rows ? update_blocks_kernel<true, false>
                                                                                         : update_blocks_kernel<true, true>;
    VI_TRY(launch_block_kernel(kernel, a, total_blocks, ix->stream, ms_kernel));  // (the block list and the caller's scratch are freed on return)
    if (kernel_bytes) *kernel_bytes = block_bytes_moved(total_blocks, ix->dq);
  }
  return prepare_rank_images(ix);
}

}  // namespace

vi_status refuse_update(const DeviceIndex &old, const char *refusal) {
  if (old.stripe_world > 1) return fail(VI_ERR_INVALID_INPUT, "%s", refusal);
  if (!old.timestamps.p || !old.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "the index keeps no ids or timestamps");
  return VI_OK;
}

vi_status begin_update(const DeviceIndex &old, DeviceIndex *ix) {
  VI_TRY(init_device_index(ix, old.device, old.dim, old.nlists));
  ix->order = old.order;
  ix->timing = old.timing;
  return VI_OK;
}

// One chunk of a labelling: labels_dev[i] = the first probe of ix's coarse step for row i of the m rows at rows_dev.
// order_scratch: m words (the coarse step writes the candidate-order ranks too: all zero at one probe).
vi_status device_index_label_chunk(const DeviceIndex &ix, const float *rows_dev, uint64_t m, uint32_t *labels_dev, uint32_t *order_scratch) {
  SearchIO io;
  io.queries = rows_dev;
  io.on_device = true;
  io.nq = m;
  io.k = 1;
  io.n_probe = 1;
  io.probes_out = labels_dev;
  io.order_out = order_scratch;
  return device_index_search(ix, io);
}

// labels_dev[i] = the list the reference's coarse step probes first for row i: the old index's own coarse step, n_probe 1
vi_status device_index_label_rows(const DeviceIndex &ix, const float *rows_dev, uint64_t n, uint32_t *labels_dev) {
  if (n == 0) return VI_OK;
  if (ix.nlists == 0) return fail(VI_ERR_INVALID_INPUT, "the index has no list to add to");
  VI_HIP(hipSetDevice(ix.device));
  DevBuf<uint32_t> order_scratch;
  VI_TRY(order_scratch.reserve(std::min(n, kLabelChunk)));
  for (uint64_t at = 0; at < n; at += kLabelChunk)
    VI_TRY(device_index_label_chunk(ix, rows_dev + at * ix.dim, std::min(kLabelChunk, n - at), labels_dev + at, order_scratch.p));
  return VI_OK;
}

// The index `old` without the records whose allow bit in `keep` is 0 (keep == nullptr: with all of them) and with n rows
// appended (n == 0: with none): the kept records of list l close up in their old order, rows order_dev[seg_host[l] ..
// seg_host[l + 1]) of rows_dev follow them.  Complete on return; `old` and `keep` are only read.
vi_status device_index_update(const DeviceIndex &old, const SlotFilter *keep, const float *rows_dev, uint64_t n,
                              const uint32_t *order_dev, const uint32_t *seg_dev, const std::vector<uint64_t> &seg_host,
                              const uint64_t *row_ext_dev, const uint64_t *row_ts_dev, const std::vector<uint32_t> &old_len_host,
                              DeviceIndex *ix, float *ms_kernel, uint64_t *kernel_bytes) {
  const uint64_t nlists = old.nlists;
  VI_TRY(refuse_update(old, !keep ? "a partitioned index takes no records" : n == 0 ? "a partitioned index gives no records up"
                                  : "a partitioned index takes no records and gives none up"));
  VI_TRY(begin_update(old, ix));
  if (ms_kernel) *ms_kernel = 0.0f;
  if (kernel_bytes) *kernel_bytes = 0;
  if (keep && keep->owner_serial != old.serial) return fail(VI_ERR_INVALID_INPUT, "the filter was made from another index");
  if (n && (seg_host.size() != nlists + 1 || seg_host[nlists] != n)) return fail(VI_ERR_OTHER, "update: grouping does not match the index");
  if (!keep && old_len_host.size() != nlists) return fail(VI_ERR_OTHER, "update: the list lengths do not match the index");
  UpdateArgs a{};
  // ---- the kept records of every list: all of them, or a count pass that also leaves those in front of every old block ----
  DevBuf<uint32_t> block_prefix, d_kept;
  std::vector<uint32_t> counted;
  if (keep) {
    VI_TRY(block_prefix.reserve(std::max<uint64_t>(1, old.lists.nblocks)));
    VI_TRY(d_kept.reserve(std::max<uint64_t>(1, nlists)));
    counted.resize(nlists);
    if (nlists) {
      hipStream_t st = ix->stream;
      CountArgs c{keep->allow.p, old.list_first_block.p, old.list_len.p, (uint32_t)nlists, block_prefix.p, d_kept.p};
      hipLaunchKernelGGL(kept_count_kernel, dim3((uint32_t)((nlists + kBlockWaves - 1) / kBlockWaves)),
                         dim3(kBlockWaves * kWave), 0, st, c);
      VI_HIP(hipGetLastError());
      VI_HIP(hipMemcpyAsync(counted.data(), d_kept.p, nlists * 4, hipMemcpyDeviceToHost, st));
      VI_HIP(hipStreamSynchronize(st));
    }
    a.allow = keep->allow.p; a.block_prefix = block_prefix.p; a.kept = d_kept.p;
  }
  const std::vector<uint32_t> &kept = keep ? counted : old_len_host;
  // the new layout from the new lengths: lists back to back in list order, each padded to whole blocks (as a load lays them)
  std::vector<uint64_t> full_len(nlists);
  for (uint64_t l = 0; l < nlists; ++l) full_len[l] = (uint64_t)kept[l] + (n ? seg_host[l + 1] - seg_host[l] : 0);
  DevBuf<uint32_t> d_block_list;
  VI_TRY(lay_out_from_old(ix, old, full_len.data(), &d_block_list));  // (the new first / len are in place for the kernel)
  if (keep && ix->nvec_resident != keep->num_allowed + n) return fail(VI_ERR_OTHER, "update: the filter's count does not match its allow words");
  if (n) {
    a.rows = rows_dev; a.row_ext = row_ext_dev; a.row_ts = row_ts_dev;
    a.order = order_dev; a.seg = seg_dev;
  }
  return finish_update(old, ix, d_block_list, a, ms_kernel, kernel_bytes);
}

}  // namespace vi
