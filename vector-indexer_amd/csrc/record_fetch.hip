// record_fetch.hip — reads records back from a resident index (record_fetch.hpp): by external id, or a range of all of
// them in list order.
//
// A get has no persistent id -> slot map to ask.  It makes a hash table of the REQUESTED ids (id_table.hpp) with two
// values per entry, scans the external id of every resident slot through it once (fetch_match_kernel: the geometry and
// the cost of an id filter), and then answers every request row from its entry (fetch_resolve_gather_kernel).  An
// export walks the blocks of a range as they lie and turns each into rows (export_blocks_kernel).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_index.hpp"
#include "id_table.hpp"
#include "list_layout.hpp"
#include "record_fetch.hpp"

namespace vi {
namespace {

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kResolveBlocks = 2048;  // workgroups of the answer kernel: 8 per CU fill the chip, each loops over its rows
constexpr uint64_t kWhereNone = ~0ull;  // VI_WHERE_NONE

// ---- get: the scan ----
struct MatchArgs {
  ResidentLists lists;
  const uint64_t *ext_ids;
  IdTable t;
  uint32_t *first_slot, *count;  // [capacity + 1], kNoSlot / 0 before the launch
};

// The walk of list_layout.hpp, masked by the list length (a pad slot's id word is never read).  A requested id's slot leaves
// the lowest slot number and one count on its entry; lists lie in list order, so that is the first record in list order.
__global__ void __launch_bounds__(256) fetch_match_kernel(MatchArgs a) {
  for_each_resident_block(a.lists, [&](uint32_t block, uint32_t lane, bool resident, uint32_t, uint32_t) {
    if (!resident) return;
    const uint32_t slot = block * 64u + lane;
    const uint64_t e = id_table_find(a.t, a.ext_ids[slot]);
    if (e == kNoEntry) return;
    atomicMin(&a.first_slot[e], slot);
    atomicAdd(&a.count[e], 1u);
  });
}

// ---- get: the answers ----
struct ResolveArgs {
  IdTable t;
  const uint32_t *first_slot, *count;
  const uint64_t *ids;
  uint64_t n;
  const float4 *blocks;
  uint32_t dq, dim;
  const uint32_t *first_block;
  uint32_t nlists;
  const uint64_t *timestamps;  // or null: the index keeps none
  uint32_t world, rank;        // stripes (1, 0: whole lists)
  uint32_t *out_count;         // any of the four may be null
  float *out_values;
  uint64_t *out_ts, *out_where;
  uint32_t *out_slot;          // internal (resolve_records_by_id): the slot `where` names, kNoSlot for an absent id; or null
  unsigned long long *found;   // requests that found a record
  bool vec_store;              // dim % 4 == 0 and out_values 16-byte aligned
};

// request row i: its count, and the slot of its first record (kNoSlot: absent)
__device__ __forceinline__ uint32_t resolve_row(const ResolveArgs &a, uint64_t i, uint32_t *slot) {
  const uint64_t e = id_table_find(a.t, a.ids[i]);
  const uint32_t cnt = e == kNoEntry ? 0u : a.count[e];
  *slot = cnt ? a.first_slot[e] : kNoSlot;
  return cnt;
}

__device__ __forceinline__ void write_row_scalars(const ResolveArgs &a, uint64_t i, uint32_t cnt, uint32_t slot) {
  if (a.out_count) a.out_count[i] = cnt;
  if (a.out_ts) a.out_ts[i] = cnt && a.timestamps ? a.timestamps[slot] : 0ull;
  if (a.out_slot) a.out_slot[i] = slot;
  if (a.out_where) {
    uint64_t w = kWhereNone;
    if (cnt) {
      const uint32_t blk = slot / 64u, l = list_of_block(a.first_block, a.nlists, blk);
      const uint64_t p = (uint64_t)(blk - a.first_block[l]) * 64u + slot % 64u;
      w = ((uint64_t)l << 32) | full_position(p, a.world, a.rank);
    }
    a.out_where[i] = w;
  }
}

// GATHER: one wave per request row; the lane for quad qd reads blocks[(blk * dq + qd) * 64 + ln] as one float4 and
// stores it into the row — 16 bytes where the row allows it, else element by element, nothing past dim.  An absent id
// gets a row of zeros.  Without GATHER (values == NULL: "contains / how many") one thread per request row.
// The requests that found a record are counted in registers, summed per workgroup through LDS and added to a.found once
// per workgroup: one atomic per row on that one word set the pace of the whole kernel (12 ns per row at a million rows).
template <bool GATHER>
__global__ void __launch_bounds__(256) fetch_resolve_gather_kernel(ResolveArgs a) {
  __shared__ uint32_t block_hits;
  const uint32_t lane = threadIdx.x & 63u;
  if (threadIdx.x == 0) block_hits = 0;
  __syncthreads();
  uint32_t hits = 0;  // of this wave (wave-uniform)
  if (!GATHER) {
    for (uint64_t i0 = (uint64_t)blockIdx.x * 256u; i0 < a.n; i0 += (uint64_t)gridDim.x * 256u) {
      const uint64_t i = i0 + threadIdx.x;
      uint32_t slot = kNoSlot, cnt = 0;
      if (i < a.n) {
        cnt = resolve_row(a, i, &slot);
        write_row_scalars(a, i, cnt, slot);
      }
      hits += (uint32_t)__popcll(__ballot(cnt != 0));
    }
  } else {
    const uint32_t nquads = (a.dim + 3u) / 4u;
    for (uint64_t i = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); i < a.n; i += (uint64_t)gridDim.x * 4u) {  // (wave-uniform)
      uint32_t slot;
      const uint32_t cnt = resolve_row(a, i, &slot);
      if (lane == 0) write_row_scalars(a, i, cnt, slot);
      hits += cnt != 0;
      const uint64_t blk = slot / 64u, ln = slot % 64u;
      float *row = a.out_values + i * a.dim;
      for (uint32_t qd = lane; qd < nquads; qd += 64u) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (cnt) v = a.blocks[(blk * a.dq + qd) * 64u + ln];
        if (a.vec_store) {
          *reinterpret_cast<float4 *>(row + 4u * qd) = v;
        } else {
          const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (uint32_t c = 0; c < 4; ++c)
            if (4u * qd + c < a.dim) row[4u * qd + c] = e[c];
        }
      }
    }
  }
  if (lane == 0 && hits) atomicAdd(&block_hits, hits);
  __syncthreads();
  if (threadIdx.x == 0 && block_hits) atomicAdd(a.found, (unsigned long long)block_hits);
}

// ---- export ----
constexpr uint32_t kChunkQuads = 8;                    // a pass moves 8 quads = 128 B of each of the block's 64 rows
constexpr uint32_t kChunkDwords = 4 * kChunkQuads;
constexpr uint32_t kRowStride = kChunkDwords + 4;      // dwords; the pad keeps 16-byte alignment and spreads the rows over the banks

struct ExportArgs {
  const float4 *blocks;
  uint32_t dq, dim;
  const uint32_t *first_block, *list_len;
  const uint64_t *prefix;  // [nlists] records before each list in list order
  uint32_t nlists;
  const uint64_t *ext_ids, *timestamps;  // timestamps or null
  uint32_t block_lo;       // first block of the range
  uint64_t first, count;
  uint32_t world, rank;
  uint64_t *out_ids;       // any of the four may be null
  float *out_values;
  uint64_t *out_ts, *out_where;
  uint32_t *out_slot;      // internal (resolve_records_by_range): the slot of every row; or null
};

// One wave (one workgroup) per resident block that intersects [first, first + count).  The wave finds its list and the
// list-order ordinal of its lane 0, masks the lanes beyond the list length and outside the range, and writes one id, one
// timestamp and one `where` per lane.  The values: a pass reads kChunkQuads quads of the block as they lie (one
// global_load_dwordx4 per quad, 1 KiB contiguous), lays them into LDS as 64 row pieces of 128 B, and reads them back
// row-wise: VEC — lane i stores quad i % 8 of row 8 it + i / 8, so one store instruction covers 8 whole 128-B row
// pieces; otherwise (dim % 4 != 0 or unaligned rows) lane i stores dword i % 32 of row 2 it + i / 32: 2 pieces of 128 B.
// Consecutive rows of the output are consecutive ordinals, so a block's rows form one contiguous span.
template <bool VEC>
__global__ void __launch_bounds__(64) export_blocks_kernel(ExportArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[64 * kRowStride];
  const uint32_t lane = threadIdx.x, b = a.block_lo + blockIdx.x;
  const uint32_t l = list_of_block(a.first_block, a.nlists, b);
  const uint32_t p0 = (b - a.first_block[l]) * 64u;       // local position of lane 0
  const uint64_t ord0 = a.prefix[l] + p0;                 // ... and its ordinal in list order
  const bool valid = p0 + lane < a.list_len[l] && ord0 + lane >= a.first && ord0 + lane < a.first + a.count;
  const uint64_t vmask = __ballot(valid);
  if (!vmask) return;
  const int64_t j0 = (int64_t)ord0 - (int64_t)a.first;    // output row of lane 0 (negative where lane 0 is before the range)
  if (valid) {
    const uint64_t slot = (uint64_t)b * 64u + lane, j = (uint64_t)(j0 + lane);
    if (a.out_ids) a.out_ids[j] = a.ext_ids[slot];
    if (a.out_slot) a.out_slot[j] = (uint32_t)slot;
    if (a.out_ts) a.out_ts[j] = a.timestamps ? a.timestamps[slot] : 0ull;
    if (a.out_where) a.out_where[j] = ((uint64_t)l << 32) | full_position((uint64_t)p0 + lane, a.world, a.rank);
  }
  if (!a.out_values) return;
  const uint32_t nquads = (a.dim + 3u) / 4u;
  const float4 *blk = a.blocks + (uint64_t)b * a.dq * 64u;
  for (uint32_t q0 = 0; q0 < nquads; q0 += kChunkQuads) {
#pragma unroll
    for (uint32_t c = 0; c < kChunkQuads; ++c)
      if (q0 + c < nquads)  // (uniform)
        *reinterpret_cast<float4 *>(&tile[lane * kRowStride + 4u * c]) = blk[(uint64_t)(q0 + c) * 64u + lane];
    __syncthreads();
    if (VEC) {
      const uint32_t c = lane % kChunkQuads;
#pragma unroll
      for (uint32_t it = 0; it < kChunkQuads; ++it) {
        const uint32_t r = it * (64u / kChunkQuads) + lane / kChunkQuads;
        if (q0 + c < nquads && ((vmask >> r) & 1ull))
          *reinterpret_cast<float4 *>(a.out_values + (uint64_t)(j0 + r) * a.dim + 4u * (q0 + c)) =
              *reinterpret_cast<const float4 *>(&tile[r * kRowStride + 4u * c]);
      }
    } else {
      const uint32_t e = lane % kChunkDwords, d = 4u * q0 + e;
      for (uint32_t it = 0; it < kChunkDwords; ++it) {
        const uint32_t r = it * (64u / kChunkDwords) + lane / kChunkDwords;
        if (d < a.dim && ((vmask >> r) & 1ull)) a.out_values[(uint64_t)(j0 + r) * a.dim + d] = tile[r * kRowStride + e];
      }
    }
    __syncthreads();  // the pass has been read out before the next one is laid in
  }
}

// The wanted outputs of a host caller: stage() points p, the caller's pointer, at the context's staging for the kernels to
// write; copy_back brings them home.  A device caller's pointers and an output not wanted stay as they are.
struct Staged {
  const bool on_device;
  struct { void *user; const void *dev; size_t bytes; } o[4];
  int n = 0;
  template <typename T>
  vi_status stage(T *&p, DevBuf<T> &buf, uint64_t count) {
    if (on_device || !p) return VI_OK;
    VI_TRY(buf.reserve(count));
    o[n++] = {p, buf.p, count * sizeof(T)};
    p = buf.p;
    return VI_OK;
  }
  vi_status copy_back(hipStream_t st) const {
    for (int i = 0; i < n; ++i) VI_HIP(hipMemcpyAsync(o[i].user, o[i].dev, o[i].bytes, hipMemcpyDeviceToHost, st));
    return VI_OK;
  }
};

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

// the host copy of the layout and the prefix of the lengths, made by the first export (or mask filter) of an index under a
// lock of its own
vi_status ensure_fetch_layout(const DeviceIndex &ix, hipStream_t st) {
  FetchState &f = ix.fetch;
  std::lock_guard<std::mutex> lock(f.layout_mu);
  if (f.layout_ready) return VI_OK;
  const uint64_t nl = ix.nlists;
  f.h_first.resize(nl);
  f.h_len.resize(nl);
  f.h_prefix.assign(nl + 1, 0);
  if (nl) {
    VI_HIP(hipMemcpyAsync(f.h_first.data(), ix.list_first_block.p, nl * 4, hipMemcpyDeviceToHost, st));
    VI_HIP(hipMemcpyAsync(f.h_len.data(), ix.list_len.p, nl * 4, hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
  }
  for (uint64_t l = 0; l < nl; ++l) f.h_prefix[l + 1] = f.h_prefix[l] + f.h_len[l];
  VI_TRY(f.prefix.reserve(std::max<uint64_t>(1, nl)));
  if (nl) {
    VI_HIP(hipMemcpyAsync(f.prefix.p, f.h_prefix.data(), nl * 8, hipMemcpyHostToDevice, st));
    VI_HIP(hipStreamSynchronize(st));
  }
  f.layout_ready = true;
  return VI_OK;
}

namespace {

// A get.  ids_on_device / on_device: where the ids and where the four public outputs are.  slot_dev (device, or null) and
// publish == false are the internal form: the slot of every request, and the handle's fetch stats left as they are.
vi_status fetch_by_id(const DeviceIndex &ix, const uint64_t *ids, uint64_t n, bool ids_on_device, bool on_device, uint32_t *count,
                      float *values, uint64_t *timestamps, uint64_t *where, uint32_t *slot_dev, bool publish) {
  if (!ix.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no external ids");
  VI_HIP(hipSetDevice(ix.device));
  vi_fetch_stats s{};
  bool done = false;  // the call succeeded: its stats become the handle's
  ContextLease lease(ix.fetch.pool, make_context<FetchContext>, [&] { if (done && publish) ix.fetch.last = s; });
  if (!lease.ctx) return VI_ERR_DEVICE;  // (the message is make_context's)
  FetchContext &c = *lease.ctx;
  hipStream_t st = c.stream;
  const bool timing = ix.timing != 0;
  const uint32_t dim = ix.dim;
  const uint64_t capacity = id_table_capacity(n);
  VI_TRY(c.first_slot.reserve(capacity + 1));
  VI_TRY(c.count.reserve(capacity + 1));
  Staged out{on_device};
  VI_TRY(out.stage(count, c.out_count, n));
  VI_TRY(out.stage(values, c.out_values, n * dim));
  VI_TRY(out.stage(timestamps, c.out_ts, n));
  VI_TRY(out.stage(where, c.out_where, n));
  // ---- the table of the requested ids (two more flag words: `found`), timed from behind the upload of host ids ----
  IdTable t;
  VI_TRY(id_set_build(c.ids, ids, n, ids_on_device, 2, st, &t, timing ? c.ev[0] : nullptr));
  if (!ids_on_device) ids = c.ids.upload.p;
  VI_HIP(hipMemsetAsync(c.first_slot.p, 0xff, (capacity + 1) * sizeof(uint32_t), st));  // kNoSlot
  VI_HIP(hipMemsetAsync(c.count.p, 0, (capacity + 1) * sizeof(uint32_t), st));
  if (timing) VI_HIP(hipEventRecord(c.ev[1], st));
  // ---- the scan of the resident ids ----
  if (ix.lists.nblocks && ix.nlists) {
    MatchArgs m{{ix.list_first_block.p, ix.list_len.p, (uint32_t)ix.nlists}, ix.ext_ids.p, t, c.first_slot.p, c.count.p};
    hipLaunchKernelGGL(fetch_match_kernel, slot_walk_grid((uint32_t)ix.nlists), dim3(256), 0, st, m);
    VI_HIP(hipGetLastError());
  }
  if (timing) VI_HIP(hipEventRecord(c.ev[2], st));
  // ---- the answers ----
  ResolveArgs r{};
  r.t = t; r.first_slot = c.first_slot.p; r.count = c.count.p; r.ids = ids; r.n = n;
  r.blocks = reinterpret_cast<const float4 *>(ix.lists.blocks.p); r.dq = ix.dq; r.dim = dim;
  r.first_block = ix.list_first_block.p; r.nlists = (uint32_t)ix.nlists; r.timestamps = ix.timestamps.p;
  r.world = ix.stripe_world; r.rank = ix.stripe_rank;
  r.out_count = count; r.out_values = values; r.out_ts = timestamps; r.out_where = where; r.out_slot = slot_dev;
  r.found = reinterpret_cast<unsigned long long *>(c.ids.flags.p + 2);
  r.vec_store = dim % 4 == 0 && aligned16(values);
  if (values) {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 3) / 4, kResolveBlocks);
    hipLaunchKernelGGL(fetch_resolve_gather_kernel<true>, dim3(grid), dim3(256), 0, st, r);
  } else {
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, kResolveBlocks);
    hipLaunchKernelGGL(fetch_resolve_gather_kernel<false>, dim3(grid), dim3(256), 0, st, r);
  }
  VI_HIP(hipGetLastError());
  if (timing) VI_HIP(hipEventRecord(c.ev[3], st));
  uint32_t fl[4] = {0, 0, 0, 0};
  VI_HIP(hipMemcpyAsync(fl, c.ids.flags.p, sizeof(fl), hipMemcpyDeviceToHost, st));
  VI_TRY(out.copy_back(st));
  if (timing) VI_HIP(hipEventRecord(c.ev[4], st));
  VI_HIP(hipStreamSynchronize(st));
  VI_TRY(id_set_check(fl, t, n, "get"));
  s.n = n;
  s.n_found = (uint64_t)fl[2] | ((uint64_t)fl[3] << 32);
  s.slots_scanned = ix.nvec_resident;
  s.bytes_moved = 16 * n + 8 * ix.nvec_resident + (count ? 4 * n : 0) + (timestamps ? 8 * n + 8 * s.n_found : 0) +
                  (where ? 8 * n : 0) + (values ? 4ull * dim * (n + s.n_found) : 0);
  if (timing) {
    s.ms_table = elapsed_ms(c.ev[0], c.ev[1]);
    s.ms_match = elapsed_ms(c.ev[1], c.ev[2]);
    s.ms_gather = elapsed_ms(c.ev[2], c.ev[3]);
    s.ms_total = elapsed_ms(c.ev[0], c.ev[4]);
  }
  done = true;
  return VI_OK;
}

// An export; slot_dev and publish as in fetch_by_id.
vi_status export_range(const DeviceIndex &ix, uint64_t first, uint64_t count, bool on_device, uint64_t *ext_ids, float *values,
                       uint64_t *timestamps, uint64_t *where, uint32_t *slot_dev, bool publish) {
  if (!ix.ext_ids.p) return fail(VI_ERR_INVALID_INPUT, "this index keeps no external ids");
  VI_HIP(hipSetDevice(ix.device));
  vi_fetch_stats s{};
  bool done = false;  // the call succeeded: its stats become the handle's
  ContextLease lease(ix.fetch.pool, make_context<FetchContext>, [&] { if (done && publish) ix.fetch.last = s; });
  if (!lease.ctx) return VI_ERR_DEVICE;  // (the message is make_context's)
  FetchContext &c = *lease.ctx;
  hipStream_t st = c.stream;
  const bool timing = ix.timing != 0;
  const uint32_t dim = ix.dim;
  VI_TRY(ensure_fetch_layout(ix, st));
  const FetchState &f = ix.fetch;  // (the layout is immutable once ready)
  // the blocks of the first and the last record of the range: every block between them belongs to a list with records
  auto block_of = [&](uint64_t ord) {
    const uint64_t l = (uint64_t)(std::upper_bound(f.h_prefix.begin(), f.h_prefix.end(), ord) - f.h_prefix.begin()) - 1;
    return (uint64_t)f.h_first[l] + (ord - f.h_prefix[l]) / 64;
  };
  const uint64_t block_lo = block_of(first), block_hi = block_of(first + count - 1);
  if (block_hi < block_lo || block_hi >= ix.lists.nblocks) return fail(VI_ERR_OTHER, "export: the list layout is inconsistent");
  const uint64_t nblk = block_hi - block_lo + 1;
  Staged out{on_device};
  VI_TRY(out.stage(ext_ids, c.out_ids, count));
  VI_TRY(out.stage(values, c.out_values, count * dim));
  VI_TRY(out.stage(timestamps, c.out_ts, count));
  VI_TRY(out.stage(where, c.out_where, count));
  ExportArgs a{};
  a.blocks = reinterpret_cast<const float4 *>(ix.lists.blocks.p); a.dq = ix.dq; a.dim = dim;
  a.first_block = ix.list_first_block.p; a.list_len = ix.list_len.p; a.prefix = f.prefix.p; a.nlists = (uint32_t)ix.nlists;
  a.ext_ids = ix.ext_ids.p; a.timestamps = ix.timestamps.p;
  a.block_lo = (uint32_t)block_lo; a.first = first; a.count = count;
  a.world = ix.stripe_world; a.rank = ix.stripe_rank;
  a.out_ids = ext_ids; a.out_values = values; a.out_ts = timestamps; a.out_where = where; a.out_slot = slot_dev;
  if (timing) VI_HIP(hipEventRecord(c.ev[0], st));
  if (dim % 4 == 0 && aligned16(values))
    hipLaunchKernelGGL(export_blocks_kernel<true>, dim3((uint32_t)nblk), dim3(64), 0, st, a);
  else
    hipLaunchKernelGGL(export_blocks_kernel<false>, dim3((uint32_t)nblk), dim3(64), 0, st, a);
  VI_HIP(hipGetLastError());
  if (timing) VI_HIP(hipEventRecord(c.ev[3], st));
  VI_TRY(out.copy_back(st));
  if (timing) VI_HIP(hipEventRecord(c.ev[4], st));
  VI_HIP(hipStreamSynchronize(st));
  s.n = s.n_found = count;
  s.slots_scanned = nblk * 64;
  s.bytes_moved = (ext_ids ? 16 * count : 0) + (timestamps ? 16 * count : 0) + (where ? 8 * count : 0) +
                  (values ? nblk * 64 * 16ull * ((dim + 3) / 4) + 4ull * dim * count : 0);
  if (timing) {
    s.ms_gather = elapsed_ms(c.ev[0], c.ev[3]);
    s.ms_total = elapsed_ms(c.ev[0], c.ev[4]);
  }
  done = true;
  return VI_OK;
}

}  // namespace

vi_status fetch_records_by_id(const DeviceIndex &ix, const uint64_t *ids, uint64_t n, bool on_device, uint32_t *count,
                              float *values, uint64_t *timestamps, uint64_t *where) {
  return fetch_by_id(ix, ids, n, on_device, on_device, count, values, timestamps, where, nullptr, true);
}

vi_status export_records(const DeviceIndex &ix, uint64_t first, uint64_t count, bool on_device, uint64_t *ext_ids,
                         float *values, uint64_t *timestamps, uint64_t *where) {
  return export_range(ix, first, count, on_device, ext_ids, values, timestamps, where, nullptr, true);
}

vi_status resolve_records_by_id(const DeviceIndex &ix, const uint64_t *ids, uint64_t n, bool ids_on_device, uint32_t *count_dev,
                                float *values_dev, uint32_t *slot_dev) {
  return fetch_by_id(ix, ids, n, ids_on_device, true, count_dev, values_dev, nullptr, nullptr, slot_dev, false);
}

vi_status resolve_records_by_range(const DeviceIndex &ix, uint64_t first, uint64_t count, float *values_dev, uint32_t *slot_dev) {
  return export_range(ix, first, count, true, nullptr, values_dev, nullptr, nullptr, slot_dev, false);
}

}  // namespace vi
