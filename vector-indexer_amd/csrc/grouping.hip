// grouping.hip — the probe grouping: counting sort of a batch's (query, probe) pairs by list, so that every list block is
// streamed once per group of queries that probe it; the scans over the lists built from it; the MFMA engine's rank work
// items (the item kernels, or the scatter that pushes them itself).  Interface and routes: grouping.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "device_index.hpp"
#include "grouping.hpp"
#include "scan.hpp"
#include "search_internal.hpp"
#include "wave_select.hpp"
#include "wave_sort.hpp"

namespace vi {
namespace {

// ------------------------------------------------------------------------------------------
// grouping (counting sort of (query, probe) pairs by list)
// ------------------------------------------------------------------------------------------
// single block (cnt = the per-list totals of list_totals_kernel): exclusive scans over the lists of
//   seg_start    Σ cnt                      (pairs grouped by list)
//   item_start   Σ ceil(cnt/QG) * nseg      (scan work items)
//   segrun_start Σ cnt * nseg [nseg > 1]    (segment runs awaiting seg_merge_kernel)
// and the grouping's counts of ws.stats (StatWord, search_internal.hpp): Σ cnt*len, items, segment runs, ...
// queries probing every list: the sum of its sub-bin counters.  A workgroup takes 64 lists, a lane per list (coalesced
// along each sub-bin row), each of its four waves a quarter of the sub-bins; the quarters meet in LDS.  (One thread
// walking all 32 counters of its list left 16 workgroups on the GPU at 4096 lists, each behind 32 loads of its own.)
// (also resets the counters group_prepare_kernel adds to — the grouping's counts — when `stats` is given: two memset
// launches less on a path made of 5-microsecond kernels)
// `prefix` (optional): where each sub-bin's pairs start within the pairs of their list, in the layout of the counters —
// every count is in hand here, and the scatter that builds the work items (item_push_kernel) adds seg_start itself,
// so no cursor_kernel reads the 32 counters of every list a second time
constexpr uint32_t kTotalsLists = 64, kTotalsWaves = 4, kTotalsBins = kSubBins / kTotalsWaves;  // per workgroup / per wave
static_assert(kTotalsBins * kTotalsWaves == kSubBins, "the waves of list_totals_kernel share the sub-bins evenly");

// what a list probed by c queries adds to the grouping: pairs, work items, segment runs, record tiles — and (v4, optional)
// to the counts vectors scanned, group records, tile blocks, tile blocks of a grouping by 128 queries
struct ListGroupCounts { uint32_t seg, item, run, tile; };
__device__ __forceinline__ ListGroupCounts list_group_counts(uint32_t c, uint32_t len, uint32_t qg, uint32_t segb0, unsigned long long *v4) {
  uint32_t segb;
  const uint32_t ns = list_segments(len, segb0, &segb);
  const uint32_t chunks = group_chunks(c, qg);
  if (v4) {
    v4[0] += (unsigned long long)c * len;
    v4[1] += 2ull * c * ns;
    v4[2] += (unsigned long long)chunks * ((len + 63) / 64);
    v4[3] += (unsigned long long)((c + 127) / 128) * ((len + 63) / 64);
  }
  return ListGroupCounts{c, chunks * ns, ns > 1 ? c * ns : 0u, chunks * ns * seg_records(segb)};
}

// The grouping's scans inside list_totals_kernel (GroupScanArgs::local set) instead of a launch of two single workgroups
// behind it (group_prepare_kernel).  A list workgroup has the totals of its 64 lists in hand: wave 0 derives every
// list's counts from them, scans them across its lanes and leaves per list (pairs, items / segment runs / record tiles of
// the workgroup's lists before it), per workgroup the four sums, and adds its share of the grouping's counts to the
// statistics.  What is then missing for an absolute offset — the sums of the workgroups before — is at most
// kGroupScanBlocks values per quantity, which every workgroup of item_push_kernel scans for itself.  A few more
// workgroups, behind the list workgroups, scan the queries' record totals into their offsets (scan_query_offsets).
struct GroupScanArgs {
  const uint32_t *list_len;
  uint32_t qg, segb0;
  uint4 *local;          // [nlists] pairs of the list; items, segment runs, record tiles before it within its 64 lists
  uint4 *block_sums;     // [workgroups] pairs, items, segment runs, record tiles of the 64 lists
  const uint32_t *qtot;  // the queries' record totals -> qoff[0..nq], qoff[nq] = their sum (both 16-byte aligned)
  uint32_t *qoff;
  uint32_t nq, q_tiles;  // ... by workgroups of q_tiles tiles each (qoff_tiles_per_block)
};

// qtot -> qoff by a few workgroups of 256 threads behind the list workgroups, each on its own run of whole tiles of 1024
// words, [begin, end): a lane on four consecutive words of a tile (16-byte loads and stores, a wave on 1 KB).  What a
// workgroup needs from the ones before it is one number, the sum of qtot[0, begin): it adds those words up itself — plain
// coalesced loads in flight together with its own tiles' — so that no workgroup waits for another and the longest
// dependent chain is one round: a DPP scan per tile and wave, the (tile, wave) sums through LDS, one barrier pair.
// (At most kQoffBlocks workgroups, so that the words read twice stay below kQoffBlocks / 2 x nq.)
constexpr uint32_t kQoffTiles = 4, kQoffBlocks = 16, kQoffTile = 4u * kTotalsLists * kTotalsWaves;  // tiles per round; words per tile
static_assert((kQoffTiles + 1) * kTotalsWaves <= kTotalsWaves * kTotalsLists, "the (tile, wave) sums fit the kernel's LDS words");
inline uint32_t qoff_tiles_per_block(uint32_t nq) { return ((nq + kQoffTile - 1) / kQoffTile + kQoffBlocks - 1) / kQoffBlocks; }
__device__ __forceinline__ void scan_query_offsets(const uint32_t *qtot, uint32_t nq, uint32_t *qoff, uint32_t begin, uint32_t end,
                                                   uint32_t *s_sum) {
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  uint4 v[kQoffTiles];
  auto load_round = [&](uint32_t r0) {
#pragma unroll
    for (uint32_t k = 0; k < kQoffTiles; ++k) {
      const uint32_t i = r0 + k * kQoffTile + 4u * t;
      v[k] = make_uint4(0u, 0u, 0u, 0u);
      if (i + 4u <= end) v[k] = *reinterpret_cast<const uint4 *>(qtot + i);
    }
#pragma unroll
    for (uint32_t k = 0; k < kQoffTiles; ++k) {  // (the last words of all: never a load past qtot[nq - 1])
      const uint32_t i = r0 + k * kQoffTile + 4u * t;
      if (i < end && i + 4u > end) {
        v[k].x = qtot[i];
        if (i + 1u < end) v[k].y = qtot[i + 1u];
        if (i + 2u < end) v[k].z = qtot[i + 2u];
      }
    }
  };
  load_round(begin);
  uint32_t head = 0;  // this lane's share of the words in front of the workgroup's (begin is a multiple of the tile)
#pragma unroll 8
  for (uint32_t i = 4u * t; i < begin; i += kQoffTile) {
    const uint4 x = *reinterpret_cast<const uint4 *>(qtot + i);
    head += x.x + x.y + x.z + x.w;
  }
  head = wave_incl_scan_u32(head);
  if (lane == 63u) s_sum[kQoffTiles * kTotalsWaves + wave] = head;
  uint32_t carry = 0;  // the sum of everything in front of the round
  for (uint32_t r0 = begin; r0 < end; r0 += kQoffTiles * kQoffTile) {
    if (r0 != begin) load_round(r0);
    uint32_t before[kQoffTiles];  // the words of the tile in front of this lane's four, within its wave
#pragma unroll
    for (uint32_t k = 0; k < kQoffTiles; ++k) {
      const uint32_t s = v[k].x + v[k].y + v[k].z + v[k].w, inc = wave_incl_scan_u32(s);
      before[k] = inc - s;
      if (lane == 63u) s_sum[k * kTotalsWaves + wave] = inc;
    }
    __syncthreads();
    if (r0 == begin) {
#pragma unroll
      for (uint32_t w = 0; w < kTotalsWaves; ++w) carry += s_sum[kQoffTiles * kTotalsWaves + w];
    }
    uint32_t run = carry;
#pragma unroll
    for (uint32_t k = 0; k < kQoffTiles; ++k) {
#pragma unroll
      for (uint32_t w = 0; w < kTotalsWaves; ++w) {
        if (w == wave) before[k] += run;
        run += s_sum[k * kTotalsWaves + w];
      }
    }
    carry = run;
#pragma unroll
    for (uint32_t k = 0; k < kQoffTiles; ++k) {
      const uint32_t i = r0 + k * kQoffTile + 4u * t;
      const uint4 o = make_uint4(before[k], before[k] + v[k].x, before[k] + v[k].x + v[k].y, before[k] + v[k].x + v[k].y + v[k].z);
      if (i + 4u <= end) *reinterpret_cast<uint4 *>(qoff + i) = o;
      else if (i < end) {
        qoff[i] = o.x;
        if (i + 1u < end) qoff[i + 1u] = o.y;
        if (i + 2u < end) qoff[i + 2u] = o.z;
      }
    }
    __syncthreads();  // (the next round writes the sums again)
  }
  if (end == nq && t == 0) qoff[nq] = carry;  // (the last workgroup)
}

// (SCANS: with GroupScanArgs — an instantiation of its own, so that the query scan's registers, a round of tiles, do not
// lower the occupancy of the plain form on tables of thousands of workgroups)
template <bool SCANS>
__global__ void __launch_bounds__(kTotalsLists * kTotalsWaves) list_totals_kernel(const uint32_t *cnt, uint32_t nlists, uint32_t *tot,
                                                                                  uint64_t *stats, uint32_t *prefix, GroupScanArgs g) {
  __shared__ uint32_t s_part[kTotalsWaves][kTotalsLists];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (SCANS && blockIdx.x * kTotalsLists >= nlists) {  // ---- the workgroups behind the lists: the queries' record offsets ----
    const uint32_t span = g.q_tiles * kQoffTile, begin = (blockIdx.x - (nlists + kTotalsLists - 1) / kTotalsLists) * span;
    scan_query_offsets(g.qtot, g.nq, g.qoff, begin, min(g.nq, begin + span), &s_part[0][0]);
    return;
  }
  const uint32_t l = blockIdx.x * kTotalsLists + lane;
  // (with the scans in this launch every workgroup ADDS to the counts: they were cleared ahead of it, by split_queries_kernel)
  if (stats && !SCANS && blockIdx.x == 0 && threadIdx.x < kStatListCounts + 1) stats[threadIdx.x < kStatListCounts ? threadIdx.x : kStatTiles128] = 0;
  const uint32_t len = (SCANS && wave == 0 && l < nlists) ? g.list_len[l] : 0u;  // (asked for with the counters)
  const uint32_t st = subbin_stride(nlists);
  uint32_t c[kTotalsBins], sum = 0;
#pragma unroll
  for (uint32_t u = 0; u < kTotalsBins; ++u) {
    c[u] = l < nlists ? cnt[(wave * kTotalsBins + u) * st + l] : 0u;
    sum += c[u];
  }
  s_part[wave][lane] = sum;
  __syncthreads();
  uint32_t run = 0, total = 0;  // the list's pairs in the sub-bins of the waves before this one, in all (0 past the last list)
#pragma unroll
  for (uint32_t w = 0; w < kTotalsWaves; ++w) {
    const uint32_t v = s_part[w][lane];
    if (w < wave) run += v;
    total += v;
  }
  if (SCANS && wave == 0) {  // (wave-uniform: all 64 lanes scan, lists past the last as zeros)
    unsigned long long v4[4] = {0, 0, 0, 0};  // vec, rec, mtile, mtile128
    const ListGroupCounts p = list_group_counts(total, len, g.qg, g.segb0, v4);
    const uint32_t is = wave_incl_scan_u32(p.seg), ii = wave_incl_scan_u32(p.item);
    const uint32_t ir = wave_incl_scan_u32(p.run), it = wave_incl_scan_u32(p.tile);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      v4[0] += __shfl_xor(v4[0], o); v4[1] += __shfl_xor(v4[1], o); v4[2] += __shfl_xor(v4[2], o); v4[3] += __shfl_xor(v4[3], o);
    }
    if (l < nlists) g.local[l] = make_uint4(p.seg, ii - p.item, ir - p.run, it - p.tile);
    if (lane == 63u) g.block_sums[blockIdx.x] = make_uint4(is, ii, ir, it);  // (the inclusive scans end here: the workgroup's sums)
    // the workgroup's share of the seven counts, a lane per count: one atomic instruction (a workgroup without a probed
    // list adds nothing)
    const uint32_t sums[3] = {readlane_u(ii, 63), readlane_u(it, 63), readlane_u(ir, 63)};
    constexpr uint32_t kWord[7] = {kStatScannedVectors, kStatGroupRecords, kStatTileBlocks, kStatTiles128, kStatItems, kStatRecordTiles, kStatSegRuns};
    unsigned long long add = 0;
    uint32_t word = 0;
#pragma unroll
    for (uint32_t i = 0; i < 7; ++i)
      if (lane == i) { add = i < 4 ? v4[i] : (unsigned long long)sums[i - 4]; word = kWord[i]; }
    if (lane < 7u && add) atomicAdd((unsigned long long *)&stats[word], add);
  }
  if (l >= nlists) return;
  if (wave == 0) tot[l] = total;
  if (!prefix) return;
#pragma unroll
  for (uint32_t u = 0; u < kTotalsBins; ++u) {
    prefix[(wave * kTotalsBins + u) * st + l] = run;
    run += c[u];
  }
}

// where each sub-bin of a list scatters to: its own slice of the list's segment of `pairs`
__global__ void cursor_kernel(const uint32_t *cnt, const uint32_t *seg_start, uint32_t nlists, uint32_t *cursor) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= nlists) return;
  const uint32_t st = subbin_stride(nlists);
  uint32_t run = seg_start[l];
#pragma unroll
  for (uint32_t s = 0; s < kSubBins; ++s) {
    cursor[s * st + l] = run;
    run += cnt[s * st + l];
  }
}

// the scan over the lists of group_prepare_kernel (one workgroup of 1024 threads)
__device__ __forceinline__ void group_scan_lists(const uint32_t *cnt, const uint32_t *list_len, uint32_t nlists, uint32_t qg,
                                                 uint32_t segb0, uint32_t *seg_start, uint32_t *item_start, uint32_t *segrun_start,
                                                 uint64_t *stats, uint32_t *tile_start, uint32_t *s_seg, uint32_t *s_item,
                                                 uint32_t *s_run, uint32_t *s_tile) {
  const uint32_t t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  // ---- lists (cnt = the per-list totals of list_totals_kernel, which also reset the counters added to below) ----
  // Wave w owns the contiguous lists [w R 64, (w + 1) R 64) as R rows of 64, a lane per list: every load and store is one
  // coalesced instruction, eight rows' loads in flight together.  (A thread walking its own 64 lists — 65 536 lists — read
  // and wrote with a stride of 256 bytes between lanes, 64 cache lines per instruction, all from the one CU this scan runs
  // on: 0.34 ms of a 4.9 ms search.)  Pass 1: the wave's totals; pass 2, behind the workgroup's prefix over the waves: a
  // DPP scan per row and quantity, the carry from row to row.
  const uint32_t rows = ((nlists + 63u) / 64u + 15u) / 16u;  // rows of 64 lists per wave
  const uint32_t l_base = (uint32_t)wave * rows * 64u;
  using PerList = ListGroupCounts;
  auto per_list = [&](uint32_t c, uint32_t len, unsigned long long *v4) { return list_group_counts(c, len, qg, segb0, v4); };
  uint32_t seg = 0, item = 0, run = 0, tile = 0;  // this lane's column sums over the wave's rows
  unsigned long long v4[4] = {0, 0, 0, 0};        // vec, rec, mtile, mtile128
  for (uint32_t r0 = 0; r0 < rows; r0 += 8) {
    uint32_t cs[8], lens[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
      const uint32_t l = l_base + (r0 + u) * 64u + (uint32_t)lane;
      const bool in = r0 + u < rows && l < nlists;
      cs[u] = in ? cnt[l] : 0u;
      lens[u] = in ? list_len[l] : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
      const PerList p = per_list(cs[u], lens[u], v4);  // (rows past the end: zeros)
      seg += p.seg; item += p.item; run += p.run; tile += p.tile;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    seg += (uint32_t)__shfl_xor((int)seg, o); item += (uint32_t)__shfl_xor((int)item, o);
    run += (uint32_t)__shfl_xor((int)run, o); tile += (uint32_t)__shfl_xor((int)tile, o);
    v4[0] += __shfl_xor(v4[0], o); v4[1] += __shfl_xor(v4[1], o); v4[2] += __shfl_xor(v4[2], o); v4[3] += __shfl_xor(v4[3], o);
  }
  if (lane == 0) {
    s_seg[wave] = seg; s_item[wave] = item; s_run[wave] = run; s_tile[wave] = tile;
    atomicAdd((unsigned long long *)&stats[kStatScannedVectors], v4[0]);
    atomicAdd((unsigned long long *)&stats[kStatGroupRecords], v4[1]);
    atomicAdd((unsigned long long *)&stats[kStatTileBlocks], v4[2]);
    atomicAdd((unsigned long long *)&stats[kStatTiles128], v4[3]);
  }
  __syncthreads();
  uint32_t rs = 0, ri = 0, rr = 0, rt = 0, tseg = 0, titem = 0, trun = 0, ttile = 0;
  for (int w = 0; w < 16; ++w) {
    if (w < wave) { rs += s_seg[w]; ri += s_item[w]; rr += s_run[w]; rt += s_tile[w]; }
    tseg += s_seg[w]; titem += s_item[w]; trun += s_run[w]; ttile += s_tile[w];
  }
  for (uint32_t r0 = 0; r0 < rows; r0 += 8) {  // (the same values again, from L2 now)
    uint32_t cs[8], lens[8];
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
      const uint32_t l = l_base + (r0 + u) * 64u + (uint32_t)lane;
      const bool in = r0 + u < rows && l < nlists;
      cs[u] = in ? cnt[l] : 0u;
      lens[u] = in ? list_len[l] : 0u;
    }
#pragma unroll
    for (uint32_t u = 0; u < 8; ++u) {
      if (r0 + u >= rows) break;  // (wave-uniform)
      const uint32_t l = l_base + (r0 + u) * 64u + (uint32_t)lane;
      const PerList p = per_list(cs[u], lens[u], nullptr);
      const uint32_t is = wave_incl_scan_u32(p.seg), ii = wave_incl_scan_u32(p.item);
      const uint32_t ir = wave_incl_scan_u32(p.run), it = wave_incl_scan_u32(p.tile);
      if (l < nlists) {
        seg_start[l] = rs + is - p.seg; item_start[l] = ri + ii - p.item; segrun_start[l] = rr + ir - p.run;
        if (tile_start) tile_start[l] = rt + it - p.tile;
      }
      rs += readlane_u(is, 63); ri += readlane_u(ii, 63); rr += readlane_u(ir, 63); rt += readlane_u(it, 63);
    }
  }
  if (t == 0) {
    seg_start[nlists] = tseg;
    item_start[nlists] = titem;
    segrun_start[nlists] = trun;
    stats[kStatItems] = titem;
    stats[kStatSegRuns] = trun;
    stats[kStatRecordTiles] = ttile;
  }
}

// the scan over the lists (workgroup 0) and, where query totals are given, the queries' record offsets (workgroup 1:
// exclusive scan of qtot, qoff[nq] = total) in one launch: both are single-workgroup scans, independent of each other.
// Without query totals workgroup 0 is launched alone.  (Folding list_totals and cursor in as well — one workgroup reading
// all 32 sub-bins of every list twice — was measured: the grouping took twice as long.)
__global__ void __launch_bounds__(1024) group_prepare_kernel(const uint32_t *cnt, const uint32_t *list_len, uint32_t nlists, uint32_t qg,
                                                             uint32_t segb0, uint32_t *seg_start, uint32_t *item_start,
                                                             uint32_t *segrun_start, uint64_t *stats, uint32_t *tile_start,
                                                             const uint32_t *qtot, uint32_t nq, uint32_t *qoff) {
  __shared__ uint32_t s_seg[16], s_item[16], s_run[16], s_tile[16];
  const uint32_t t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  if (blockIdx.x == 1) {  // ---- query offsets ----
    if (!qtot) return;
    const uint32_t per = (nq + 1023) / 1024;
    const uint32_t beg = min(nq, t * per), end = min(nq, beg + per);
    uint32_t sum = 0;
    for (uint32_t i = beg; i < end; ++i) sum += qtot[i];
    uint32_t inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t x = (uint32_t)__shfl_up((int)inc, o);
      if (lane >= o) inc += x;
    }
    if (lane == 63) s_seg[wave] = inc;
    __syncthreads();
    uint32_t w = 0, tot = 0;
    for (int i = 0; i < 16; ++i) {
      if (i < wave) w += s_seg[i];
      tot += s_seg[i];
    }
    uint32_t run = w + inc - sum;
    for (uint32_t i = beg; i < end; ++i) { qoff[i] = run; run += qtot[i]; }
    if (t == 0) qoff[nq] = tot;
    return;
  }
  group_scan_lists(cnt, list_len, nlists, qg, segb0, seg_start, item_start, segrun_start, stats, tile_start, s_seg, s_item, s_run, s_tile);
}

// (list ids are range-checked wherever they index: a caller-supplied probe list, vi_indexer_search_probed_device, is
// validated up front by validate_probes_kernel, and a stray word can then still not fault the GPU)
__global__ void histogram_kernel(const uint32_t *probes, const uint32_t *list_len, uint32_t nlists, uint32_t n, uint32_t P,
                                 uint32_t *cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t l = probes[i];
  if (l < nlists && list_len[l] > 0) atomicAdd(&cnt[subbin_index(l, div_probes(i, P) & (kSubBins - 1), nlists)], 1u);
}

__global__ void group_scatter_kernel(const uint32_t *probes, const uint32_t *list_len, uint32_t nlists, uint32_t P,
                                     uint32_t *cursor, uint32_t *pairs, uint32_t total, const uint32_t *seg_start,
                                     uint32_t *pair_pos) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t l = probes[i];
  if (l >= nlists || list_len[l] == 0) return;
  const uint32_t pos = atomicAdd(&cursor[subbin_index(l, div_probes(i, P) & (kSubBins - 1), nlists)], 1u);
  pairs[pos] = i;  // slot id = q*P + rank
  if (pair_pos) pair_pos[i] = pos - seg_start[l];  // MFMA path: where the pair sits among the pairs of its list
}

// the same without atomics: the pair's place among the pairs of its (list, sub-bin) came back from the histogram
// increment of the kernel that chose the probe (coarse_select_direct_kernel) — 320 000 returning atomics on counters
// shared across the XCDs were most of the scatter's 17 us
__global__ void group_scatter_ranked_kernel(const uint32_t *probes, const uint32_t *list_len, uint32_t nlists, uint32_t P,
                                            const uint32_t *cursor, const uint32_t *pair_rank, uint32_t *pairs, uint32_t total,
                                            const uint32_t *seg_start, uint32_t *pair_pos) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t l = probes[i];
  if (l >= nlists || list_len[l] == 0) return;
  const uint32_t pos = cursor[subbin_index(l, div_probes(i, P) & (kSubBins - 1), nlists)] + pair_rank[i];
  pairs[pos] = i;
  if (pair_pos) pair_pos[i] = pos - seg_start[l];
}

// ---- the MFMA engine's rank work items ----
// list of every work item: keeps a 12-step dependent binary search out of each rank workgroup's prologue
__global__ void item_list_kernel(const uint32_t *item_start, uint32_t nlists, uint32_t nitems, uint32_t *item_list) {
  const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
  if (item >= nitems) return;
  uint32_t lo = 0, hi = nlists;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (item_start[mid] <= item) lo = mid; else hi = mid;
  }
  item_list[item] = lo;
}

// everything a list-rank work item needs to know about itself, 32 bytes it reads with two wave-uniform loads instead
// of a chain of five dependent ones (list -> offsets -> length -> ...) at the head of every workgroup:
// {first pair, queries, first block of the list, b0, b1, segment, first record tile, -}
// Workgroup -> item: the hardware deals workgroups to the 8 XCDs round-robin (workgroup w runs on XCD w % 8), and each
// XCD has its own L2.  The query groups of one list segment stream the SAME blocks, so they are numbered next to each
// other (segment-major) and dealt in runs of `run` items to one XCD: workgroup w = (cycle, r, x) -> item
// cycle * 8 run + x * run + r.  They start together, the followers hit the L2 lines the first one brought in, and a
// hit is faster than a miss, which keeps them together.  (run <= 1: workgroup w takes item w.)
__global__ void item_desc_kernel(const uint32_t *item_start, const uint32_t *seg_start, const uint32_t *list_len,
                                 const uint32_t *first_block, const uint32_t *tile_start, uint32_t nlists, uint32_t nitems,
                                 uint32_t segb0, uint32_t gq, uint32_t run, uint4 *items) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= nitems) return;
  uint32_t item = w;
  if (run > 1u) {
    const uint32_t span = 8u * run, cycle = w / span;
    if ((cycle + 1u) * span <= nitems) {  // (the last, partial cycle keeps its order)
      const uint32_t in = w - cycle * span;
      item = cycle * span + (in & 7u) * run + (in >> 3);
    }
  }
  uint32_t lo = 0, hi = nlists;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (item_start[mid] <= item) lo = mid; else hi = mid;
  }
  const uint32_t l = lo;
  const uint32_t s0 = seg_start[l], cnt = seg_start[l + 1] - s0, len = list_len[l];
  uint32_t segb;
  const uint32_t nseg = list_segments(len, segb0, &segb);
  const uint32_t local = item - item_start[l];
  const uint32_t nchunk = (cnt + gq - 1u) / gq;  // query groups of the list: its items are nchunk * nseg
  const uint32_t seg = local / nchunk, chunk = local - seg * nchunk;
  const uint32_t j0 = chunk * gq;
  const uint32_t nblk = (len + 63u) / 64u, b0 = seg * segb, b1 = min(nblk, b0 + segb);
  items[2 * (size_t)w] = make_uint4(s0 + j0, min(gq, cnt - j0), first_block[l], b0);
  items[2 * (size_t)w + 1] = make_uint4(b1, seg, tile_start[l] + (chunk * nseg + seg) * seg_records(segb), 0u);
}

// Per (work item, column of its query group): the query, and where its group record goes — so that the rank
// workgroup finds everything about an item at addresses it can compute from the item's index alone (no chain
// descriptor -> pairs -> query offsets at the head of every item) — and the place word of the pair's two group records
// (probe rank | segment << 6 | lane half << 13; every (pair, segment) sits in exactly one item).  One workgroup per
// item; workgroup 0 also resets the rank kernel's work counter and the "a query has a lo plane" and "a query is no int8
// image" flags of the next batch.
__global__ void item_cols_kernel(const uint4 *items, const uint32_t *pairs, const uint32_t *qoff, const uint32_t *rel, uint32_t P,
                                 uint32_t gq, uint32_t *qcol, uint32_t *grec, uint4 *sdesc, uint32_t *gmeta, uint64_t *stats) {
  const uint32_t w = blockIdx.x;
  const uint4 d0 = items[2 * (size_t)w], d1 = items[2 * (size_t)w + 1];
  if (threadIdx.x == 0) {
    sdesc[w] = make_uint4(d0.y, d0.z + d0.w, 2u * (d1.x - d0.w), d1.z);  // queries, first block, tiles, first record tile
    if (w == 0) { stats[kStatQueryLo] = 0; stats[kStatQueryNotI8] = 0; }
  }
  if (w == 0 && threadIdx.x < kStatRankWorkCount) stats[kStatRankWork + kStatRankWorkStride * threadIdx.x] = 0;  // the rank kernel's work counters (one per XCD queue, 128 bytes apart)
  for (uint32_t col = threadIdx.x; col < gq; col += blockDim.x) {
    uint32_t q = ~0u, g = ~0u;
    if (col < d0.y) {
      const uint32_t slot = pairs[d0.x + col];
      q = div_probes(slot, P);
      g = qoff[q] + rel[slot] + 2u * d1.y;
      const uint32_t place = (slot - q * P) | (d1.y << 6);
      *reinterpret_cast<uint2 *>(gmeta + g) = make_uint2(place, place | (1u << 13));  // (g is even: 8-byte aligned)
    }
    qcol[(size_t)w * gq + col] = q;
    grec[(size_t)w * gq + col] = g;
  }
}

// The scatter and both kernels above in one launch, for the streaming rank kernel (VI_ITEM_PUSH=0: the chain above).
// Every (query, probe) pair knows its list, and with the list its work items: the thread that places the pair among the
// pairs of its list writes the pair's column of every item it sits in itself, instead of leaving `pairs` behind for
// item_desc_kernel (a 12-step binary search per item for the list) and item_cols_kernel (items -> pairs -> qoff / rel,
// three dependent loads) to find it again.  What a list owns rather than a pair — the items' descriptors, and the dead
// columns behind the last query group of every segment, which the rank kernel reads as ~0 — is written by a wave per
// probed list: the workgroups behind the pairs' (a giant list's dead columns are no work for one pair's thread).
// subprefix: a sub-bin's start within the pairs of its list (list_totals_kernel).  The item and record buffers are sized
// by counts the host reads back while this kernel runs: it is given their capacities as they are and leaves everything
// but the resets alone when the batch needs more (group_pairs grows them and launches it again).
struct ItemPushArgs {
  const uint32_t *probes, *pair_rank, *subprefix, *list_len, *first_block, *seg_start, *item_start, *tile_start, *qoff, *rel;
  uint32_t total, P, nlists, gq, segb0, run;
  uint32_t pair_groups;      // workgroups [0, pair_groups): a thread per pair; behind them: a wave per list
  uint64_t cap_items, cap_records;  // work items the column / descriptor buffers hold, group records gmeta holds
  // the lists' offsets as list_totals_kernel leaves them when it scans itself (GroupScanArgs), or null (seg_start,
  // item_start, tile_start as group_prepare_kernel wrote them): per list, relative to its 64 lists, and the sums of
  // every 64 lists — scanned here by every workgroup.  tile_out: each list's absolute first record tile, for the selects
  const uint4 *local, *block_sums;
  uint32_t *tile_out;
  uint32_t *pair_pos, *qcol, *grec, *gmeta;
  uint4 *sdesc;
  uint64_t *stats;
};

// workgroup of the rank kernel that takes `item`: the inverse of item_desc_kernel's dealing in runs to the XCDs
__device__ __forceinline__ uint32_t item_workgroup(uint32_t item, uint32_t run, uint32_t nitems) {
  if (run <= 1u) return item;
  const uint32_t span = 8u * run, pow2 = (run & (run - 1u)) == 0u, sh = (uint32_t)__builtin_ctz(run);
  const uint32_t cycle = pow2 ? item >> (sh + 3u) : item / span;
  if ((cycle + 1u) * span > nitems) return item;  // (the last, partial cycle keeps its order)
  const uint32_t in = item - cycle * span, x = pow2 ? in >> sh : in / run;
  return cycle * span + (in - x * run) * 8u + x;
}

__global__ void __launch_bounds__(256) item_push_kernel(ItemPushArgs a) {
  __shared__ uint2 s_base[kGroupScanBlocks];  // items, record tiles of the 64-list workgroups before each (a.local only)
  __shared__ uint2 s_wave[4];
  // the rank kernel's work counters and the batch flags of the next batch (their D2H copy is ahead of this kernel)
  if (blockIdx.x == 0) {
    if (threadIdx.x < kStatRankWorkCount) a.stats[kStatRankWork + kStatRankWorkStride * threadIdx.x] = 0;
    if (threadIdx.x == 0) { a.stats[kStatQueryLo] = 0; a.stats[kStatQueryNotI8] = 0; }
  }
  // (the pair's own words are asked for ahead of the counts the test below waits for)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool pair = blockIdx.x < a.pair_groups && i < a.total;
  const uint32_t l_pair = pair ? a.probes[i] : kNoPos, rank = pair ? a.pair_rank[i] : 0u, rel = pair ? a.rel[i] : 0u;
  uint4 sums = make_uint4(0u, 0u, 0u, 0u);
  if (a.local && threadIdx.x < (a.nlists + 63u) / 64u) sums = a.block_sums[threadIdx.x];
  const uint64_t nitems64 = a.stats[kStatItems];
  if (nitems64 > a.cap_items || a.stats[kStatGroupRecords] > a.cap_records) return;  // (every thread of the grid alike)
  const uint32_t nitems = (uint32_t)nitems64, gq = a.gq;
  if (a.local) {  // the exclusive scan of the 64-list sums, a thread per sum
    const uint32_t wv = threadIdx.x >> 6, ii = wave_incl_scan_u32(sums.y), it = wave_incl_scan_u32(sums.w);
    if ((threadIdx.x & 63u) == 63u) s_wave[wv] = make_uint2(ii, it);
    __syncthreads();
    uint2 base = make_uint2(ii - sums.y, it - sums.w);
#pragma unroll
    for (uint32_t w = 0; w < 3; ++w)
      if (w < wv) { base.x += s_wave[w].x; base.y += s_wave[w].y; }
    s_base[threadIdx.x] = base;
    __syncthreads();
  }
  if (blockIdx.x < a.pair_groups) {  // ---- a thread per pair: its place, and its column in the items of its list ----
    const uint32_t l = l_pair;
    if (l >= a.nlists) return;
    const uint32_t len = a.list_len[l];
    if (len == 0) return;
    const uint32_t q = div_probes(i, a.P);
    uint32_t cnt, it0;
    if (a.local) {
      const uint4 lc = a.local[l];
      cnt = lc.x; it0 = s_base[l >> 6].x + lc.y;
    } else {
      const uint32_t s0 = a.seg_start[l];
      cnt = a.seg_start[l + 1] - s0; it0 = a.item_start[l];
    }
    const uint32_t pp = a.subprefix[subbin_index(l, q & (kSubBins - 1), a.nlists)] + rank;
    if (pp >= cnt) return;  // (never: the ranks are the histogram's own increments)
    a.pair_pos[i] = pp;
    uint32_t segb;
    const uint32_t nseg = list_segments(len, a.segb0, &segb);
    // (chunk = pp / gq, by group_chunks' shift for the group widths in use)
    const uint32_t nchunk = group_chunks(cnt, gq), chunk = group_chunks(pp + 1u, gq) - 1u, col = pp - chunk * gq;
    const uint32_t g0 = a.qoff[q] + rel, r = i - q * a.P;
    uint32_t item = it0 + chunk;  // segment-major: segment s, chunk c = item_start + s * nchunk + c
    for (uint32_t s = 0; s < nseg; ++s, item += nchunk) {
      const size_t o = (size_t)item_workgroup(item, a.run, nitems) * gq + col;
      const uint32_t g = g0 + 2u * s, place = r | (s << 6);
      a.qcol[o] = q;
      a.grec[o] = g;
      *reinterpret_cast<uint2 *>(a.gmeta + g) = make_uint2(place, place | (1u << 13));  // (g is even: 8-byte aligned)
    }
    return;
  }
  // ---- a wave per probed list: its items' descriptors, the dead columns of every segment's last query group ----
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t l = (blockIdx.x - a.pair_groups) * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (l >= a.nlists) return;
  uint32_t cnt, it0, t0;
  if (a.local) {
    const uint4 lc = a.local[l];
    const uint2 base = s_base[l >> 6];
    cnt = lc.x; it0 = base.x + lc.y; t0 = base.y + lc.w;
    if (lane == 0) a.tile_out[l] = t0;  // (every list, as group_prepare_kernel: the selects read it for every probe)
    if (cnt == 0) return;
  } else {
    const uint32_t s0 = a.seg_start[l];
    cnt = a.seg_start[l + 1] - s0;
    if (cnt == 0) return;
    it0 = a.item_start[l]; t0 = a.tile_start[l];
  }
  const uint32_t len = a.list_len[l], fb = a.first_block[l];
  uint32_t segb;
  const uint32_t nseg = list_segments(len, a.segb0, &segb);
  const uint32_t nchunk = group_chunks(cnt, gq), nblk = (len + 63u) / 64u, srec = seg_records(segb);
  for (uint32_t k = lane; k < nchunk * nseg; k += 64u) {
    const uint32_t seg = k / nchunk, chunk = k - seg * nchunk;
    const uint32_t b0 = seg * segb, b1 = min(nblk, b0 + segb);
    // queries, first block, tiles, first record tile
    a.sdesc[item_workgroup(it0 + k, a.run, nitems)] =
        make_uint4(min(gq, cnt - chunk * gq), fb + b0, 2u * (b1 - b0), t0 + (chunk * nseg + seg) * srec);
  }
  const uint32_t last = nchunk - 1u, live = cnt - last * gq;
  if (live == gq) return;
  for (uint32_t seg = 0; seg < nseg; ++seg) {
    const size_t o = (size_t)item_workgroup(it0 + seg * nchunk + last, a.run, nitems) * gq;
    for (uint32_t col = live + lane; col < gq; col += 64u) { a.qcol[o + col] = ~0u; a.grec[o + col] = ~0u; }
  }
}

bool pushes_items(GroupingRoute route) { return route == GroupingRoute::PreparePush || route == GroupingRoute::ScansPush; }

// histogram (ws.cnt) -> totals -> offsets of the lists in pairs / items / records -> what the route's scatter starts
// from: absolute cursors, or each sub-bin's start within its list (left by list_totals_kernel — one launch less)
vi_status launch_group_scans(const DeviceIndex &ix, SearchWorkspace &ws, const GroupingRequest &rq, GroupingRoute route, hipStream_t st) {
  const uint32_t nlists = (uint32_t)ix.nlists, nq = (uint32_t)rq.nq;
  const bool push = pushes_items(route);
  VI_TRY(ws.list_tot.reserve(std::max<uint32_t>(1, nlists)));
  uint32_t *cursor = ws.cnt.p + subbin_words(nlists);
  const uint32_t list_blocks = (nlists + kTotalsLists - 1) / kTotalsLists;
  if (route == GroupingRoute::ScansPush) {  // (grouping_route: at most kGroupScanBlocks workgroups of lists, the counts cleared, qtot given)
    VI_TRY(ws.list_local.reserve(4ull * std::max<uint32_t>(1, nlists)));
    VI_TRY(ws.list_block_sums.reserve(4ull * kGroupScanBlocks));
    const uint32_t q_tiles = std::max(1u, qoff_tiles_per_block(nq)), q_blocks = std::max(1u, (nq + q_tiles * kQoffTile - 1) / (q_tiles * kQoffTile));
    const GroupScanArgs g{ix.list_len.p, rq.qg, rq.segb0, (uint4 *)ws.list_local.p, (uint4 *)ws.list_block_sums.p, rq.qtot, rq.qoff, nq, q_tiles};
    hipLaunchKernelGGL(list_totals_kernel<true>, dim3(list_blocks + q_blocks), dim3(kTotalsLists * kTotalsWaves), 0, st, ws.cnt.p, nlists, ws.list_tot.p,
                       ws.stats.p, cursor, g);
    VI_HIP(hipGetLastError());
    return VI_OK;
  }
  hipLaunchKernelGGL(list_totals_kernel<false>, dim3(list_blocks), dim3(kTotalsLists * kTotalsWaves), 0, st, ws.cnt.p, nlists, ws.list_tot.p, ws.stats.p,
                     push ? cursor : nullptr, GroupScanArgs{});
  // (with query totals: + their offsets, by a second workgroup of the same launch)
  hipLaunchKernelGGL(group_prepare_kernel, dim3(rq.qtot ? 2 : 1), dim3(1024), 0, st, ws.list_tot.p, ix.list_len.p, nlists, rq.qg, rq.segb0,
                     ws.seg_start.p, ws.item_start.p, ws.segrun_start.p, ws.stats.p, (rq.tile_start || push) ? ws.tile_start.p : nullptr,
                     rq.qtot, nq, rq.qoff);
  if (!push) hipLaunchKernelGGL(cursor_kernel, dim3((nlists + 255) / 256), dim3(256), 0, st, ws.cnt.p, ws.seg_start.p, nlists, cursor);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

// the grouping's scatter for the streaming rank kernel (item_push_kernel), with the item and record buffers as they stand
vi_status launch_item_push(const DeviceIndex &ix, SearchWorkspace &ws, const GroupingRequest &rq, GroupingRoute route, hipStream_t st) {
  const uint32_t nlists = (uint32_t)ix.nlists, total = (uint32_t)(rq.nq * rq.P);
  VI_TRY(ws.item_qcol.reserve(1));  // (no null pointers; a first batch finds no room and is pushed again)
  VI_TRY(ws.item_grec.reserve(1));
  VI_TRY(ws.item_sdesc.reserve(4));
  VI_TRY(ws.gpos.reserve(1));
  ItemPushArgs a{};
  a.probes = rq.probes; a.pair_rank = rq.pair_rank; a.subprefix = ws.cnt.p + subbin_words(nlists);
  a.list_len = ix.list_len.p; a.first_block = ix.list_first_block.p; a.seg_start = ws.seg_start.p; a.item_start = ws.item_start.p;
  a.tile_start = ws.tile_start.p; a.qoff = rq.qoff; a.rel = ws.pair_rel.p;
  if (route == GroupingRoute::ScansPush) {  // (the lists' offsets come in two parts, list_totals_kernel's)
    a.local = (const uint4 *)ws.list_local.p; a.block_sums = (const uint4 *)ws.list_block_sums.p; a.tile_out = ws.tile_start.p;
    a.seg_start = a.item_start = a.tile_start = nullptr;  // (not written by this search)
  }
  a.total = total; a.P = rq.P; a.nlists = nlists; a.gq = rq.qg; a.segb0 = rq.segb0; a.run = rq.push_run;
  a.pair_groups = (total + 255u) / 256u;
  a.cap_items = std::min<uint64_t>(std::min(ws.item_qcol.n, ws.item_grec.n) / rq.qg, ws.item_sdesc.n / 4);
  a.cap_records = ws.gpos.n;
  a.pair_pos = ws.pair_pos.p; a.qcol = ws.item_qcol.p; a.grec = ws.item_grec.p; a.gmeta = ws.gpos.p;
  a.sdesc = (uint4 *)ws.item_sdesc.p; a.stats = ws.stats.p;
  hipLaunchKernelGGL(item_push_kernel, dim3(std::max(1u, a.pair_groups + (nlists + 3u) / 4u)), dim3(256), 0, st, a);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

}  // namespace

// (push: the caller has what item_push_kernel needs — the pairs' ranks, the histogram they are the increments of, the
//  record offsets.  Scans in the totals: where item_push_kernel, which completes the lists' offsets, follows, the counts
//  were cleared ahead, and the query scan's 16-byte loads and stores are aligned)
GroupingRoute grouping_route(const GroupingRequest &rq, uint64_t nlists) {
  const bool ranked = rq.pair_rank && rq.histogram_done;
  if (!(ranked && rq.push_run != 0 && rq.qtot)) return ranked ? GroupingRoute::RankedScatter : GroupingRoute::AtomicScatter;
  const bool in_totals = rq.counts_cleared && group_scan_in_totals_applicable(nlists) && (((uintptr_t)rq.qtot | (uintptr_t)rq.qoff) & 15u) == 0;
  return in_totals ? GroupingRoute::ScansPush : GroupingRoute::PreparePush;
}

vi_status launch_probe_histogram(const DeviceIndex &ix, SearchWorkspace &ws, const uint32_t *probes, uint32_t total, uint32_t P, hipStream_t st) {
  const uint64_t nlists = ix.nlists;
  VI_TRY(ws.cnt.reserve(2 * subbin_words(nlists)));
  VI_HIP(hipMemsetAsync(ws.cnt.p, 0, subbin_words(nlists) * sizeof(uint32_t), st));
  hipLaunchKernelGGL(histogram_kernel, dim3((total + 255) / 256), dim3(256), 0, st, probes, ix.list_len.p, (uint32_t)nlists, total, P, ws.cnt.p);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

vi_status group_probes(const DeviceIndex &ix, SearchContext &ctx, const GroupingRequest &rq, GroupingCounts &counts) {
  SearchWorkspace &ws = ctx.ws;
  hipStream_t st = ctx.stream;
  const uint64_t nlists = ix.nlists;
  const uint32_t total = (uint32_t)(rq.nq * rq.P);
  const GroupingRoute route = grouping_route(rq, nlists);
  const bool pair_pos = rq.pair_pos || pushes_items(route), tile_start = rq.tile_start || pushes_items(route);
  VI_TRY(ws.cnt.reserve(2 * subbin_words(nlists)));
  VI_TRY(ws.seg_start.reserve(nlists + 1));
  VI_TRY(ws.item_start.reserve(nlists + 1));
  VI_TRY(ws.segrun_start.reserve(nlists + 1));
  VI_TRY(ws.pairs.reserve(total));
  if (pair_pos) VI_TRY(ws.pair_pos.reserve(total));
  if (tile_start) VI_TRY(ws.tile_start.reserve(nlists + 1));
  VI_TRY(ws.stats.reserve(kStatWords));
  // (the layout of ws.stats: StatWord, search_internal.hpp — the grouping's counts are reset by list_totals_kernel)
  if (!rq.histogram_done) VI_TRY(launch_probe_histogram(ix, ws, rq.probes, total, rq.P, st));
  VI_TRY(launch_group_scans(ix, ws, rq, route, st));
  // the host waits for the counts (grid size, scratch) while the scatter runs
  // (into page-locked memory: a copy to the caller's stack array is staged by the runtime and costs a few microseconds
  // more on the one synchronisation point of the pipeline)
  if (!ws.hstats_pinned) VI_HIP(hipHostMalloc((void **)&ws.hstats_pinned, kStatGroupingLanding * sizeof(uint64_t)));
  VI_HIP(hipMemcpyAsync(ws.hstats_pinned, ws.stats.p, sizeof(GroupingCounts), hipMemcpyDeviceToHost, st));
  VI_HIP(hipEventRecord(ctx.ev[5], st));
  const dim3 grid((total + 255) / 256), block(256);
  uint32_t *cursor = ws.cnt.p + subbin_words(nlists), *pos_out = pair_pos ? ws.pair_pos.p : nullptr;
  switch (route) {
    case GroupingRoute::AtomicScatter:
      hipLaunchKernelGGL(group_scatter_kernel, grid, block, 0, st, rq.probes, ix.list_len.p, (uint32_t)nlists, rq.P, cursor, ws.pairs.p, total,
                         ws.seg_start.p, pos_out);
      break;
    case GroupingRoute::RankedScatter:
      hipLaunchKernelGGL(group_scatter_ranked_kernel, grid, block, 0, st, rq.probes, ix.list_len.p, (uint32_t)nlists, rq.P, cursor, rq.pair_rank,
                         ws.pairs.p, total, ws.seg_start.p, pos_out);
      break;
    case GroupingRoute::PreparePush:
    case GroupingRoute::ScansPush:
      VI_TRY(launch_item_push(ix, ws, rq, route, st));
      break;
  }
  VI_HIP(hipGetLastError());
  VI_HIP(hipEventSynchronize(ctx.ev[5]));
  std::memcpy(counts.data(), ws.hstats_pinned, sizeof(GroupingCounts));
  return VI_OK;
}

vi_status repush_items(const DeviceIndex &ix, SearchWorkspace &ws, const GroupingRequest &rq, hipStream_t st) {
  return launch_item_push(ix, ws, rq, grouping_route(rq, ix.nlists), st);
}

vi_status launch_item_list(const DeviceIndex &ix, SearchWorkspace &ws, uint32_t nitems, hipStream_t st) {
  VI_TRY(ws.item_list.reserve(std::max<uint32_t>(1, nitems)));
  if (!nitems) return VI_OK;
  hipLaunchKernelGGL(item_list_kernel, dim3((nitems + 255) / 256), dim3(256), 0, st, ws.item_start.p, (uint32_t)ix.nlists, nitems, ws.item_list.p);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

vi_status launch_item_desc(const DeviceIndex &ix, SearchWorkspace &ws, const EngineKnobs &kn, uint32_t gq, uint32_t nitems, hipStream_t st) {
  VI_TRY(ws.items.reserve(std::max<uint32_t>(1, nitems) * 8ull));
  if (!nitems) return VI_OK;
  hipLaunchKernelGGL(item_desc_kernel, dim3((nitems + 255) / 256), dim3(256), 0, st, ws.item_start.p, ws.seg_start.p, ix.list_len.p,
                     ix.list_first_block.p, ws.tile_start.p, (uint32_t)ix.nlists, nitems, kn.segb0, gq, kn.item_run, (uint4 *)ws.items.p);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

vi_status launch_item_cols(SearchWorkspace &ws, uint32_t P, uint32_t gq, uint32_t nitems, hipStream_t st) {
  VI_TRY(ws.item_qcol.reserve(std::max<uint64_t>(1, (uint64_t)nitems * gq)));
  VI_TRY(ws.item_grec.reserve(std::max<uint64_t>(1, (uint64_t)nitems * gq)));
  VI_TRY(ws.item_sdesc.reserve(std::max<uint64_t>(1, (uint64_t)nitems * 4)));
  if (!nitems) return VI_OK;
  hipLaunchKernelGGL(item_cols_kernel, dim3(nitems), dim3(128), 0, st, (const uint4 *)ws.items.p, ws.pairs.p, ws.qoff.p, ws.pair_rel.p, P, gq,
                     ws.item_qcol.p, ws.item_grec.p, (uint4 *)ws.item_sdesc.p, ws.gpos.p, ws.stats.p);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

}  // namespace vi
