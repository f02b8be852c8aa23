// search_kernels.hip — the exact-order VALU engine: its gfx950 kernels and the pipeline that runs a SearchBatch through them
// (the dispatcher is search.hip), and the two small utilities built on its kernels (merge_partials*, l2sq_pairs_device).
//
// Reference path being replaced: IvfIndex::search_with_paths (src/ivf_index.rs:190-267):
//   coarse  : euclidean_distance_squared(q, c_i) for all centroids, stable sort, take n_probe
//   scan    : euclidean_distance_squared(q, v) for every vector of the probed lists
//   select  : stable sort of all candidates, take k
// with euclidean_distance_squared = strictly sequential f32 sum of (x-y)^2 (src/utils.rs:28-30).
//
// GPU formulation (all distances are computed in the reference's exact summation order, so
// ids AND distances are bit-identical; nothing is re-ranked):
//   scan_kernel<COARSE>   one wave = (group of QG queries) x (range of centroid blocks);
//                         lane = centroid, per-lane sequential f32 chain over d; wave-resident
//                         sorted top-P list per query (DPP shift insertion)
//   coarse_merge_kernel   one wave per query: S sorted partial runs -> probe list, shard
//                         visiting order, histogram of probed lists
//   grouping (grouping.hip)  counting sort of (query,probe) pairs by list  => every list block is
//                         streamed once per group of QG queries that probe it
//   scan_kernel<LISTS>    one wave = (list) x (group of <= QG queries probing it)
//   final_merge_kernel    one wave per query: P sorted runs -> top-k, ids, tie keys
//
// Compiled with -ffp-contract=off: a fused multiply-add would change the rounding of
// acc + t*t and break bit parity with the reference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "device_index.hpp"
#include "device_math.hpp"
#include "grouping.hpp"
#include "scan.hpp"
#include "search_internal.hpp"
#include "slot_filter.hpp"
#include "wave_select.hpp"
#include "wave_sort.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;
constexpr int kWavesPerBlock = 4;
constexpr int kBlockThreads = kWave * kWavesPerBlock;

// ------------------------------------------------------------------------------------------
// Exact-order accumulators.  SCALAR: src/utils.rs:28-30.  LANES: src/kmeans.rs:377-419
// (8-lane chunks, then one 4-lane chunk, then a scalar tail; reduce order see oracle header).
// ------------------------------------------------------------------------------------------
// Accumulator state of QG (query, vector) pairs per lane.  add<T>() consumes quad T (0..3) of the
// current group of 4 quads; `qi` is the absolute quad index (wave-uniform).
template <int ORDER, int QG>
struct Acc;

template <int QG>
struct Acc<VI_ORDER_SCALAR, QG> {
  float a[QG];
  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int j = 0; j < QG; ++j) a[j] = 0.0f;
  }
  template <int T>
  __device__ __forceinline__ void add(int j, uint32_t, uint32_t, bool, const float4 &q, const float4 &x) {
    sq_add(a[j], q.x, x.x);
    sq_add(a[j], q.y, x.y);
    sq_add(a[j], q.z, x.z);
    sq_add(a[j], q.w, x.w);
  }
  __device__ __forceinline__ float finish(int j) const { return a[j]; }
};

template <int QG>
struct Acc<VI_ORDER_LANES, QG> {
  float a8[QG][8], a4[QG][4], tail[QG];
  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int j = 0; j < QG; ++j) {
#pragma unroll
      for (int l = 0; l < 8; ++l) a8[j][l] = 0.0f;
      a4[j][0] = a4[j][1] = a4[j][2] = a4[j][3] = 0.0f;
      tail[j] = 0.0f;
    }
  }
  // n8x2 = 2*(dim/8): quads below it feed the 8 lane accumulators (kmeans.rs:387-396); the next
  // quad is the f32x4 chunk if at least 4 dims remain (:399-408); what is left is the scalar
  // tail (:411-416).  Zero padding contributes exact +0 wherever it lands.
  template <int T>
  __device__ __forceinline__ void add(int j, uint32_t qi, uint32_t n8x2, bool has4, const float4 &q,
                                      const float4 &x) {
    if (qi < n8x2) {
      constexpr int h = (T & 1) * 4;
      sq_add(a8[j][h + 0], q.x, x.x); sq_add(a8[j][h + 1], q.y, x.y);
      sq_add(a8[j][h + 2], q.z, x.z); sq_add(a8[j][h + 3], q.w, x.w);
    } else if (qi == n8x2 && has4) {
      sq_add(a4[j][0], q.x, x.x); sq_add(a4[j][1], q.y, x.y);
      sq_add(a4[j][2], q.z, x.z); sq_add(a4[j][3], q.w, x.w);
    } else {
      sq_add(tail[j], q.x, x.x); sq_add(tail[j], q.y, x.y);
      sq_add(tail[j], q.z, x.z); sq_add(tail[j], q.w, x.w);
    }
  }
  __device__ __forceinline__ float finish(int j) const {
    const float lo = VI_REDUCE4(a8[j][0], a8[j][1], a8[j][2], a8[j][3]);  // include/vi_reduce_order.h
    const float hi = VI_REDUCE4(a8[j][4], a8[j][5], a8[j][6], a8[j][7]);
    const float r4 = VI_REDUCE4(a4[j][0], a4[j][1], a4[j][2], a4[j][3]);
    return ((lo + hi) + r4) + tail[j];
  }
};

// ------------------------------------------------------------------------------------------
// scan kernel
// ------------------------------------------------------------------------------------------
// FILT (lists only): a vector is a candidate only if its bit of the block's allow word is set (slot_filter.hpp) — an
// instantiation of its own, so that the unfiltered kernels keep their registers
template <int QG, int ORDER, bool COARSE, bool DUMP, bool FILT = false>
__global__ void __launch_bounds__(kBlockThreads) scan_kernel(ScanArgs a) {
  extern __shared__ float4 smem[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  float4 *lq = smem + (size_t)wave * QG * a.dq;
  const uint32_t item = blockIdx.x * kWavesPerBlock + wave;

  uint32_t nqi, b0, b1, len, fb;
  uint32_t nseg = 1, seg = 0, segrun0 = 0;
  uint32_t slot[QG], qid[QG];
  if (COARSE) {
    const uint32_t nqg = (a.nq + QG - 1) / QG;
    if (item >= nqg * a.S) return;
    const uint32_t qc = item / a.S, sp = item - qc * a.S;
    const uint32_t q0 = qc * QG;
    nqi = min((uint32_t)QG, a.nq - q0);
#pragma unroll
    for (int j = 0; j < QG; ++j) { qid[j] = q0 + j; slot[j] = (q0 + j) * a.S + sp; }
    const uint32_t nblk = (a.nvec + kWave - 1) / kWave;
    b0 = sp * a.bps;
    b1 = min(nblk, b0 + a.bps);
    fb = 0;
    len = a.nvec;
  } else {
    const uint32_t nitems = a.item_start[a.nlists];
    if (item >= nitems) return;
    // largest l with item_start[l] <= item  (lists with no items have equal neighbours)
    uint32_t lo = 0, hi = a.nlists;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (a.item_start[mid] <= item) lo = mid; else hi = mid;
    }
    const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    const uint32_t s0 = a.seg_start[l], cnt = a.seg_start[l + 1] - s0;
    len = a.list_len[l];
    uint32_t segb;
    nseg = list_segments(len, a.segb0, &segb);
    const uint32_t local = item - a.item_start[l];
    const uint32_t chunk = local / nseg;
    seg = local - chunk * nseg;
    const uint32_t j0 = chunk * QG;
    nqi = min((uint32_t)QG, cnt - j0);
#pragma unroll
    for (int j = 0; j < QG; ++j) {
      const uint32_t s = (j < (int)nqi) ? a.pairs[s0 + j0 + j] : 0u;
      slot[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)s);
      qid[j] = slot[j] / a.P;
    }
    segrun0 = nseg > 1 ? a.segrun_start[l] + j0 * nseg + seg : 0u;
    fb = a.first_block[l];
    const uint32_t nblk = (len + kWave - 1) / kWave;
    b0 = seg * segb;
    b1 = min(nblk, b0 + segb);
    if (a.max_blocks) b1 = min(b1, a.max_blocks);
  }

  // stage the group's queries in this wave's LDS slice, zero padded to dq*4 floats
  {
    float *lqf = reinterpret_cast<float *>(lq);
    const uint32_t dpad = a.dq * 4;
#pragma unroll
    for (int j = 0; j < QG; ++j) {
      const float *src = a.Q + (size_t)qid[j] * a.dim;
      const bool live = j < (int)nqi;
      for (uint32_t e = lane; e < dpad; e += kWave) lqf[j * dpad + e] = (live && e < a.dim) ? src[e] : 0.0f;
    }
    wave_lds_sync();
  }

  WaveTopK sel[QG];
#pragma unroll
  for (int j = 0; j < QG; ++j) sel[j].init();
  const int K = (int)a.K;

  // Flat software-pipelined sweep over (block, group-of-4-quads): the next group's four
  // global_load_dwordx4 are issued before the current group is consumed, also across block
  // boundaries, so the selection step of a block overlaps the first loads of the next one.
  const uint32_t gpb = a.dq >> 2;  // dq is a multiple of 4 (layout pads dims to 16)
  const uint32_t total = (b1 - b0) * gpb;
  const uint32_t n8x2 = 2 * (a.dim / 8);
  const bool has4 = (a.dim - 4 * n8x2) >= 4;
  const float4 *vbase = a.blocks + ((size_t)(fb + b0) * a.dq) * kWave + lane;
  Acc<ORDER, QG> acc;
  acc.reset();
  float4 xn0, xn1, xn2, xn3;
  if (total) {
    xn0 = vbase[0]; xn1 = vbase[kWave]; xn2 = vbase[2 * kWave]; xn3 = vbase[3 * kWave];
  }
  uint32_t gq = 0, blk = b0;
  for (uint32_t g = 0; g < total; ++g) {
    const float4 x0 = xn0, x1 = xn1, x2 = xn2, x3 = xn3;
    if (g + 1 < total) {
      const float4 *nx = vbase + (size_t)(g + 1) * 4 * kWave;  // groups are contiguous in memory
      xn0 = nx[0]; xn1 = nx[kWave]; xn2 = nx[2 * kWave]; xn3 = nx[3 * kWave];
    }
    const uint32_t qi = gq * 4;
#pragma unroll
    for (int j = 0; j < QG; ++j) acc.template add<0>(j, qi + 0, n8x2, has4, lq[j * a.dq + qi + 0], x0);
#pragma unroll
    for (int j = 0; j < QG; ++j) acc.template add<1>(j, qi + 1, n8x2, has4, lq[j * a.dq + qi + 1], x1);
#pragma unroll
    for (int j = 0; j < QG; ++j) acc.template add<2>(j, qi + 2, n8x2, has4, lq[j * a.dq + qi + 2], x2);
#pragma unroll
    for (int j = 0; j < QG; ++j) acc.template add<3>(j, qi + 3, n8x2, has4, lq[j * a.dq + qi + 3], x3);
    if (++gq == gpb) {
      const uint32_t pos = blk * kWave + lane;
      bool valid = pos < len;
      if constexpr (FILT) valid = valid && ((a.allow[fb + blk] >> lane) & 1ull) != 0ull;  // (one word per block: a scalar load)
      const uint32_t p = valid ? pos : kNoPos;
#pragma unroll
      for (int j = 0; j < QG; ++j)
        if (j < (int)nqi) {
          const float dj = valid ? acc.finish(j) : INFINITY;
          if (DUMP) {  // generic path: every candidate is written out, nothing is selected
            if (valid) {
              const uint32_t idx = COARSE ? pos : a.dump_off[slot[j]] + pos;
              const uint64_t row = COARSE ? (uint64_t)qid[j] : (uint64_t)(slot[j] / a.P);
              a.dump_keys[row * a.dump_row + idx] = ((uint64_t)__float_as_uint(dj) << 32) | idx;
            }
          } else {
            sel[j].offer(dj, p, K);
          }
        }
      acc.reset();
      gq = 0;
      ++blk;
    }
  }

  if (!DUMP && lane < K) {
#pragma unroll
    for (int j = 0; j < QG; ++j)
      if (j < (int)nqi) {
        if (COARSE || nseg == 1) {
          a.run_dist[(size_t)slot[j] * K + lane] = sel[j].d;
          a.run_pos[(size_t)slot[j] * K + lane] = sel[j].p;
        } else {
          const size_t r = (size_t)(segrun0 + (uint32_t)j * nseg) * K + lane;
          a.seg_run_dist[r] = sel[j].d;
          a.seg_run_pos[r] = sel[j].p;
        }
      }
  }
}

// merge the segment runs of every (query, list) pair whose list was cut into segments
struct SegMergeArgs {
  const uint32_t *seg_start, *segrun_start, *list_len, *pairs;
  uint32_t nlists, segb0, K;
  const float *seg_run_dist;
  const uint32_t *seg_run_pos;
  float *run_dist;
  uint32_t *run_pos;
};

__global__ void __launch_bounds__(kBlockThreads) seg_merge_kernel(SegMergeArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t pi = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (pi >= a.seg_start[a.nlists]) return;
  uint32_t lo = 0, hi = a.nlists;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.seg_start[mid] <= pi) lo = mid; else hi = mid;
  }
  const uint32_t l = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
  uint32_t segb;
  const uint32_t nseg = list_segments(a.list_len[l], a.segb0, &segb);
  if (nseg <= 1) return;
  const uint32_t K = a.K;
  const size_t base = ((size_t)a.segrun_start[l] + (size_t)(pi - a.seg_start[l]) * nseg + lane) * K;
  uint32_t head = 0, hp = kNoPos;
  float hd = INFINITY;
  if ((uint32_t)lane < nseg) { hd = a.seg_run_dist[base]; hp = a.seg_run_pos[base]; }
  float od = INFINITY;
  uint32_t op = kNoPos;
  for (uint32_t i = 0; i < K; ++i) {
    // segments hold increasing positions, so (dist, segment) == (dist, position) order
    const uint64_t key = (hp == kNoPos) ? ~0ull : (((uint64_t)__float_as_uint(hd) << 32) | (uint32_t)lane);
    const uint64_t m = wave_min_u64(key);
    if (m == ~0ull) break;
    const int win = (int)(uint32_t)m;
    const uint32_t wp = readlane_u(hp, win);
    if ((uint32_t)lane == i) { od = __uint_as_float((uint32_t)(m >> 32)); op = wp; }
    if (lane == win) {
      ++head;
      if (head < K) { hd = a.seg_run_dist[base + head]; hp = a.seg_run_pos[base + head]; }
      else hp = kNoPos;
    }
  }
  if ((uint32_t)lane < K) {
    const size_t o = (size_t)a.pairs[pi] * K + lane;
    a.run_dist[o] = od;
    a.run_pos[o] = op;
  }
}

// ------------------------------------------------------------------------------------------
// coarse merge: S sorted runs per query -> probes (rank order), shard visiting order, histogram
// ------------------------------------------------------------------------------------------
struct CoarseMergeArgs {
  const float *run_dist;
  const uint32_t *run_pos;
  uint32_t nq, S, P;              // P = entries per run = probes per query (<= 64), S <= 64
  const uint32_t *list_shard, *list_len;
  uint32_t *probes, *gorder, *cnt;
  uint32_t nlists;
};

__global__ void __launch_bounds__(kBlockThreads) coarse_merge_kernel(CoarseMergeArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t q = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (q >= a.nq) return;
  const size_t base = ((size_t)q * a.S + lane) * a.P;
  uint32_t head = 0;
  float hd = INFINITY;
  uint32_t hp = kNoPos;
  if (lane < (int)a.S) { hd = a.run_dist[base]; hp = a.run_pos[base]; }
  uint32_t mylist = kNoPos;
  uint32_t found = 0;
  for (uint32_t i = 0; i < a.P; ++i) {
    // key = (dist, centroid index): stable sort over index order (ivf_index.rs:205-215)
    const uint64_t key = (hp == kNoPos) ? ~0ull : (((uint64_t)__float_as_uint(hd) << 32) | hp);
    const uint64_t m = wave_min_u64(key);
    if (m == ~0ull) break;
    if ((uint32_t)lane == i) mylist = (uint32_t)m;
    if (key == m) {
      ++head;
      if (head < a.P) { hd = a.run_dist[base + head]; hp = a.run_pos[base + head]; }
      else hp = kNoPos;
    }
    ++found;
  }
  const bool live = (uint32_t)lane < found;
  const uint32_t g = probe_candidate_order(lane, found, mylist, a.list_shard);
  if ((uint32_t)lane < a.P) {
    a.probes[(size_t)q * a.P + lane] = live ? mylist : kNoPos;
    a.gorder[(size_t)q * a.P + lane] = live ? g : kNoPos;
    if (live && a.list_len[mylist] > 0) atomicAdd(&a.cnt[subbin_index(mylist, q & (kSubBins - 1), a.nlists)], 1u);
  }
}

// caller-supplied probe lists (multi-GPU: another rank's coarse step), one wave per row: every probe must name a list of
// this index or be the empty marker, the real probes of a row must come first, and their candidate-order ranks must be
// distinct and below the row's number of real probes (a permutation of 0 .. found-1: the MFMA select inverts it with one
// ds_permute).  The ranks of the markers are not read.  A bitmap of the ranks seen in LDS, (P + 31) / 32 words.
__global__ void __launch_bounds__(64) validate_probes_kernel(const uint32_t *probes, const uint32_t *order, uint32_t P,
                                                             uint32_t nlists, uint32_t *bad) {
  extern __shared__ uint32_t seen[];
  const uint32_t q = blockIdx.x, lane = threadIdx.x, words = (P + 31u) / 32u;
  const uint32_t *row = probes + (size_t)q * P, *ord = order + (size_t)q * P;
  for (uint32_t w = lane; w < words; w += 64u) seen[w] = 0u;
  bool ok = true;
  uint32_t found = 0;
  for (uint32_t r0 = 0; r0 < P; r0 += 64u) {
    const uint32_t r = r0 + lane;
    const uint32_t l = r < P ? row[r] : kNoPos;
    const bool real = l != kNoPos;
    if (real && (l >= nlists || (r > 0 && row[r - 1] == kNoPos))) ok = false;
    found += (uint32_t)__popcll(__ballot(real));
  }
  __syncthreads();
  for (uint32_t r = lane; r < P; r += 64u) {
    if (row[r] == kNoPos) continue;
    const uint32_t g = ord[r];
    if (g >= found || (atomicOr(&seen[g >> 5], 1u << (g & 31u)) >> (g & 31u)) & 1u) ok = false;
  }
  if (!ok) atomicOr(bad, 1u);
}

// ------------------------------------------------------------------------------------------
// final merge: P sorted runs per query -> top-k in the reference's stable candidate order
// ------------------------------------------------------------------------------------------
struct FinalMergeArgs {
  const float *run_dist;
  const uint32_t *run_pos;
  uint32_t nq, P, K, k;           // K entries per run; k outputs per query
  const uint32_t *probes, *gorder, *first_block;
  const uint64_t *ext_ids;
  float *D;
  int64_t *I;
  uint64_t *tie;                  // optional
  uint64_t *slots;                // optional
  uint32_t *counts;               // optional
};

__global__ void __launch_bounds__(kBlockThreads) final_merge_kernel(FinalMergeArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t q = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (q >= a.nq) return;
  const size_t slot = (size_t)q * a.P + lane;
  const size_t base = slot * a.K;
  uint32_t head = 0, hp = kNoPos, g = kNoPos, list = kNoPos;
  float hd = INFINITY;
  if (lane < (int)a.P) {
    list = a.probes[slot];
    g = a.gorder[slot];
    if (list != kNoPos) { hd = a.run_dist[base]; hp = a.run_pos[base]; }
  }
  uint32_t found = 0;
  const uint32_t kk = a.k < a.P * a.K ? a.k : a.P * a.K;
  for (uint32_t i = 0; i < kk; ++i) {
    // (dist, shard-visit/probe order g, position): the stable sort of ivf_index.rs:265
    const uint64_t key = (hp == kNoPos) ? ~0ull : (((uint64_t)__float_as_uint(hd) << 32) | g);
    const uint64_t m = wave_min_u64(key);
    if (m == ~0ull) break;
    if (key == m) {
      const size_t o = (size_t)q * a.k + i;
      const uint64_t gslot = (uint64_t)a.first_block[list] * kWave + hp;
      a.D[o] = hd;
      a.I[o] = (int64_t)a.ext_ids[gslot];
      if (a.tie) a.tie[o] = ((uint64_t)g << 32) | hp;
      if (a.slots) a.slots[o] = gslot;
      ++head;
      if (head < a.K) { hd = a.run_dist[base + head]; hp = a.run_pos[base + head]; }
      else hp = kNoPos;
    }
    ++found;
  }
  for (uint32_t i = found + lane; i < a.k; i += kWave) {  // lib.rs:179-187 padding
    const size_t o = (size_t)q * a.k + i;
    a.D[o] = INFINITY;
    a.I[o] = -1;
    if (a.tie) a.tie[o] = ~0ull;
    if (a.slots) a.slots[o] = ~0ull;
  }
  if (a.counts && lane == 0) a.counts[q] = found;
}

// merge `parts` partial top-k lists per query (multi-GPU): key = (dist, tie)
// part p of Dp / Ip / Tp starts p * stride elements (of the respective type) after part 0
__global__ void __launch_bounds__(kBlockThreads) merge_partials_kernel(uint64_t nq, uint32_t k, uint32_t parts,
                                                                      const float *Dp0, const int64_t *Ip0,
                                                                      const uint64_t *Tp0, size_t strideD,
                                                                      size_t strideI, float *D, int64_t *I) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint64_t q = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (q >= nq) return;
  // lane = part (parts <= 64); each part's list is sorted by (dist, tie) already
  const float *Dp = Dp0 + (size_t)(lane < (int)parts ? lane : 0) * strideD;
  const int64_t *Ip = Ip0 + (size_t)(lane < (int)parts ? lane : 0) * strideI;
  const uint64_t *Tp = Tp0 + (size_t)(lane < (int)parts ? lane : 0) * strideI;
  const size_t base = (size_t)q * k;
  uint32_t head = 0;
  bool live = lane < (int)parts;
  float hd = INFINITY;
  uint64_t ht = ~0ull;
  int64_t hi = -1;
  // an empty slot is marked by its tie key (ids are arbitrary u64: one >= 2^63 reads as a negative i64)
  if (live) { hd = Dp[base]; ht = Tp[base]; hi = Ip[base]; live = ht != ~0ull; }
  uint32_t found = 0;
  for (uint32_t i = 0; i < k; ++i) {
    // two-level key: distance bits first, then the 64-bit tie key
    const uint64_t kd = live ? (uint64_t)__float_as_uint(hd) : ~0ull;
    const uint64_t md = wave_min_u64(kd);
    if (md == ~0ull) break;
    const uint64_t kt = (live && kd == md) ? ht : ~0ull;
    const uint64_t mt = wave_min_u64(kt);
    if (live && kd == md && kt == mt) {
      D[q * k + i] = hd;
      I[q * k + i] = hi;
      ++head;
      if (head < k) { hd = Dp[base + head]; ht = Tp[base + head]; hi = Ip[base + head]; live = ht != ~0ull; }
      else live = false;
    }
    ++found;
  }
  for (uint32_t i = found + lane; i < k; i += kWave) { D[q * k + i] = INFINITY; I[q * k + i] = -1; }
}

// plain pairwise distances in either order (vi_l2sq_pairs)
__global__ void l2sq_pairs_kernel(const float *a, const float *b, uint64_t n, uint32_t d, int order, float *out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float *p = a + i * d, *c = b + i * d;
  out[i] = order == VI_ORDER_SCALAR ? l2sq_scalar_dev(p, c, d) : l2sq_lanes_dev(p, c, d);
}

// ------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------
template <int QG, int ORDER, bool COARSE, bool DUMP, bool FILT = false>
vi_status launch_scan_t(const ScanArgs &a, uint32_t nitems_upper, hipStream_t st) {
  if (nitems_upper == 0) return VI_OK;
  const uint32_t grid = (nitems_upper + kWavesPerBlock - 1) / kWavesPerBlock;
  const size_t smem = (size_t)kWavesPerBlock * QG * a.dq * sizeof(float4);
  if (smem > 64 * 1024)
    VI_HIP(hipFuncSetAttribute((const void *)scan_kernel<QG, ORDER, COARSE, DUMP, FILT>,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  hipLaunchKernelGGL((scan_kernel<QG, ORDER, COARSE, DUMP, FILT>), dim3(grid), dim3(kBlockThreads), smem, st, a);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

// mode (table / lists), output (runs / one key per candidate) and, on lists, with or without allow bits
template <int QG, int ORDER>
vi_status launch_scan_q(const ScanArgs &a, bool coarse, uint32_t nitems_upper, hipStream_t st) {
  const bool dump = a.dump_keys != nullptr;
  if (coarse)
    return dump ? launch_scan_t<QG, ORDER, true, true>(a, nitems_upper, st) : launch_scan_t<QG, ORDER, true, false>(a, nitems_upper, st);
  if (a.allow)
    return dump ? launch_scan_t<QG, ORDER, false, true, true>(a, nitems_upper, st)
                : launch_scan_t<QG, ORDER, false, false, true>(a, nitems_upper, st);
  return dump ? launch_scan_t<QG, ORDER, false, true>(a, nitems_upper, st) : launch_scan_t<QG, ORDER, false, false>(a, nitems_upper, st);
}

}  // namespace

// Chosen so that QG*dq float4 per wave stays within the 160 KiB LDS of a CU at 4 waves/block.
int pick_qg(uint32_t dq, double avg_queries_per_unit, int order) {
  const int cap = order == VI_ORDER_LANES ? 4 : 8;
  // QG=8 halves the block re-reads but needs 154 VGPRs (3 waves/SIMD); QG=4 (102 VGPRs, 4 waves/SIMD)
  // measured 10 % faster on the C2 workload (profiles/r01_experiments.md)
  int qg = 1;
  if (avg_queries_per_unit >= 3.0) qg = 4;
  (void)cap;
  qg = std::min(qg, cap);
  while (qg > 1 && (size_t)kWavesPerBlock * qg * dq * sizeof(float4) > 96 * 1024) qg = (qg == 8) ? 4 : 1;
  return qg;
}

vi_status launch_scan(const ScanArgs &a, int qg, int order, bool coarse, uint32_t nitems_upper, hipStream_t st) {
#define VI_SCAN_CASE(QGV)                                                                                  \
  if (qg == QGV) {                                                                                         \
    constexpr int QL = QGV > 4 ? 4 : QGV; /* LANES order keeps 8 accumulators per pair: cap the group */   \
    if (order == VI_ORDER_SCALAR) return launch_scan_q<QGV, VI_ORDER_SCALAR>(a, coarse, nitems_upper, st); \
    return launch_scan_q<QL, VI_ORDER_LANES>(a, coarse, nitems_upper, st);                                 \
  }
  VI_SCAN_CASE(1)
  VI_SCAN_CASE(2)
  VI_SCAN_CASE(4)
  VI_SCAN_CASE(8)
#undef VI_SCAN_CASE
  return fail(VI_ERR_OTHER, "unsupported query group %d", qg);
}

uint32_t coarse_splits(uint64_t nq, int qg, uint32_t nblk, uint32_t *bps) {
  const uint32_t nqg = (uint32_t)((nq + qg - 1) / qg);
  uint32_t S = std::max<uint32_t>(1, std::min<uint32_t>({(uint32_t)kMaxSelect, nblk, (4096 + nqg - 1) / nqg}));
  *bps = (std::max<uint32_t>(nblk, 1) + S - 1) / S;
  return std::max<uint32_t>(1, (nblk + *bps - 1) / *bps);
}

// ------------------------------------------------------------------------------------------
// pipeline stages
// ------------------------------------------------------------------------------------------
// 1+2: coarse scan over the centroid table, merge -> ws.probes / ws.gorder, histogram in ws.cnt
vi_status stage_coarse(SearchBatch &b) {
  const DeviceIndex &ix = b.ix;
  SearchWorkspace &ws = b.ws();
  hipStream_t st = b.st();
  const uint32_t P = b.P, dim = ix.dim, dq = ix.dq;
  const uint64_t nq = b.nq, nlists = ix.nlists;
  VI_TRY(ws.cnt.reserve(2 * subbin_words(nlists)));
  VI_HIP(hipMemsetAsync(ws.cnt.p, 0, subbin_words(nlists) * sizeof(uint32_t), st));
  const uint32_t nblk_c = (uint32_t)ix.centroids.nblocks;
  const int qg_c = pick_qg(dq, (double)nq, ix.order);
  const uint32_t nqg = (uint32_t)((nq + qg_c - 1) / qg_c);
  uint32_t bps = 0;
  const uint32_t S = coarse_splits(nq, qg_c, nblk_c, &bps);
  VI_TRY(ws.crun_dist.reserve(nq * S * P));
  VI_TRY(ws.crun_pos.reserve(nq * S * P));
  {
    ScanArgs a{};
    a.blocks = (const float4 *)ix.centroids.blocks.p; a.dq = dq; a.dim = dim; a.Q = b.Qd; a.nq = (uint32_t)nq;
    a.K = P; a.run_dist = ws.crun_dist.p; a.run_pos = ws.crun_pos.p;
    a.nvec = (uint32_t)nlists; a.S = S; a.bps = bps;
    VI_TRY(launch_scan(a, qg_c, ix.order, true, nqg * S, st));
  }
  VI_TRY(ws.probes.reserve(nq * P));
  VI_TRY(ws.gorder.reserve(nq * P));
  CoarseMergeArgs a{ws.crun_dist.p, ws.crun_pos.p, (uint32_t)nq, S, P, ix.list_shard.p, ix.list_len.p,
                    ws.probes.p, ws.gorder.p, ws.cnt.p, (uint32_t)nlists};
  hipLaunchKernelGGL(coarse_merge_kernel, dim3((uint32_t)((nq + kWavesPerBlock - 1) / kWavesPerBlock)),
                     dim3(kBlockThreads), 0, st, a);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

// probes given by the caller (multi-GPU: coarse step done elsewhere): probe lists + candidate-order ranks into
// the workspace, and the per-list histogram the grouping scan starts from
vi_status adopt_probes(SearchBatch &b, bool histogram) {
  const DeviceIndex &ix = b.ix;
  SearchWorkspace &ws = b.ws();
  const uint64_t nq = b.nq;
  const uint32_t P = b.P, *probes_in = b.probes_in, *order_in = b.order_in;
  hipStream_t st = b.st();
  VI_TRY(ws.probes.reserve(nq * P));
  VI_TRY(ws.gorder.reserve(nq * P));
  VI_HIP(hipMemcpyAsync(ws.probes.p, probes_in, nq * P * 4, hipMemcpyDeviceToDevice, st));
  VI_HIP(hipMemcpyAsync(ws.gorder.p, order_in, nq * P * 4, hipMemcpyDeviceToDevice, st));
  VI_TRY(validate_probe_rows(ix, ws, probes_in, order_in, nq, P, st));
  if (histogram) VI_TRY(launch_probe_histogram(ix, ws, ws.probes.p, (uint32_t)(nq * P), P, st));
  return VI_OK;
}

vi_status validate_probe_rows(const DeviceIndex &ix, SearchWorkspace &ws, const uint32_t *probes, const uint32_t *order, uint64_t nq,
                              uint32_t P, hipStream_t st) {
  const uint64_t nlists = ix.nlists;
  VI_TRY(ws.probe_flag.reserve(1));
  VI_HIP(hipMemsetAsync(ws.probe_flag.p, 0, 4, st));
  hipLaunchKernelGGL(validate_probes_kernel, dim3((uint32_t)nq), dim3(64), ((P + 31u) / 32u) * 4u, st, probes, order, P,
                     (uint32_t)nlists, ws.probe_flag.p);
  VI_HIP(hipGetLastError());
  uint32_t bad = 0;
  VI_HIP(hipMemcpyAsync(&bad, ws.probe_flag.p, 4, hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  if (bad)
    return fail(VI_ERR_INVALID_INPUT, "probe lists out of range: every probe must be < %llu (or the empty marker 0xFFFFFFFF "
                "after the last real probe of a row), and the orders of a row's real probes must be distinct and below "
                "its number of real probes", (unsigned long long)nlists);
  return VI_OK;
}

// exact-order VALU pipeline: coarse -> group -> list scan -> final merge (k <= 64: the wave-resident top-k)
vi_status search_valu_pipeline(SearchBatch &b, uint64_t k, const SelectOutputs &out) {
  const DeviceIndex &ix = b.ix;
  const EngineKnobs &kn = b.kn;
  SearchContext &ctx = b.ctx;
  SearchWorkspace &ws = ctx.ws;
  vi_search_stats &stt = ctx.stats;
  hipStream_t st = ctx.stream;
  const uint64_t nq = b.nq, nlists = ix.nlists;
  const uint32_t P = b.P, K = (uint32_t)std::min<uint64_t>(k, kMaxSelect), dim = ix.dim, dq = ix.dq;
  const bool timing = b.timing == 1, rank_timing = b.timing != 0;
  VI_TRY(ws.run_dist.reserve(nq * P * K));
  VI_TRY(ws.run_pos.reserve(nq * P * K));
  // runs of lists that are not resident here (other rank / unreadable shard) stay empty
  VI_HIP(hipMemsetAsync(ws.run_pos.p, 0xFF, nq * P * K * sizeof(uint32_t), st));

  if (timing) VI_HIP(hipEventRecord(ctx.ev[0], st));
  if (b.probes_in) VI_TRY(adopt_probes(b, true));
  else VI_TRY(stage_coarse(b));
  VI_TRY(prune_staged_probes(b, true));
  if (timing) VI_HIP(hipEventRecord(ctx.ev[1], st));
  // ---- 3. group (query,probe) pairs by list ----
  const double avg_q_per_list = (double)nq * P / (double)std::max<uint64_t>(1, nlists);
  int qg_l = pick_qg(dq, avg_q_per_list, ix.order);
  {
    const uint32_t f = kn.force_qg;
    if (f == 1 || f == 2 || f == 4 || (f == 8 && ix.order == VI_ORDER_SCALAR)) qg_l = (int)f;
  }
  const uint32_t kSegBlocks = kn.seg_blocks;
  // exact work-item / segment-run counts size the scan grid and its scratch (record tiles, pair positions: the MFMA engine's)
  GroupingRequest rq;
  rq.probes = ws.probes.p; rq.nq = nq; rq.P = P; rq.qg = (uint32_t)qg_l; rq.segb0 = kSegBlocks; rq.histogram_done = true;
  GroupingCounts hstats;
  VI_TRY(group_probes(ix, ctx, rq, hstats));
  stt.scanned_vectors = hstats[kStatScannedVectors];
  stt.scan_items = hstats[kStatItems];
  const uint64_t nsegruns = hstats[kStatSegRuns];
  VI_TRY(ws.seg_run_dist.reserve(nsegruns * K));
  VI_TRY(ws.seg_run_pos.reserve(nsegruns * K));
  if (rank_timing) VI_HIP(hipEventRecord(ctx.ev[2], st));
  // ---- 4. list scan ----
  {
    ScanArgs a{};
    a.blocks = (const float4 *)ix.lists.blocks.p; a.dq = dq; a.dim = dim; a.Q = b.Qd; a.nq = (uint32_t)nq;
    a.K = K; a.run_dist = ws.run_dist.p; a.run_pos = ws.run_pos.p;
    a.first_block = ix.list_first_block.p; a.list_len = ix.list_len.p; a.item_start = ws.item_start.p;
    a.seg_start = ws.seg_start.p; a.pairs = ws.pairs.p; a.nlists = (uint32_t)nlists; a.P = P;
    a.segb0 = kSegBlocks; a.segrun_start = ws.segrun_start.p;
    a.seg_run_dist = ws.seg_run_dist.p; a.seg_run_pos = ws.seg_run_pos.p;
    a.allow = b.flt ? b.flt->allow.p : nullptr;  // excluded vectors never enter a run: the merges below see none of them
    VI_TRY(launch_scan(a, qg_l, ix.order, false, (uint32_t)hstats[kStatItems], st));
    if (nsegruns) {
      SegMergeArgs m{ws.seg_start.p, ws.segrun_start.p, ix.list_len.p, ws.pairs.p, (uint32_t)nlists, kSegBlocks, K,
                     ws.seg_run_dist.p, ws.seg_run_pos.p, ws.run_dist.p, ws.run_pos.p};
      const uint32_t npairs = (uint32_t)(nq * P);
      hipLaunchKernelGGL(seg_merge_kernel, dim3((npairs + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlockThreads),
                         0, st, m);
      VI_HIP(hipGetLastError());
    }
  }
  if (rank_timing) VI_HIP(hipEventRecord(ctx.ev[3], st));
  // ---- 5. final merge ----
  {
    FinalMergeArgs a{ws.run_dist.p, ws.run_pos.p, (uint32_t)nq, P, K, (uint32_t)k, ws.probes.p, ws.gorder.p,
                     ix.list_first_block.p, ix.ext_ids.p, out.D, out.I, out.tie, out.slots, out.counts};
    hipLaunchKernelGGL(final_merge_kernel, dim3((uint32_t)((nq + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kBlockThreads), 0, st, a);
    VI_HIP(hipGetLastError());
  }
  if (timing) VI_HIP(hipEventRecord(ctx.ev[4], st));
  return VI_OK;
}

vi_status merge_partials_device(int device, uint64_t nq, uint64_t k, uint32_t parts, const float *D_parts,
                                const int64_t *I_parts, const uint64_t *tie_parts, float *D_out, int64_t *I_out) {
  if (parts == 0 || parts > kWave) return fail(VI_ERR_INVALID_INPUT, "parts must be 1..64");
  if (nq == 0 || k == 0) return VI_OK;
  VI_HIP(hipSetDevice(device));
  hipLaunchKernelGGL(merge_partials_kernel, dim3((uint32_t)((nq + kWavesPerBlock - 1) / kWavesPerBlock)),
                     dim3(kBlockThreads), 0, 0, nq, (uint32_t)k, parts, D_parts, I_parts, tie_parts, (size_t)(nq * k),
                     (size_t)(nq * k), D_out, I_out);
  VI_HIP(hipGetLastError());
  VI_HIP(hipStreamSynchronize(0));
  return VI_OK;
}

// parts packed one after the other, each [D f32 nq*k | pad to 8 B | I i64 nq*k | tie u64 nq*k]: what ONE all-gather of a
// rank's packed results produces
vi_status merge_partials_packed_device(int device, uint64_t nq, uint64_t k, uint32_t parts, const void *packed,
                                       float *D_out, int64_t *I_out) {
  if (parts == 0 || parts > kWave) return fail(VI_ERR_INVALID_INPUT, "parts must be 1..64");
  if (nq == 0 || k == 0) return VI_OK;
  VI_HIP(hipSetDevice(device));
  const size_t offI = (nq * k * 4 + 7) / 8 * 8, offT = offI + nq * k * 8, stride = offT + nq * k * 8;
  const uint8_t *b = static_cast<const uint8_t *>(packed);
  hipLaunchKernelGGL(merge_partials_kernel, dim3((uint32_t)((nq + kWavesPerBlock - 1) / kWavesPerBlock)),
                     dim3(kBlockThreads), 0, 0, nq, (uint32_t)k, parts, reinterpret_cast<const float *>(b),
                     reinterpret_cast<const int64_t *>(b + offI), reinterpret_cast<const uint64_t *>(b + offT),
                     stride / 4, stride / 8, D_out, I_out);
  VI_HIP(hipGetLastError());
  VI_HIP(hipStreamSynchronize(0));
  return VI_OK;
}

vi_status l2sq_pairs_device(const float *a, const float *b, uint64_t n, uint32_t d, int order, float *out) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(VI_ERR_DEVICE, "no HIP device visible");
  if (n == 0) return VI_OK;
  DevBuf<float> da, db, dout;
  VI_TRY(da.reserve(n * d));
  VI_TRY(db.reserve(n * d));
  VI_TRY(dout.reserve(n));
  VI_HIP(hipMemcpy(da.p, a, n * d * 4, hipMemcpyHostToDevice));
  VI_HIP(hipMemcpy(db.p, b, n * d * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(l2sq_pairs_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, da.p, db.p, n, d, order,
                     dout.p);
  VI_HIP(hipGetLastError());
  VI_HIP(hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
  return VI_OK;
}

}  // namespace vi
