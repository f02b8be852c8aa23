// flat_ip.hip — exact (flat) inner-product k-NN over every resident record: per query the k records with the LARGEST
// score q.v, from one dense sweep of ALL blocks against ALL queries on the matrix cores (the contract is
// vi_indexer_search_exact_ip in include/vi_amd.h).  The score is the f32 chain of ip_scalar (flat_common.hpp).
//
// The resident bf16 block images are those of the L2 calls (§4r – §4u): their accumulator ||v'||^2 - 2 q'.v', started at
// zero instead of at the norms and fed the UNCENTRED query, is -2 q.v' = -2 q.v + 2 q.mu (v' = v - mu, mu = 0 where the
// index is not centred).  Nothing new is resident.
//
//   1. seed     the ordinary (L2, probed) top-k search at seed_probe, slots asked for.  flat_ip_prepare_kernel, one wave
//               per query: the chain score of the seed's k hits, their smallest t_q — the hits are k distinct admitted
//               records, so the k-th largest score of the index is >= t_q whatever the seed found — the rank threshold
//               thr_q (below) and the bf16 hi / lo image of -2 q.  A query whose seed holds fewer than k records, or whose
//               magnitude the rank arithmetic cannot be trusted with, is flagged for step 4 and skipped by the sweep.
//   1b. ladder  ip_seed_ladder (flat_ip_seed.hip): hi-plane sweeps over nested samples of the blocks raise
//               t_q to the k-th largest chain score each sample holds and re-form thr_q; a query with fewer than k seed
//               hits may gain its bound there.  VI_EXACT_IP_LADDER=0 skips it; no result depends on it.
//   2. sweep    flat_ip_sweep_kernel: the blocking of the radius sweep (§4s) — 256 threads own 128 queries and a strided
//               share of all blocks, a wave owns one 32-column tile, B fragments (hi and lo) in registers for the whole
//               sweep at D <= 128, block images by LDS-DMA into two buffers, bf16 x 3 on v_mfma_f32_32x32x16_bf16 — with
//               NO norm staged or read: the two accumulators start at 0, at kBig on pad slots and on slots a filter
//               excludes (one 64-bit word per block, fetched a block ahead).  Per accumulator tile: !(x > thr_q), one
//               ballot, survivors into a per-wave LDS queue of 32 x 32 entries, drained 64 at a time: the chain score s
//               from the f32 blocks, kept if s >= t_q, appended with one atomicAdd as (descending score bits, ordinal).
//   3. finish   flat_ip_finish_kernel: one wave per query sorts its candidates in LDS, cuts at k, resolves ordinals to ids
//               and undoes the key map.
//   4. overflow flat_ip_keys_kernel writes the key of every admitted record for each flagged query, sort_rows_u64 sorts
//               the rows, flat_ip_take_kernel cuts at k.  Slow and always right.
// The seed's own hits are not copied into the candidates: their scores are >= t_q, so the sweep meets them like any
// other record and nothing can be appended twice.  No result depends on a rank value.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "device_index.hpp"
#include "flat_common.hpp"
#include "flat_ip.hpp"
#include "flat_ip_seed.hpp"
#include "mfma_bf16.hpp"
#include "record_fetch.hpp"
#include "search_internal.hpp"
#include "select_device.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

constexpr uint32_t kTileQ = 128;       // queries per workgroup: four waves of one 32-column B tile each
constexpr uint32_t kMaxChunks = 8;     // D <= 128: chunks of 16 dimensions whose B fragments a wave keeps in registers
constexpr uint32_t kStreamChunks = 2;  // D > 128: chunks per K step (both operands stream through LDS)
constexpr uint32_t kQueueLen = 1024;   // survivors of one wave and accumulator tile: 32 queries x 32 vectors, never more
constexpr uint64_t kNoKey = ~0ull;
constexpr uint64_t kOverflowKeys = 1ull << 25;  // keys of one chunk of overflow rows (256 MB)

enum { kCountSurvivors = 0, kCountCandidates = 1, kCounters = 2 };
constexpr uint32_t kAllCounters = kCounters + kIpSeedCounters;  // the final sweep's, then the ladder's (flat_ip_seed.hpp)

__global__ void flat_ip_clear_kernel(uint32_t *cnt, uint32_t *ovf, uint32_t nq, unsigned long long *counters) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < kAllCounters) counters[q] = 0ull;
  if (q < nq) { cnt[q] = 0u; ovf[q] = 0u; }
}

// ---- step 1: bound, threshold and image of every query; one wave per query ----
struct IpPrepareArgs {
  SelectCommon c;             // the frame of lists ranked with bf16 x 3: mu, e_scale, gamma, xmax2 = max ||v'||^2
  const uint64_t *seed_slots; // [nq][k] global slots of the seed's hits, all ones where it found none
  float vmax_raw;             // max ||v|| over the stored vectors, uncentred (rounded up): the chain's own rounding
  uint32_t nq, k, nc;
  IpQueryTerms t;             // the bound, both thresholds and the frame terms the ladder re-forms them from
  uint32_t *cnt, *ovf;
  uint4 *qimg;  // [query][plane hi / lo][chunk][half] x 16 B of -2 q: the layout of split_query_image, not centred
  unsigned long long *counters;
};

__global__ void __launch_bounds__(256) flat_ip_prepare_kernel(IpPrepareArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x < kAllCounters) a.counters[threadIdx.x] = 0ull;
  if (q >= a.nq) return;
  SelectCommon c0 = a.c;  // the query as it is: ||q||^2, its image and the budget E all live in the uncentred frame
  c0.mu = nullptr;
  const QueryFrame f = query_frame<false>(c0, q, lane, nullptr, nullptr);
  const float *row = a.c.Q + (size_t)q * a.c.dim;
  float qm, am;  // q.mu and sum |q_i mu_i|
  ip_centre_terms(a.c, row, lane, qm, am);
  float t = INFINITY;  // the smallest chain score among the seed's hits
  bool missing = false;
  for (uint32_t i = lane; i < a.k; i += kWave) {
    const uint64_t slot = a.seed_slots[(size_t)q * a.k + i];
    if (slot == kNoKey) { missing = true; continue; }
    t = fminf(t, ip_scalar(row, a.c.blocks + (size_t)(slot >> 6) * a.c.dq * kWave + (slot & 63ull), a.c.dim));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t = fminf(t, __shfl_xor(t, o));
  const bool bounded = !f.distrust && __ballot(missing) == 0ull && fabsf(t) < 1.0e37f;
  const float thr = ip_rank_threshold(a.c, f, qm, am, a.vmax_raw, t);  // (flat_common.hpp)
  if (lane == 0) {
    const bool ok = bounded && fabsf(thr) < 1.0e37f;  // (a NaN or huge threshold: no bound)
    a.t.thr[q] = ok ? thr : -INFINITY;
    a.t.tq[q] = a.t.t0[q] = ok ? t : -INFINITY;
    // the sampled levels compare without margins; a query without a bound admits everything there and may gain one,
    // unless its magnitude is distrusted
    a.t.sthr[q] = f.distrust ? -INFINITY : (ok ? -2.0f * t + 2.0f * qm : INFINITY);
    a.t.qn[q] = f.qn; a.t.E[q] = f.E; a.t.qm[q] = qm; a.t.am[q] = am;
    a.cnt[q] = 0u;
    a.ovf[q] = ok ? 0u : 1u;
  }
  split_query_image(c0, q, a.nc, lane, a.qimg);
}

// ---- step 2: the sweep ----
struct IpSweepArgs {
  const uint4 *img;     // the lists' bf16 image: [block][chunk][plane][half][64 columns] x 16 B (rank_images.hip)
  const uint4 *qimg;
  const float4 *blocks;
  const float *Q;
  const uint32_t *block_ord, *block_cnt;
  const uint64_t *allow;  // one allow word per block, or null
  const float *thr;       // [nq] -inf: the overflow path answers the query
  const float *tq;        // [nq] the score a candidate must reach
  uint32_t *cnt, *ovf;
  uint64_t *cand;         // [nq][cap]
  unsigned long long *counters;
  uint32_t nq, dim, dq, nc, nblocks, nsplit, cap;
  uint32_t lo_planes;     // the lists' lo planes are multiplied (some stored value is not bf16-exact)
};

// LDS, in 16-byte words: two K-step buffers and the waves' survivor queues — 2 x 32 KB + 8 KB = 72 KB with the queries
// RESIDENT in registers at D = 128: two workgroups per CU.  A K step holds `kc` chunks of a block's image — all of them
// when RESIDENT — and, when the queries stream, the same chunks of the tile's 128 queries behind them.
__host__ __device__ inline uint32_t ip_step_words(bool resident, uint32_t nc) {
  return resident ? nc * 256u : kStreamChunks * (256u + 512u);
}
__host__ __device__ inline uint32_t ip_lds_words(bool resident, uint32_t nc) {
  return 2u * ip_step_words(resident, nc) + 4u * kQueueLen * 2u / 16u;
}

template <bool RESIDENT>
__global__ void __launch_bounds__(256, 2) flat_ip_sweep_kernel(IpSweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_ip[];
  const uint32_t q0 = blockIdx.x * kTileQ, split = blockIdx.y;
  if (split >= a.nblocks) return;  // (the host launches nsplit <= nblocks; workgroup-uniform, before any barrier)

  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const uint32_t nc = a.nc, kc = RESIDENT ? nc : kStreamChunks, nslab = RESIDENT ? 1u : (nc + kc - 1) / kc;
  const uint32_t bufsz = ip_step_words(RESIDENT, nc);
  uint16_t *s_queue = (uint16_t *)(s_ip + 2 * bufsz) + (uint32_t)wave * kQueueLen;
  const uint32_t nmine = (a.nblocks - split + a.nsplit - 1) / a.nsplit, nsteps = nmine * nslab;
  const uint64_t below = (1ull << lane) - 1ull;

  const uint32_t w0 = q0 + 32u * (uint32_t)wave, qg = w0 + (uint32_t)j;  // this lane's query: both lane halves hold column j
  const float thr = qg < a.nq ? a.thr[qg] : -INFINITY;                    // (-inf: no query, or one the overflow path answers)
  const bool lane_live = thr > -INFINITY;
  const bool wave_live = __ballot(lane_live) != 0ull;

  // RESIDENT: the B fragments of this lane's query, hi and lo, of every chunk: 2 x 4 VGPRs per chunk, read once.  The loop
  // is unrolled over the most chunks there can be, under a wave-uniform guard, so that every index is a constant
  bf16x8 bh[kMaxChunks], bl[kMaxChunks];
  if (RESIDENT) {
    const uint4 *qi = a.qimg + (size_t)min(qg, a.nq - 1u) * 4 * nc;  // (a tile's tail repeats the last query)
#pragma unroll
    for (uint32_t c = 0; c < kMaxChunks; ++c) {
      uint4 vh = make_uint4(0u, 0u, 0u, 0u), vl = vh;
      if (c < nc) { vh = qi[2 * c + (uint32_t)h]; vl = qi[2 * nc + 2 * c + (uint32_t)h]; }
      bh[c] = __builtin_bit_cast(bf16x8, vh);
      bl[c] = __builtin_bit_cast(bf16x8, vl);
    }
  }

  // streaming: chunks [c0, c0 + kcs) of the tile's query image -> dst: piece (chunk, plane, half) of 128 queries = 2 KB
  auto stage_queries = [&](float *dst, uint32_t c0, uint32_t kcs) {
    for (uint32_t pi = wave; pi < kcs * 8u; pi += 4u) {
      const uint32_t piece = pi >> 1, qh = pi & 1u, c = piece >> 2, pc = piece & 3u;
      const uint32_t q = min(q0 + 64u * qh + (uint32_t)lane, a.nq - 1u);
      glds16_asm(a.qimg + (size_t)q * 4 * nc + (pc >> 1) * 2 * nc + 2 * (c0 + c) + (pc & 1u), dst + (piece * 128u + 64u * qh) * 4u);
    }
  };
  // K step `step` of this workgroup -> buffer `buf`: nothing but the image (no norms, no bounds)
  auto stage = [&](uint32_t step, uint32_t buf) {
    const uint32_t b = split + (step / nslab) * a.nsplit, s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    float *dst = (float *)(s_ip + buf * bufsz);
    const uint4 *src = a.img + ((size_t)b * nc + c0) * 256 + lane;
    for (uint32_t p = wave; p < kcs * 4u; p += 4u) glds16_asm(src + p * 64u, dst + p * 256u);
    if (!RESIDENT) stage_queries(dst + kStreamChunks * 1024u, c0, kcs);
  };
  // the slots of block b that take part: records (no pad slot) the filter admits; wave-uniform, two scalar loads
  auto live_slots = [&](uint32_t b) -> uint64_t {
    const uint32_t nrec = a.block_cnt[b];
    const uint64_t rec = nrec >= 64u ? ~0ull : (1ull << nrec) - 1ull;
    return a.allow ? (a.allow[b] & rec) : rec;
  };

  f32x16 acc0, acc1;  // vectors 0..31 and 32..63 of the block's image x this wave's 32 queries
  uint32_t nsurv = 0;

  // chunk c of the K step in s_a against the B fragments (fh, fl): the three products of bf16 x 3
  auto multiply = [&](const uint4 *s_a, uint32_t c, const bf16x8 &fh, const bf16x8 &fl) {
    const bf16x8 h0 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 0u + h) * 64u + j]);
    const bf16x8 h1 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 0u + h) * 64u + 32u + j]);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, fh, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, fh, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, fl, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, fl, acc1, 0, 0, 0);
    if (a.lo_planes) {
      const bf16x8 l0 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 2u + h) * 64u + j]);
      const bf16x8 l1 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 2u + h) * 64u + 32u + j]);
      acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(l0, fh, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(l1, fh, acc1, 0, 0, 0);
    }
  };

  // ---- epilogue of one accumulator tile: register r of tile t in lane half h is vector 32 t + 16 h + r of the block ----
  auto epilogue = [&](const f32x16 &acc, uint32_t t, uint32_t b, uint64_t live) {
    uint32_t m = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) m |= (!(acc[r] > thr) ? 1u : 0u) << r;  // (!(x > y): a NaN rank value is evaluated, never skipped)
    if (!lane_live) m = 0u;
    if (__ballot(m != 0u) == 0ull) return;
    uint32_t n = 0;  // survivors (query of the wave | vector << 5), compacted into the wave's queue
    for (uint32_t bit = 0; bit < 16u; ++bit) {
      const bool sv = (m >> bit) & 1u;
      const uint64_t bal = __ballot(sv);
      if (!bal) continue;
      if (sv) s_queue[n + (uint32_t)__popcll(bal & below)] = (uint16_t)((uint32_t)j | ((32u * t + 16u * (uint32_t)h + bit) << 5));
      n += (uint32_t)__popcll(bal);
    }
    wave_lds_sync();
    nsurv += n;
    const uint32_t ord0 = a.block_ord[b];
    // ---- the drain: 64 entries a round, each evaluated in the chain and kept if it reaches the query's t_q ----
    for (uint32_t at = 0; at < n; at += kWave) {
      const uint32_t i = at + (uint32_t)lane;
      const uint32_t e = i < n ? s_queue[i] : 0u;
      const uint32_t q = w0 + (e & 31u), v = e >> 5;
      if (i < n && q < a.nq && ((live >> v) & 1ull)) {  // a record (no pad slot) that the filter admits
        const float s = ip_scalar(a.Q + (size_t)q * a.dim, a.blocks + (size_t)b * a.dq * kWave + v, a.dim);
        if (s >= a.tq[q]) {
          const uint32_t pos = atomicAdd(a.cnt + q, 1u);
          if (pos < a.cap) a.cand[(size_t)q * a.cap + pos] = ip_key(s, ord0 + v);  // (nothing is written past the array)
          else a.ovf[q] = 1u;
        }
      }
    }
    wave_lds_sync();  // the queue is free again
  };

  stage(0, 0);
  uint64_t live = live_slots(split), live_next = 0ull;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (uint32_t step = 0; step < nsteps; ++step) {
    const uint32_t cur = step & 1u;
    const uint32_t b = split + (step / nslab) * a.nsplit, s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    // the next step lands in the other buffer under this step's MFMAs (every wave left it at the last barrier); where
    // it begins a block, that block's live word comes with it
    if (step + 1 < nsteps) {
      stage(step + 1, cur ^ 1u);
      if (s + 1 == nslab) live_next = live_slots(b + a.nsplit);
    }
    if (wave_live) {
      const uint4 *s_a = s_ip + cur * bufsz;
      if (s == 0) {  // no norm: 0 where a record takes part, kBig elsewhere (vector 32 t + 16 h + r in register r)
        const uint32_t l0 = (uint32_t)(live >> (16u * (uint32_t)h)), l1 = (uint32_t)(live >> (32u + 16u * (uint32_t)h));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          acc0[r] = ((l0 >> r) & 1u) ? 0.0f : kBig;
          acc1[r] = ((l1 >> r) & 1u) ? 0.0f : kBig;
        }
      }
      if (RESIDENT) {
#pragma unroll
        for (uint32_t c = 0; c < kMaxChunks; ++c)
          if (c < nc) multiply(s_a, c, bh[c], bl[c]);
      } else {
        const uint4 *s_b = s_a + kStreamChunks * 256u;
        for (uint32_t c = 0; c < kcs; ++c) {
          const bf16x8 fh = __builtin_bit_cast(bf16x8, s_b[(c * 4u + 0u + h) * 128u + 32u * wave + j]);
          const bf16x8 fl = __builtin_bit_cast(bf16x8, s_b[(c * 4u + 2u + h) * 128u + 32u * wave + j]);
          multiply(s_a, c, fh, fl);
        }
      }
      if (s + 1 == nslab) {  // the queue is drained once per accumulator tile: 32 x 32 entries can never overflow it
        epilogue(acc0, 0u, b, live);
        epilogue(acc1, 1u, b, live);
      }
    }
    if (s + 1 == nslab) live = live_next;
    // the next step has landed (this wave's loads, stores and atomics too), every wave is done with this buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  if (lane == 0 && nsurv) atomicAdd(a.counters + kCountSurvivors, (unsigned long long)nsurv);
}

// ---- steps 3 and 4: sorted keys -> the rows of the caller ----
struct IpOutArgs {
  const uint32_t *block_ord;
  const uint64_t *ext_ids;
  uint32_t nblocks, k;
  float *S;
  int64_t *I;
  uint64_t *ord, *counts;  // or null
};

// one wave: row q of the outputs from `navail` ascending keys (kNoKey: none from there on)
__device__ __forceinline__ void ip_emit_row(const IpOutArgs &o, uint32_t q, const uint64_t *keys, uint32_t navail, int lane) {
  uint32_t found = 0;
  for (uint32_t i = lane; i < o.k; i += kWave) {
    const uint64_t key = i < navail ? keys[i] : kNoKey;
    const size_t at = (size_t)q * o.k + i;
    if (key == kNoKey) {
      o.S[at] = -INFINITY; o.I[at] = -1;
      if (o.ord) o.ord[at] = kNoKey;
      continue;
    }
    ++found;
    const uint32_t ordinal = (uint32_t)key;
    const uint32_t lo = block_of_ordinal(o.block_ord, o.nblocks, ordinal);
    o.S[at] = ip_key_score(key);
    o.I[at] = (int64_t)o.ext_ids[(size_t)lo * kWave + (ordinal - o.block_ord[lo])];
    if (o.ord) o.ord[at] = ordinal;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) found += (uint32_t)__shfl_xor((int)found, s);
  if (o.counts && lane == 0) o.counts[q] = found;
}

// one wave per query: its candidates sorted in LDS (a bitonic network over the next power of two), cut at k
__global__ void __launch_bounds__(64) flat_ip_finish_kernel(IpOutArgs o, const uint64_t *cand, const uint32_t *cnt, const uint32_t *ovf,
                                                            uint32_t cap, unsigned long long *counters) {
  extern __shared__ __attribute__((aligned(16))) uint64_t s_ip_keys[];
  const int lane = threadIdx.x;
  const uint32_t q = blockIdx.x;
  if (ovf[q]) return;  // (step 4 writes the row)
  const uint32_t n = min(cnt[q], cap);
  uint32_t P = kWave;
  while (P < n) P <<= 1;
  for (uint32_t i = lane; i < P; i += kWave) s_ip_keys[i] = i < n ? cand[(size_t)q * cap + i] : kNoKey;
  wave_lds_sync();
  for (uint32_t k2 = 2; k2 <= P; k2 <<= 1)
    for (uint32_t j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      for (uint32_t t = lane; t < P / 2; t += kWave) {
        const uint32_t i = ((t & ~(j2 - 1u)) << 1) | (t & (j2 - 1u));
        const uint64_t x = s_ip_keys[i], y = s_ip_keys[i + j2];
        if ((x > y) == ((i & k2) == 0u)) { s_ip_keys[i] = y; s_ip_keys[i + j2] = x; }
      }
      wave_lds_sync();
    }
  ip_emit_row(o, q, s_ip_keys, P, lane);
  if (lane == 0 && n) atomicAdd(counters + kCountCandidates, (unsigned long long)n);
}

// row r of `keys` (2^logL each): the key of every record query rows[r] is offered, kNoKey on every other place
__global__ void __launch_bounds__(256) flat_ip_keys_kernel(IpSweepArgs a, const uint32_t *rows, uint32_t logL, uint64_t *keys) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, q = rows[blockIdx.y];
  if (i >= (1u << logL)) return;
  uint64_t key = kNoKey;
  const uint32_t b = i >> 6, v = i & 63u;
  if (b < a.nblocks && v < a.block_cnt[b] && (!a.allow || ((a.allow[b] >> v) & 1ull)))
    key = ip_key(ip_scalar(a.Q + (size_t)q * a.dim, a.blocks + (size_t)b * a.dq * kWave + v, a.dim), a.block_ord[b] + v);
  keys[((size_t)blockIdx.y << logL) + i] = key;
}

__global__ void __launch_bounds__(64) flat_ip_take_kernel(IpOutArgs o, const uint64_t *keys, uint32_t logL, const uint32_t *rows) {
  ip_emit_row(o, rows[blockIdx.x], keys + ((size_t)blockIdx.x << logL), 1u << logL, (int)threadIdx.x);
}

thread_local vi_exact_stats g_last_stats{};
thread_local vi_exact_ip_seed_stats g_last_seed_stats{};

vi_status exact_ip_in_context(const DeviceIndex &ix, SearchContext &ctx, const ExactIO &io) {
  SearchWorkspace &ws = ctx.ws;
  auto &fw = ws.flat;
  hipStream_t st = ctx.stream;
  const uint64_t nq = io.nq, k = io.k;
  const uint32_t dim = ix.dim, nc = ix.dq / 4, nblocks = (uint32_t)ix.lists.nblocks;
  const char *te = getenv("VI_EXACT_TIMING");
  const bool timing = te && *te != '0';
  const char *le = getenv("VI_EXACT_IP_LADDER");
  const bool ladder = !(le && *le == '0');
  vi_exact_stats es{};
  vi_exact_ip_seed_stats ss{};
  es.nq = nq; es.k = k; es.query_tile = kTileQ;
  es.cand_cap = exact_cand_cap(io.cand_cap, k);
  es.seed_probe = std::min<uint64_t>(io.seed_probe ? io.seed_probe : kExactSeedProbe, std::max<uint64_t>(1, ix.nlists));
  const uint32_t cap = (uint32_t)es.cand_cap;
  if (nq * std::max<uint64_t>(k, 64) > 0x7FFFFFFFull || nq * (uint64_t)cap > (1ull << 33))
    return fail(VI_ERR_INVALID_INPUT, "batch too large: split nq");
  const double t0 = now_ms();

  // ---- queries and outputs on the device ----
  const float *Qd = io.queries;
  if (!io.on_device) {
    VI_TRY(ws.q.reserve(nq * dim));
    VI_HIP(hipMemcpyAsync(ws.q.p, io.queries, nq * dim * sizeof(float), hipMemcpyHostToDevice, st));
    Qd = ws.q.p;
  }
  IpOutArgs o{nullptr, ix.ext_ids.p, nblocks, (uint32_t)k, io.D, io.I, io.ord, io.counts};
  if (!io.on_device) {
    VI_TRY(fw.D.reserve(nq * k));
    VI_TRY(fw.I.reserve(nq * k));
    o.S = fw.D.p; o.I = fw.I.p;
    if (io.ord) { VI_TRY(fw.ord.reserve(nq * k)); o.ord = fw.ord.p; }
    if (io.counts) { VI_TRY(fw.counts.reserve(nq)); o.counts = fw.counts.p; }
  }
  VI_TRY(fw.cnt.reserve(nq));
  VI_TRY(fw.ovf.reserve(nq));
  VI_TRY(fw.cand.reserve(nq * cap));
  VI_TRY(fw.counters.reserve(kAllCounters));
  const dim3 per_query((uint32_t)((std::max<uint64_t>(nq, kAllCounters) + 255) / 256)), per_wave((uint32_t)((nq + 3) / 4));
  std::vector<uint32_t> h_ovf(nq, 0u);

  const bool empty = ix.nlists == 0 || ix.nvec_resident == 0 || nblocks == 0;
  double t2 = t0;  // where the finish begins
  if (empty) {  // nothing is resident: every row is padding
    hipLaunchKernelGGL(flat_ip_clear_kernel, per_query, dim3(256), 0, st, fw.cnt.p, fw.ovf.p, (uint32_t)nq, fw.counters.p);
    VI_HIP(hipGetLastError());
  } else {
    // ---- 1. seed: the L2 search's hits, by slot ----
    VI_TRY(fw.seed_D.reserve(nq * k));
    VI_TRY(fw.seed_I.reserve(nq * k));
    VI_TRY(ws.slots.reserve(nq * k));
    SearchIO sio;
    sio.queries = Qd; sio.on_device = true; sio.nq = nq; sio.k = k; sio.n_probe = es.seed_probe;
    sio.D = fw.seed_D.p; sio.I = fw.seed_I.p; sio.slots = ws.slots.p; sio.filter = io.filter;
    VI_TRY(topk_search(ix, ctx, sio));  // (synchronised)
    es.ms_seed = timing ? (float)(now_ms() - t0) : 0.0f;
    const double t1 = now_ms();

    // ---- 2. bounds, images, sweep ----
    VI_TRY(ensure_fetch_layout(ix, st));
    VI_TRY(fw.block_ord.reserve(nblocks));
    VI_TRY(fw.block_cnt.reserve(nblocks));
    VI_TRY(fw.thr.reserve(IpQueryTerms::kArrays * nq));  // the thresholds, the scores t_q and the frame terms behind them
    VI_TRY(fw.qimg.reserve(nq * nc * 16));
    hipLaunchKernelGGL(flat_blocks_kernel, dim3((nblocks + 255) / 256), dim3(256), 0, st, ix.list_first_block.p, ix.list_len.p,
                       ix.fetch.prefix.p, (uint32_t)ix.nlists, nblocks, fw.block_ord.p, fw.block_cnt.p);
    o.block_ord = fw.block_ord.p;
    // the frame of lists ranked with bf16 x 3 whatever the engines' switches say: this sweep multiplies nothing else
    SearchBatch b{ix, ctx, io.filter, nullptr, nullptr};
    b.kn = read_engine_knobs();
    b.kn.rank_bf16 = true; b.kn.stats = false;
    b.Qd = Qd; b.nq = nq;
    const SelectCommon c = select_common(b, (const float4 *)ix.lists.blocks.p, ix.centered ? ix.xmax2_c : ix.xmax2, kTileQ);
    const IpQueryTerms terms = IpQueryTerms::at(fw.thr.p, nq);
    const float *tq = terms.tq;
    const float vmax_raw = (float)(std::sqrt((double)ix.xmax2) * 1.0001);
    IpPrepareArgs pa{c, ws.slots.p, vmax_raw, (uint32_t)nq, (uint32_t)k, nc, terms, fw.cnt.p, fw.ovf.p, (uint4 *)fw.qimg.p, fw.counters.p};
    hipLaunchKernelGGL(flat_ip_prepare_kernel, per_wave, dim3(256), 0, st, pa);
    VI_HIP(hipGetLastError());

    int cus = 0;
    VI_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix.device));
    const uint64_t *allow = io.filter ? io.filter->allow.p : nullptr;

    // ---- 1b. the ladder: sampled hi-plane sweeps raise t_q before the sweep that has to be sound ----
    if (ladder) {
      const IpSeedSchedule sched = ip_seed_schedule(nblocks, cap, k);
      ss.levels = sched.levels; ss.ratio = sched.ratio;
      for (uint32_t l = 0; l < sched.levels; ++l) ss.strides[l] = sched.strides[l];
      double tl = 0.0;
      if (timing) { VI_HIP(hipStreamSynchronize(st)); tl = now_ms(); }
      IpLadderArgs la{c, vmax_raw, (const uint4 *)ix.lists_bf16.p, (const uint4 *)fw.qimg.p, fw.block_cnt.p, allow, terms, fw.cnt.p,
                      fw.ovf.p, (uint32_t *)fw.cand.p, fw.counters.p + kCounters, (uint32_t)nq, (uint32_t)k, nc, nblocks, cap, cus};
      VI_TRY(ip_seed_ladder(la, sched, st));
      if (timing) { VI_HIP(hipStreamSynchronize(st)); ss.ms_ladder = (float)(now_ms() - tl); }
    }
    const uint32_t ntiles = (uint32_t)((nq + kTileQ - 1) / kTileQ);
    // two workgroups per CU at a time: two rounds of them, so that the tail of the grid is short
    const uint32_t nsplit = exact_block_splits(4u, cus, ntiles, nblocks);
    es.block_splits = nsplit;
    IpSweepArgs sa{(const uint4 *)ix.lists_bf16.p, (const uint4 *)fw.qimg.p, (const float4 *)ix.lists.blocks.p, Qd,
                   fw.block_ord.p, fw.block_cnt.p, allow, terms.thr, tq, fw.cnt.p, fw.ovf.p,
                   fw.cand.p, fw.counters.p, (uint32_t)nq, dim, ix.dq, nc, nblocks, nsplit, cap, ix.lists_lo_zero ? 0u : 1u};
    const bool resident = dim <= kNarrowDim;
    const int lds = (int)(ip_lds_words(resident, nc) * 16u);
    const void *fn = resident ? (const void *)flat_ip_sweep_kernel<true> : (const void *)flat_ip_sweep_kernel<false>;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
      return fail(VI_ERR_DEVICE, "cannot reserve %d bytes of LDS for the exact inner-product search's sweep", lds);
    if (resident) hipLaunchKernelGGL(flat_ip_sweep_kernel<true>, dim3(ntiles, nsplit), dim3(256), lds, st, sa);
    else hipLaunchKernelGGL(flat_ip_sweep_kernel<false>, dim3(ntiles, nsplit), dim3(256), lds, st, sa);
    VI_HIP(hipGetLastError());
    if (timing) {
      VI_HIP(hipStreamSynchronize(st));
      es.ms_sweep = (float)(now_ms() - t1) - ss.ms_ladder;
    }
    t2 = now_ms();

    // ---- 4. the rows the sweep could not answer (read back first: the finish kernel skips them) ----
    VI_HIP(hipMemcpyAsync(h_ovf.data(), fw.ovf.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
    std::vector<uint32_t> rows;
    for (uint64_t q = 0; q < nq; ++q)
      if (h_ovf[q]) rows.push_back((uint32_t)q);
    es.overflow_rows = rows.size();
    if (!rows.empty()) {
      uint32_t logL = 11;  // (sort_rows_u64: rows of at least 2048 keys)
      while ((1ull << logL) < (uint64_t)nblocks * kWave) ++logL;
      const uint64_t chunk = std::max<uint64_t>(1, kOverflowKeys >> logL);
      VI_TRY(upload(fw.rows, rows.data(), rows.size(), st));
      VI_TRY(fw.keys.reserve(std::min<uint64_t>(chunk, rows.size()) << logL));
      for (uint64_t r0 = 0; r0 < rows.size(); r0 += chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, rows.size() - r0);
        hipLaunchKernelGGL(flat_ip_keys_kernel, dim3((1u << logL) / 256u, m), dim3(256), 0, st, sa, fw.rows.p + r0, logL, fw.keys.p);
        VI_HIP(hipGetLastError());
        VI_TRY(sort_rows_u64(fw.keys.p, m, logL, st));
        hipLaunchKernelGGL(flat_ip_take_kernel, dim3(m), dim3(64), 0, st, o, (const uint64_t *)fw.keys.p, logL, fw.rows.p + r0);
        VI_HIP(hipGetLastError());
      }
      VI_HIP(hipStreamSynchronize(st));  // (`rows` is read by its upload until here)
    }
  }

  // ---- 3. finish ----
  uint32_t p2 = kWave;
  while (p2 < cap) p2 <<= 1;
  const int lds_finish = (int)(p2 * sizeof(uint64_t));
  if (hipFuncSetAttribute((const void *)flat_ip_finish_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_finish) != hipSuccess)
    return fail(VI_ERR_DEVICE, "cannot reserve %d bytes of LDS for the exact inner-product search's sort", lds_finish);
  hipLaunchKernelGGL(flat_ip_finish_kernel, dim3((uint32_t)nq), dim3(64), lds_finish, st, o, (const uint64_t *)fw.cand.p, fw.cnt.p, fw.ovf.p, cap, fw.counters.p);
  VI_HIP(hipGetLastError());
  unsigned long long h_count[kAllCounters] = {};
  VI_HIP(hipMemcpyAsync(h_count, fw.counters.p, sizeof(h_count), hipMemcpyDeviceToHost, st));
  if (!io.on_device) {
    VI_HIP(hipMemcpyAsync(io.D, o.S, nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
    VI_HIP(hipMemcpyAsync(io.I, o.I, nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (io.ord) VI_HIP(hipMemcpyAsync(io.ord, o.ord, nq * k * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (io.counts) VI_HIP(hipMemcpyAsync(io.counts, o.counts, nq * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  }
  VI_HIP(hipStreamSynchronize(st));
  es.survivors = h_count[kCountSurvivors];
  es.candidates = h_count[kCountCandidates];
  for (uint32_t l = 0; l < ss.levels; ++l) {
    ss.level_survivors[l] = h_count[kCounters + kSeedCountSurvivors + l];
    ss.level_candidates[l] = h_count[kCounters + kSeedCountCandidates + l];
  }
  ss.rows_tightened = h_count[kCounters + kSeedCountTightened];
  ss.rows_level_overflow = h_count[kCounters + kSeedCountLevelOverflow];
  const double t3 = now_ms();
  es.ms_finish = timing ? (float)(t3 - t2) : 0.0f;
  es.ms_total = timing ? (float)(t3 - t0) : 0.0f;
  g_last_stats = es;
  g_last_seed_stats = ss;
  return VI_OK;
}

}  // namespace

vi_exact_stats exact_ip_last_stats() { return g_last_stats; }
vi_exact_ip_seed_stats exact_ip_seed_last_stats() { return g_last_seed_stats; }

vi_status device_index_search_exact_ip(const DeviceIndex &ix, const ExactIO &io) {
  g_last_stats = vi_exact_stats{};
  g_last_seed_stats = vi_exact_ip_seed_stats{};
  if (io.nq == 0) return VI_OK;
  // the limits of the exact L2 search (§4r): VI_ERR_INVALID_INPUT before any device work, never a slower path
  if (ix.stripe_world > 1) return fail(VI_ERR_INVALID_INPUT, "exact inner-product search needs the whole index on one handle");
  if (ix.order != VI_ORDER_SCALAR)
    return fail(VI_ERR_INVALID_INPUT, "exact inner-product search needs an index whose distances are VI_ORDER_SCALAR");
  if (ix.dim < 4 || (ix.dim & 3) || ix.dim > kMaxMfmaDim)
    return fail(VI_ERR_INVALID_INPUT, "exact inner-product search needs a dimension that is a multiple of 4 and at most %u, not %u",
                kMaxMfmaDim, ix.dim);
  if (ix.lists.nblocks * 64ull >= (1ull << kPosBits))
    return fail(VI_ERR_INVALID_INPUT, "exact inner-product search needs an index of fewer than 2^%u slots", kPosBits);
  if (ix.nvec_resident >= (1ull << 32)) return fail(VI_ERR_INVALID_INPUT, "ordinals must fit 32 bits");  // (implied by the slot limit)
  if (!(ix.xmax2 < 1.0e30f)) return fail(VI_ERR_INVALID_INPUT, "exact inner-product search needs stored vectors of squared norm below 1e30");
  if (ix.lists.nblocks && (!ix.ext_ids.p || !ix.lists_bf16.p)) return fail(VI_ERR_INVALID_INPUT, "this index keeps no external ids or ranking images");
  if (io.filter && io.filter->owner_serial != ix.serial) return fail(VI_ERR_INVALID_INPUT, "the filter was made for another index");
  const vi_status s = with_search_context(ix, [&](SearchContext &ctx) { return exact_ip_in_context(ix, ctx, io); });
  if (s != VI_OK) (void)hipGetLastError();  // (a failed allocation is this call's failure, not the next call's)
  return s;
}

}  // namespace vi
