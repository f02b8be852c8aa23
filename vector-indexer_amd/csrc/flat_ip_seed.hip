// flat_ip_seed.hip — the score-seeded ladder of the exact inner-product search: between the L2 seed's
// bound and the final sweep of flat_ip.hip, a few cheap sweeps over nested samples of the index raise every query's t_q.
//
// The rule it rests on (§4v): the smallest chain score (ip_scalar) among ANY k distinct admitted records is a lower bound
// of the query's true k-th largest score.  So a level may choose records as approximately as it likes; only the scores it
// reports must be the chain's, and t_q := max(t_q, k-th largest chain score the level collected) stays sound.
//
// The samples are measured in blocks of 64 slots: the level of stride s holds the blocks whose index is 0 mod s.  Strides
// are powers of one ratio r, so the samples are nested: what a level found is in every finer one, and a finer level can
// only find more above the bound.  The schedule (ip_seed_schedule):
//   r        the largest power of two <= cand_cap / (2 k), clamped to [2, 4]: a level is expected to collect about k r
//            scores (the records of an r times larger sample above the k-th of the smaller one), at most half of cand_cap.
//            A sample of blocks is a cluster sample — a block's 64 records belong to one list — and the estimate is
//            optimistic for it: replayed on the CPU over 2 000 clustered rows of spread norms (§4x), one level of r = 8
//            left up to 898 candidates to the final sweep where k r is 80, r = 4 left 108, r = 2 left 41.  Hence 4
//   strides  r^m, r^(m-1), ..., r, coarsest first; m is the smallest with ceil(nblocks / r^m) * 64 <= cand_cap, so the
//            coarsest sample cannot collect more than cand_cap scores — or, where cand_cap < 64, the smallest with a
//            sample of one block.  No level where nblocks * 64 <= cand_cap.  At most 8 levels: a longer ladder drops
//            its coarsest ones
//   stride 1 is the unchanged final sweep.
//
//   flat_ip_seed_kernel     one level.  The blocking of the final sweep — 256 threads own 128 queries and a strided share
//            of the sample's blocks, a wave owns one 32-column tile, B fragments in registers for the whole level at
//            D <= 128, block images by LDS-DMA into two buffers, both operands streaming above — but it needs no
//            soundness: it stages and multiplies the HI planes only (one v_mfma_f32_32x32x16_bf16 per chunk and tile
//            where the final sweep issues two or three; half the LDS per block), starts every accumulator at zero,
//            compares against sthr_q = -2 t_q + 2 q.mu with NO margin, and masks pad slots and filtered slots with the
//            block's live word in the epilogue.  Survivors are evaluated in the chain; those with s >= t_q append their
//            32-bit score key (no ordinal: a level meets a record once).  A row that fills its cand_cap keys stores no
//            more and is NOT flagged: its stored keys are still cand_cap distinct admitted records at or above t_q.
//   flat_ip_tighten_kernel  one wave per query: the k-th largest of the keys the level stored (FastTopK / FastTop128,
//            wave_sort.hpp); if the row stored >= k and that score is above t_q it becomes t_q, thr_q is re-formed with
//            ip_rank_threshold from the frame terms flat_ip_prepare_kernel kept, sthr_q for the next level, and a query
//            the L2 seed could not bound (fewer than k hits) gains its bound and leaves the overflow path.  A query of
//            distrusted magnitude takes no part (sthr_q = -inf).  The row's count is cleared for the next level.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "device_index.hpp"
#include "flat_common.hpp"
#include "flat_ip_seed.hpp"
#include "flat_search.hpp"
#include "mfma_bf16.hpp"
#include "wave_sort.hpp"

namespace vi {
namespace {

constexpr uint32_t kTileQ = 128;       // queries per workgroup: four waves of one 32-column B tile each
constexpr uint32_t kMaxChunks = 8;     // D <= 128: chunks of 16 dimensions whose hi B fragments a wave keeps in registers
constexpr uint32_t kStreamChunks = 2;  // D > 128: chunks per K step (both operands stream through LDS)
constexpr uint32_t kQueueLen = 1024;   // survivors of one wave and accumulator tile: 32 queries x 32 vectors, never more

struct IpSeedArgs {
  const uint4 *img, *qimg;
  const float4 *blocks;
  const float *Q;
  const uint32_t *block_cnt;
  const uint64_t *allow;
  const float *sthr, *tq;
  uint32_t *cnt, *keys;
  unsigned long long *survivors;  // this level's counter
  uint32_t nq, dim, dq, nc, nsample, stride, nsplit, cap;
};

// LDS, in 16-byte words: two K-step buffers of hi planes and the waves' survivor queues — 2 x 16 KB + 8 KB = 40 KB with
// the queries RESIDENT at D = 128; 144 VGPRs keep three workgroups on a CU, which 120 KB of its LDS serve.  A K step
// holds the hi plane of `kc` chunks of a block (128 words a chunk) and, when the queries stream, the hi plane of the
// same chunks of the tile's 128 queries behind them (256 words a chunk).
__host__ __device__ inline uint32_t seed_step_words(bool resident, uint32_t nc) {
  return resident ? nc * 128u : kStreamChunks * (128u + 256u);
}
__host__ __device__ inline uint32_t seed_lds_words(bool resident, uint32_t nc) {
  return 2u * seed_step_words(resident, nc) + 4u * kQueueLen * 2u / 16u;
}

template <bool RESIDENT>
__global__ void __launch_bounds__(256, 3) flat_ip_seed_kernel(IpSeedArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_seed[];
  const uint32_t q0 = blockIdx.x * kTileQ, split = blockIdx.y;
  if (split >= a.nsample) return;  // (the host launches nsplit <= nsample; workgroup-uniform, before any barrier)

  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const uint32_t nc = a.nc, kc = RESIDENT ? nc : kStreamChunks, nslab = RESIDENT ? 1u : (nc + kc - 1) / kc;
  const uint32_t bufsz = seed_step_words(RESIDENT, nc);
  uint16_t *s_queue = (uint16_t *)(s_seed + 2 * bufsz) + (uint32_t)wave * kQueueLen;
  // sample block i of this workgroup is block stride * (split + i * nsplit) of the index
  const uint32_t nmine = (a.nsample - split + a.nsplit - 1) / a.nsplit, nsteps = nmine * nslab;
  const uint64_t below = (1ull << lane) - 1ull;

  const uint32_t w0 = q0 + 32u * (uint32_t)wave, qg = w0 + (uint32_t)j;  // this lane's query: both lane halves hold column j
  const float thr = qg < a.nq ? a.sthr[qg] : -INFINITY;                   // (-inf: no query, or one no level may bound)
  const bool lane_live = thr > -INFINITY;
  const bool wave_live = __ballot(lane_live) != 0ull;

  // RESIDENT: the hi B fragment of this lane's query of every chunk: 4 VGPRs per chunk, read once (the unrolled loop
  // under a wave-uniform guard keeps every index a constant)
  bf16x8 bh[kMaxChunks];
  if (RESIDENT) {
    const uint4 *qi = a.qimg + (size_t)min(qg, a.nq - 1u) * 4 * nc;  // (a tile's tail repeats the last query)
#pragma unroll
    for (uint32_t c = 0; c < kMaxChunks; ++c) {
      uint4 vh = make_uint4(0u, 0u, 0u, 0u);
      if (c < nc) vh = qi[2 * c + (uint32_t)h];
      bh[c] = __builtin_bit_cast(bf16x8, vh);
    }
  }

  // K step `step` of this workgroup -> buffer `buf`: piece (chunk, half) of the block's hi plane = 1 KB, and when the
  // queries stream piece (chunk, half) of the hi plane of the tile's 128 queries = 2 KB
  auto stage = [&](uint32_t step, uint32_t buf) {
    const uint32_t b = a.stride * (split + (step / nslab) * a.nsplit), s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    float *dst = (float *)(s_seed + buf * bufsz);
    const uint4 *src = a.img + ((size_t)b * nc + c0) * 256 + lane;
    for (uint32_t p = wave; p < kcs * 2u; p += 4u) glds16_asm(src + (p >> 1) * 256u + (p & 1u) * 64u, dst + p * 256u);
    if (!RESIDENT) {
      float *qdst = dst + kStreamChunks * 512u;
      for (uint32_t pi = wave; pi < kcs * 4u; pi += 4u) {
        const uint32_t piece = pi >> 1, qh = pi & 1u, c = piece >> 1, hh = piece & 1u;
        const uint32_t q = min(q0 + 64u * qh + (uint32_t)lane, a.nq - 1u);
        glds16_asm(a.qimg + (size_t)q * 4 * nc + 2 * (c0 + c) + hh, qdst + (piece * 128u + 64u * qh) * 4u);
      }
    }
  };
  // the slots of block b that take part: records (no pad slot) the filter admits; wave-uniform, two scalar loads
  auto live_slots = [&](uint32_t b) -> uint64_t {
    const uint32_t nrec = a.block_cnt[b];
    const uint64_t rec = nrec >= 64u ? ~0ull : (1ull << nrec) - 1ull;
    return a.allow ? (a.allow[b] & rec) : rec;
  };

  f32x16 acc0, acc1;  // vectors 0..31 and 32..63 of the block's image x this wave's 32 queries
  uint32_t nsurv = 0;

  // ---- epilogue of one accumulator tile: register r of tile t in lane half h is vector 32 t + 16 h + r of the block ----
  auto epilogue = [&](const f32x16 &acc, uint32_t t, uint32_t b, uint64_t live) {
    uint32_t m = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) m |= (!(acc[r] > thr) ? 1u : 0u) << r;
    m &= (uint32_t)(live >> (32u * t + 16u * (uint32_t)h)) & 0xFFFFu;  // pad slots and filtered slots leave here
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
    // ---- the drain: 64 entries a round, each evaluated in the chain; the key of a score that reaches t_q is kept ----
    for (uint32_t at = 0; at < n; at += kWave) {
      const uint32_t i = at + (uint32_t)lane;
      const uint32_t e = i < n ? s_queue[i] : 0u;
      const uint32_t q = w0 + (e & 31u), v = e >> 5;
      if (i < n && q < a.nq) {
        const float s = ip_scalar(a.Q + (size_t)q * a.dim, a.blocks + (size_t)b * a.dq * kWave + v, a.dim);
        if (s >= a.tq[q]) {
          const uint32_t pos = atomicAdd(a.cnt + q, 1u);
          if (pos < a.cap) a.keys[(size_t)q * a.cap + pos] = (uint32_t)(ip_key(s, 0u) >> 32);  // (nothing past the array)
        }
      }
    }
    wave_lds_sync();  // the queue is free again
  };

  stage(0, 0);
  uint64_t live = live_slots(a.stride * split), live_next = 0ull;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (uint32_t step = 0; step < nsteps; ++step) {
    const uint32_t cur = step & 1u;
    const uint32_t b = a.stride * (split + (step / nslab) * a.nsplit), s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    // the next step lands in the other buffer under this step's MFMAs (every wave left it at the last barrier); where
    // it begins a block, that block's live word comes with it
    if (step + 1 < nsteps) {
      stage(step + 1, cur ^ 1u);
      if (s + 1 == nslab) live_next = live_slots(b + a.stride * a.nsplit);
    }
    if (wave_live) {
      const uint4 *s_a = s_seed + cur * bufsz;
      if (s == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
      }
      if (RESIDENT) {
#pragma unroll
        for (uint32_t c = 0; c < kMaxChunks; ++c)
          if (c < nc) {
            const bf16x8 h0 = __builtin_bit_cast(bf16x8, s_a[(c * 2u + h) * 64u + j]);
            const bf16x8 h1 = __builtin_bit_cast(bf16x8, s_a[(c * 2u + h) * 64u + 32u + j]);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, bh[c], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, bh[c], acc1, 0, 0, 0);
          }
      } else {
        const uint4 *s_b = s_a + kStreamChunks * 128u;
        for (uint32_t c = 0; c < kcs; ++c) {
          const bf16x8 fh = __builtin_bit_cast(bf16x8, s_b[(c * 2u + h) * 128u + 32u * wave + j]);
          const bf16x8 h0 = __builtin_bit_cast(bf16x8, s_a[(c * 2u + h) * 64u + j]);
          const bf16x8 h1 = __builtin_bit_cast(bf16x8, s_a[(c * 2u + h) * 64u + 32u + j]);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, fh, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, fh, acc1, 0, 0, 0);
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
  if (lane == 0 && nsurv) atomicAdd(a.survivors, (unsigned long long)nsurv);
}

// ---- the k-th largest of a level's scores; one wave per query ----
struct IpTightenArgs {
  SelectCommon c;
  float vmax_raw;
  IpQueryTerms t;
  uint32_t *cnt, *ovf;
  const uint32_t *keys;
  unsigned long long *counters;  // the ladder's (kSeedCount...)
  uint32_t nq, k, cap, level;
};

// one wave: the k-th largest score among n >= k keys (a key orders scores descending: offered as -score, smallest first)
template <class Top>
__device__ __forceinline__ float kth_largest_score(const uint32_t *keys, uint32_t n, uint32_t k, int lane) {
  Top top;
  top.init();
  for (uint32_t at = 0; at < n; at += kWave) {
    const uint32_t i = at + (uint32_t)lane;
    float d = INFINITY;
    uint32_t pos = kNoPos;
    if (i < n) { d = -ip_key_score((uint64_t)keys[i] << 32); pos = i; }
    top.offer_bulk(d, pos, (int)k);
  }
  return -top.kth((int)k);
}

__global__ void __launch_bounds__(256) flat_ip_tighten_kernel(IpTightenArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (q >= a.nq) return;
  const uint32_t c = a.cnt[q];
  if (c == 0u) return;
  const uint32_t n = min(c, a.cap);
  float t = -INFINITY;
  if (n >= a.k) {
    const uint32_t *keys = a.keys + (size_t)q * a.cap;
    t = a.k <= 64u ? kth_largest_score<FastTopK>(keys, n, a.k, lane) : kth_largest_score<FastTop128>(keys, n, a.k, lane);
  }
  if (lane != 0) return;
  a.cnt[q] = 0u;  // (every lane read it above, in the same instruction)
  atomicAdd(a.counters + kSeedCountCandidates + a.level, (unsigned long long)c);
  if (c > a.cap) atomicAdd(a.counters + kSeedCountLevelOverflow, 1ull);
  const float old = a.t.tq[q];
  if (!(t > old)) return;  // fewer than k scores, or nothing gained: the bound stays
  QueryFrame f{};
  f.qn = a.t.qn[q];
  f.E = a.t.E[q];
  const float qm = a.t.qm[q];
  const float thr = ip_rank_threshold(a.c, f, qm, a.t.am[q], a.vmax_raw, t);
  if (!(fabsf(t) < 1.0e37f && fabsf(thr) < 1.0e37f)) return;  // (what flat_ip_prepare_kernel accepts as a bound)
  a.t.thr[q] = thr;
  a.t.tq[q] = t;
  a.t.sthr[q] = -2.0f * t + 2.0f * qm;
  a.ovf[q] = 0u;  // (a query without a bound until now has one)
  if (old == a.t.t0[q]) atomicAdd(a.counters + kSeedCountTightened, 1ull);
}

}  // namespace

IpSeedSchedule ip_seed_schedule(uint64_t nblocks, uint64_t cap, uint64_t k) {
  IpSeedSchedule s;
  uint64_t r = 2;
  while (r < 4 && 2 * r <= cap / (2 * std::max<uint64_t>(k, 1))) r *= 2;
  s.ratio = (uint32_t)r;
  if (nblocks * 64 <= cap) return s;
  uint32_t m = 1;
  uint64_t stride = r;
  while (stride < nblocks && (nblocks + stride - 1) / stride * 64 > cap) { stride *= r; ++m; }  // (cap < 64: one block)
  if (m > kIpSeedMaxLevels) { m = kIpSeedMaxLevels; stride = 1; for (uint32_t i = 0; i < m; ++i) stride *= r; }
  s.levels = m;
  for (uint32_t l = 0; l < m; ++l, stride /= r) s.strides[l] = (uint32_t)stride;
  return s;
}

vi_status ip_seed_ladder(const IpLadderArgs &a, const IpSeedSchedule &s, hipStream_t st) {
  const bool resident = a.c.dim <= kMaxChunks * 16u;
  const uint32_t ntiles = (a.nq + kTileQ - 1) / kTileQ;
  const int lds = (int)(seed_lds_words(resident, a.nc) * 16u);
  for (uint32_t l = 0; l < s.levels; ++l) {
    const uint32_t stride = s.strides[l], nsample = (a.nblocks + stride - 1) / stride;
    // three workgroups per CU at a time (144 VGPRs): two rounds of them where the sample has the blocks for it
    const uint32_t nsplit = exact_block_splits(6u, a.cus, ntiles, nsample);
    IpSeedArgs sa{a.img, a.qimg, a.c.blocks, a.c.Q, a.block_cnt, a.allow, a.t.sthr, a.t.tq, a.cnt, a.keys,
                  a.counters + kSeedCountSurvivors + l, a.nq, a.c.dim, a.c.dq, a.nc, nsample, stride, nsplit, a.cap};
    if (resident) hipLaunchKernelGGL(flat_ip_seed_kernel<true>, dim3(ntiles, nsplit), dim3(256), lds, st, sa);
    else hipLaunchKernelGGL(flat_ip_seed_kernel<false>, dim3(ntiles, nsplit), dim3(256), lds, st, sa);
    VI_HIP(hipGetLastError());
    IpTightenArgs ta{a.c, a.vmax_raw, a.t, a.cnt, a.ovf, a.keys, a.counters, a.nq, a.k, a.cap, l};
    hipLaunchKernelGGL(flat_ip_tighten_kernel, dim3((a.nq + 3) / 4), dim3(256), 0, st, ta);
    VI_HIP(hipGetLastError());
  }
  return VI_OK;
}

}  // namespace vi
