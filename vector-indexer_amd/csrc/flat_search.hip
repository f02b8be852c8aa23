// flat_search.hip — exact (flat) k-NN over every resident record: one dense sweep of ALL blocks against ALL queries on the
// matrix cores (the contract is vi_indexer_search_exact in include/vi_amd.h).
//
//   1. seed     an ordinary top-k search at seed_probe: the distance d_k of a query's k-th hit bounds its true k-th key
//               from above (any k admitted records do), B_q = (d_k, every ordinal).  flat_prepare_kernel turns it into the
//               rank threshold of DESIGN §2b in the query's frame (query_frame, rank_threshold: the selects' own) and
//               splits the batch into its bf16 image.  A query without k hits, or one whose magnitude the rank
//               arithmetic cannot be trusted with, is flagged for step 4 and skipped by the sweep.
//   2. sweep    flat_sweep_kernel: a workgroup owns 128 queries and a strided share of all blocks in storage order; per
//               64-vector block it accumulates ||v||^2 - 2 q.v with v_mfma_f32_32x32x16_bf16 (hi.hi + hi.lo + lo.hi;
//               lo.hi dropped where every stored value is bf16-exact), compares the 32 values a lane holds with its
//               query's threshold and ballots.  No survivor — the common case — falls through to the next block.
//               Survivors are compacted per wave, the admitted ones evaluated exactly in the reference's chain from the f32
//               blocks, and those at or under the bound appended to the query's candidates with one atomicAdd.
//   3. finish   flat_finish_kernel: one wave per query sorts its candidates in LDS, cuts at k, resolves ordinals to ids.
//   4. overflow flat_keys_kernel writes the exact key of every admitted record for each flagged query, sort_rows_u64 sorts
//               the rows, flat_take_kernel cuts at k.  Slow and always right.
// The seed's own hits are not copied into the candidates: they lie under the bound, so the sweep meets them like any
// other record and nothing can be appended twice.  No result depends on a rank value.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "device_index.hpp"
#include "flat_common.hpp"
#include "flat_search.hpp"
#include "mfma_bf16.hpp"
#include "record_fetch.hpp"
#include "search_internal.hpp"
#include "select_device.hpp"
#include "slot_filter.hpp"

namespace vi {
namespace {

constexpr uint32_t kTileQ = 128;       // queries per workgroup: four waves of one 32-column B tile each
constexpr uint32_t kStreamChunks = 2;  // D > 128: chunks of 16 dimensions per K step (both operands stream through LDS)
constexpr uint32_t kQueueLen = 2048;   // survivors of one wave and block: 32 queries x 64 vectors, never more
constexpr uint64_t kNoKey = ~0ull;
constexpr uint64_t kOverflowKeys = 1ull << 25;  // keys of one chunk of overflow rows (256 MB)

enum { kCountSurvivors = 0, kCountCandidates = 1, kCounters = 2 };

__global__ void flat_clear_kernel(uint32_t *cnt, uint32_t *ovf, uint32_t nq) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < nq) { cnt[q] = 0u; ovf[q] = 0u; }
}

// ---- step 1: bound, threshold and image of every query; one wave per query ----
struct PrepareArgs {
  SelectCommon c;
  const float *seed_D;
  uint32_t nq, k, nc;
  float *thr;
  uint64_t *bound;
  uint32_t *cnt, *ovf;
  uint4 *qimg;  // [query][plane hi / lo][chunk][half] x 16 B of -2 (q - mu): the layout every rank kernel reads
  unsigned long long *counters;
};

__global__ void __launch_bounds__(256) flat_prepare_kernel(PrepareArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const uint32_t q = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (blockIdx.x == 0 && threadIdx.x < kCounters) a.counters[threadIdx.x] = 0ull;
  if (q >= a.nq) return;
  const QueryFrame f = query_frame<false>(a.c, q, lane, nullptr, nullptr);
  float d = 0.0f;  // the seed's largest distance; +inf where it found fewer than k
  for (uint32_t i = lane; i < a.k; i += kWave) d = fmaxf(d, a.seed_D[(size_t)q * a.k + i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) d = fmaxf(d, __shfl_xor(d, o));
  const bool bounded = !f.distrust && d < 1.0e37f;
  // a record with reference distance <= d has a true rank value <= d - qn up to the rounding of the reference's own
  // sum (w, as the radius select forms it); rank_threshold adds the rank arithmetic's margins
  const float w = ((float)(a.c.dim >> 6) + 9.0f) * 6.1e-8f * (fabsf(d) + f.qn);
  const float thr = bounded ? rank_threshold(a.c, f, (d - f.qn) + w) : -INFINITY;
  if (lane == 0) {
    const bool ok = bounded && thr < INFINITY;
    a.thr[q] = ok ? thr : -INFINITY;
    a.bound[q] = ok ? (((uint64_t)__float_as_uint(d) << 32) | 0xFFFFFFFFull) : kNoKey;
    a.cnt[q] = 0u;
    a.ovf[q] = ok ? 0u : 1u;
  }
  split_query_image(a.c, q, a.nc, lane, a.qimg);
}

// ---- step 2: the sweep ----
struct SweepArgs {
  const uint4 *img;     // the lists' bf16 image: [block][chunk][plane][half][64 columns] x 16 B (rank_images.hip)
  const float *xnorm;   // squared norms in image-column order, kBig on pad slots and on slots a filter excludes
  const uint4 *qimg;
  const float4 *blocks;
  const float *Q;
  const uint32_t *block_ord, *block_cnt;
  const uint64_t *allow;  // one allow word per block, or null
  const float *thr;
  const uint64_t *bound;
  uint32_t *cnt, *ovf;
  uint64_t *cand;         // [nq][cap]
  unsigned long long *counters;
  uint32_t nq, dim, dq, nc, nblocks, nsplit, cap;
  uint32_t lo_planes;     // the lists' lo planes are multiplied (some stored value is not bf16-exact)
};

// LDS, in 16-byte words: two K-step buffers, (RESIDENT) the tile's whole query image, the norms of two blocks, the waves'
// survivor queues.  A K step holds `kc` chunks of a block's image — all of them when RESIDENT — and, when the queries
// stream, the same chunks of the tile's 128 queries behind them.
__host__ __device__ inline uint32_t flat_step_words(bool resident, uint32_t nc) {
  return resident ? nc * 256u : kStreamChunks * (256u + 512u);
}
__host__ __device__ inline uint32_t flat_lds_words(bool resident, uint32_t nc) {
  return 2u * flat_step_words(resident, nc) + (resident ? nc * 512u : 0u) + 32u + 4u * kQueueLen * 2u / 16u;
}

template <bool RESIDENT>
__global__ void __launch_bounds__(256, 1) flat_sweep_kernel(SweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 s_flat[];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const int j = lane & 31, h = lane >> 5;
  const uint32_t nc = a.nc, kc = RESIDENT ? nc : kStreamChunks, nslab = (nc + kc - 1) / kc;
  const uint32_t bufsz = flat_step_words(RESIDENT, nc);
  uint4 *s_query = s_flat + 2 * bufsz;                                   // RESIDENT only
  float *s_norm = (float *)(s_query + (RESIDENT ? nc * 512u : 0u));      // [2][64]
  uint16_t *s_queue = (uint16_t *)(s_norm + 128) + (uint32_t)wave * kQueueLen;
  const uint32_t q0 = blockIdx.x * kTileQ, split = blockIdx.y;
  if (split >= a.nblocks) return;  // (the host launches nsplit <= nblocks)
  const uint32_t nmine = (a.nblocks - split + a.nsplit - 1) / a.nsplit, nsteps = nmine * nslab;

  const uint32_t qg = q0 + 32u * (uint32_t)wave + (uint32_t)j;  // this lane's query: both lane halves hold column j
  const float thr = qg < a.nq ? a.thr[qg] : -INFINITY;          // (-inf: no query, or one the overflow path answers)
  const bool wave_live = __ballot(thr > -INFINITY) != 0ull;

  // chunks [c0, c0 + kcs) of the tile's query image -> dst: piece (chunk, plane, half) of 128 queries = 2 KB, lane = query
  auto stage_queries = [&](float *dst, uint32_t c0, uint32_t kcs) {
    for (uint32_t pi = wave; pi < kcs * 8u; pi += 4u) {
      const uint32_t piece = pi >> 1, qh = pi & 1u, c = piece >> 2, pc = piece & 3u;
      const uint32_t q = min(q0 + 64u * qh + (uint32_t)lane, a.nq - 1u);  // (a tile's tail repeats the last query)
      glds16_asm(a.qimg + (size_t)q * 4 * nc + (pc >> 1) * 2 * nc + 2 * (c0 + c) + (pc & 1u), dst + (piece * 128u + 64u * qh) * 4u);
    }
  };
  // K step `step` of this workgroup -> buffer `buf`
  auto stage = [&](uint32_t step, uint32_t buf) {
    const uint32_t b = split + (step / nslab) * a.nsplit, s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    float *dst = (float *)(s_flat + buf * bufsz);
    const uint4 *src = a.img + ((size_t)b * nc + c0) * 256 + lane;
    for (uint32_t p = wave; p < kcs * 4u; p += 4u) glds16_asm(src + p * 64u, dst + p * 256u);
    if (!RESIDENT) stage_queries(dst + kStreamChunks * 1024u, c0, kcs);
    if (s == 0 && wave == 0) glds4_asm(a.xnorm + (size_t)b * kWave + lane, s_norm + buf * 64u);
  };

  stage(0, 0);
  if (RESIDENT) stage_queries((float *)s_query, 0, nc);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  f32x16 acc0, acc1;  // rows 0..31 and 32..63 of the block's image x this wave's 32 queries
  uint32_t nsurv = 0;
  for (uint32_t step = 0; step < nsteps; ++step) {
    const uint32_t cur = step & 1u;
    const uint32_t b = split + (step / nslab) * a.nsplit, s = step % nslab, c0 = s * kc, kcs = min(kc, nc - c0);
    // the next step lands in the other buffer under this step's MFMAs (every wave left it at the last barrier)
    if (step + 1 < nsteps) stage(step + 1, cur ^ 1u);
    if (wave_live) {
      const uint4 *s_a = s_flat + cur * bufsz;
      const uint4 *s_b = RESIDENT ? s_query : s_a + kStreamChunks * 256u;
      if (s == 0) {
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {  // rows 8 q4 + 4 h + (0..3) of a tile live in registers 4 q4 .. 4 q4 + 3
          const float4 n0 = *reinterpret_cast<const float4 *>(s_norm + cur * 64u + 8 * q4 + 4 * h);
          const float4 n1 = *reinterpret_cast<const float4 *>(s_norm + cur * 64u + 32 + 8 * q4 + 4 * h);
          acc0[4 * q4 + 0] = n0.x; acc0[4 * q4 + 1] = n0.y; acc0[4 * q4 + 2] = n0.z; acc0[4 * q4 + 3] = n0.w;
          acc1[4 * q4 + 0] = n1.x; acc1[4 * q4 + 1] = n1.y; acc1[4 * q4 + 2] = n1.z; acc1[4 * q4 + 3] = n1.w;
        }
      }
      for (uint32_t c = 0; c < kcs; ++c) {
        const uint32_t cb = RESIDENT ? c0 + c : c;  // the chunk's place in the query image that is in LDS
        const bf16x8 bh = __builtin_bit_cast(bf16x8, s_b[(cb * 4u + 0u + h) * 128u + 32u * wave + j]);
        const bf16x8 bl = __builtin_bit_cast(bf16x8, s_b[(cb * 4u + 2u + h) * 128u + 32u * wave + j]);
        const bf16x8 h0 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 0u + h) * 64u + j]);
        const bf16x8 h1 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 0u + h) * 64u + 32u + j]);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, bh, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, bh, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h0, bl, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(h1, bl, acc1, 0, 0, 0);
        if (a.lo_planes) {
          const bf16x8 l0 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 2u + h) * 64u + j]);
          const bf16x8 l1 = __builtin_bit_cast(bf16x8, s_a[(c * 4u + 2u + h) * 64u + 32u + j]);
          acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(l0, bh, acc0, 0, 0, 0);
          acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(l1, bh, acc1, 0, 0, 0);
        }
      }
      if (s + 1 == nslab) {
        // ---- epilogue: register r of tile t in lane half h is vector 32 t + 16 h + r of the block (image_column) ----
        uint32_t m = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          m |= (acc0[r] <= thr ? 1u : 0u) << r;
          m |= (acc1[r] <= thr ? 1u : 0u) << (16 + r);
        }
        if (__ballot(m != 0u) != 0ull) {
          uint32_t n = 0;  // survivors (query of the wave | vector << 5), compacted into the wave's queue
          for (uint32_t bit = 0; bit < 32u; ++bit) {
            const bool sv = (m >> bit) & 1u;
            const uint64_t bal = __ballot(sv);
            if (!bal) continue;
            if (sv) s_queue[n + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] =
                        (uint16_t)((uint32_t)j | ((32u * (bit >> 4) + 16u * (uint32_t)h + (bit & 15u)) << 5));
            n += (uint32_t)__popcll(bal);
          }
          wave_lds_sync();
          nsurv += n;
          const uint32_t nrec = a.block_cnt[b], ord0 = a.block_ord[b];
          const uint64_t allow = a.allow ? a.allow[b] : ~0ull;
          for (uint32_t at = 0; at < n; at += kWave) {
            const uint32_t i = at + (uint32_t)lane;
            const uint32_t e = i < n ? s_queue[i] : 0u;
            const uint32_t q = q0 + 32u * (uint32_t)wave + (e & 31u), v = e >> 5;
            // admitted: a record (no pad slot) that the filter lets through
            if (i < n && q < a.nq && v < nrec && ((allow >> v) & 1ull)) {
              const float d = exact_scalar(a.Q + (size_t)q * a.dim, a.blocks + (size_t)b * a.dq * kWave + v, a.dim);
              const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (ord0 + v);
              if (key <= a.bound[q]) {
                const uint32_t pos = atomicAdd(a.cnt + q, 1u);
                if (pos < a.cap) a.cand[(size_t)q * a.cap + pos] = key;  // (nothing is written past the array)
                else a.ovf[q] = 1u;
              }
            }
          }
          wave_lds_sync();  // the queue is free again
        }
      }
    }
    // the next step has landed (this wave's loads, stores and atomics too), every wave is done with this buffer
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }
  if (lane == 0 && nsurv) atomicAdd(a.counters + kCountSurvivors, (unsigned long long)nsurv);
}

// ---- steps 3 and 4: sorted keys -> the rows of the caller ----
struct OutArgs {
  const uint32_t *block_ord;
  const uint64_t *ext_ids;
  uint32_t nblocks, k;
  float *D;
  int64_t *I;
  uint64_t *ord, *counts;  // or null
};

// one wave: row q of the outputs from `navail` ascending keys (kNoKey: none from there on)
__device__ __forceinline__ void emit_row(const OutArgs &o, uint32_t q, const uint64_t *keys, uint32_t navail, int lane) {
  uint32_t found = 0;
  for (uint32_t i = lane; i < o.k; i += kWave) {
    const uint64_t key = i < navail ? keys[i] : kNoKey;
    const size_t at = (size_t)q * o.k + i;
    if (key == kNoKey) {
      o.D[at] = INFINITY; o.I[at] = -1;
      if (o.ord) o.ord[at] = kNoKey;
      continue;
    }
    ++found;
    const uint32_t ordinal = (uint32_t)key;
    const uint32_t lo = block_of_ordinal(o.block_ord, o.nblocks, ordinal);
    o.D[at] = __uint_as_float((uint32_t)(key >> 32));
    o.I[at] = (int64_t)o.ext_ids[(size_t)lo * kWave + (ordinal - o.block_ord[lo])];
    if (o.ord) o.ord[at] = ordinal;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) found += (uint32_t)__shfl_xor((int)found, s);
  if (o.counts && lane == 0) o.counts[q] = found;
}

// one wave per query: its candidates sorted in LDS (a bitonic network over the next power of two), cut at k
__global__ void __launch_bounds__(64) flat_finish_kernel(OutArgs o, const uint64_t *cand, const uint32_t *cnt, const uint32_t *ovf,
                                                         uint32_t cap, unsigned long long *counters) {
  extern __shared__ __attribute__((aligned(16))) uint64_t s_keys[];
  const int lane = threadIdx.x;
  const uint32_t q = blockIdx.x;
  if (ovf[q]) return;  // (step 4 writes the row)
  const uint32_t n = min(cnt[q], cap);
  uint32_t P = kWave;
  while (P < n) P <<= 1;
  for (uint32_t i = lane; i < P; i += kWave) s_keys[i] = i < n ? cand[(size_t)q * cap + i] : kNoKey;
  wave_lds_sync();
  for (uint32_t k2 = 2; k2 <= P; k2 <<= 1)
    for (uint32_t j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      for (uint32_t t = lane; t < P / 2; t += kWave) {
        const uint32_t i = ((t & ~(j2 - 1u)) << 1) | (t & (j2 - 1u));
        const uint64_t x = s_keys[i], y = s_keys[i + j2];
        if ((x > y) == ((i & k2) == 0u)) { s_keys[i] = y; s_keys[i + j2] = x; }
      }
      wave_lds_sync();
    }
  emit_row(o, q, s_keys, P, lane);
  if (lane == 0 && n) atomicAdd(counters + kCountCandidates, (unsigned long long)n);
}

// row r of `keys` (2^logL each): the exact key of every record query rows[r] is offered, kNoKey on every other place
__global__ void __launch_bounds__(256) flat_keys_kernel(SweepArgs a, const uint32_t *rows, uint32_t logL, uint64_t *keys) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x, q = rows[blockIdx.y];
  if (i >= (1u << logL)) return;
  uint64_t key = kNoKey;
  const uint32_t b = i >> 6, v = i & 63u;
  if (b < a.nblocks && v < a.block_cnt[b] && (!a.allow || ((a.allow[b] >> v) & 1ull))) {
    const float d = exact_scalar(a.Q + (size_t)q * a.dim, a.blocks + (size_t)b * a.dq * kWave + v, a.dim);
    key = ((uint64_t)__float_as_uint(d) << 32) | (a.block_ord[b] + v);
  }
  keys[((size_t)blockIdx.y << logL) + i] = key;
}

__global__ void __launch_bounds__(64) flat_take_kernel(OutArgs o, const uint64_t *keys, uint32_t logL, const uint32_t *rows) {
  emit_row(o, rows[blockIdx.x], keys + ((size_t)blockIdx.x << logL), 1u << logL, (int)threadIdx.x);
}

thread_local vi_exact_stats g_last_stats{};

vi_status exact_in_context(const DeviceIndex &ix, SearchContext &ctx, const ExactIO &io) {
  SearchWorkspace &ws = ctx.ws;
  auto &fw = ws.flat;
  hipStream_t st = ctx.stream;
  const uint64_t nq = io.nq, k = io.k;
  const uint32_t dim = ix.dim, nc = ix.dq / 4, nblocks = (uint32_t)ix.lists.nblocks;
  const char *te = getenv("VI_EXACT_TIMING");
  const bool timing = te && *te != '0';
  vi_exact_stats es{};
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
  OutArgs o{nullptr, ix.ext_ids.p, nblocks, (uint32_t)k, io.D, io.I, io.ord, io.counts};
  if (!io.on_device) {
    VI_TRY(fw.D.reserve(nq * k));
    VI_TRY(fw.I.reserve(nq * k));
    o.D = fw.D.p; o.I = fw.I.p;
    if (io.ord) { VI_TRY(fw.ord.reserve(nq * k)); o.ord = fw.ord.p; }
    if (io.counts) { VI_TRY(fw.counts.reserve(nq)); o.counts = fw.counts.p; }
  }
  VI_TRY(fw.cnt.reserve(nq));
  VI_TRY(fw.ovf.reserve(nq));
  VI_TRY(fw.cand.reserve(nq * cap));
  VI_TRY(fw.counters.reserve(kCounters));
  const dim3 per_query((uint32_t)((nq + 255) / 256)), per_wave((uint32_t)((nq + 3) / 4));
  std::vector<uint32_t> h_ovf(nq, 0u);

  const bool empty = ix.nlists == 0 || ix.nvec_resident == 0 || nblocks == 0;
  double t2 = t0;  // where the finish begins
  if (empty) {  // nothing is resident: every row is padding
    hipLaunchKernelGGL(flat_clear_kernel, per_query, dim3(256), 0, st, fw.cnt.p, fw.ovf.p, (uint32_t)nq);
    VI_HIP(hipMemsetAsync(fw.counters.p, 0, kCounters * sizeof(unsigned long long), st));
  } else {
    // ---- 1. seed ----
    VI_TRY(fw.seed_D.reserve(nq * k));
    VI_TRY(fw.seed_I.reserve(nq * k));
    SearchIO sio;
    sio.queries = Qd; sio.on_device = true; sio.nq = nq; sio.k = k; sio.n_probe = es.seed_probe;
    sio.D = fw.seed_D.p; sio.I = fw.seed_I.p; sio.filter = io.filter;
    VI_TRY(topk_search(ix, ctx, sio));  // (synchronised)
    es.ms_seed = timing ? (float)(now_ms() - t0) : 0.0f;
    const double t1 = now_ms();

    // ---- 2. bounds, images, sweep ----
    VI_TRY(ensure_fetch_layout(ix, st));
    VI_TRY(fw.block_ord.reserve(nblocks));
    VI_TRY(fw.block_cnt.reserve(nblocks));
    VI_TRY(fw.thr.reserve(nq));
    VI_TRY(fw.bound.reserve(nq));
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
    PrepareArgs pa{c, fw.seed_D.p, (uint32_t)nq, (uint32_t)k, nc, fw.thr.p, fw.bound.p, fw.cnt.p, fw.ovf.p, (uint4 *)fw.qimg.p, fw.counters.p};
    hipLaunchKernelGGL(flat_prepare_kernel, per_wave, dim3(256), 0, st, pa);
    VI_HIP(hipGetLastError());

    int cus = 0;
    VI_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix.device));
    const uint32_t ntiles = (uint32_t)((nq + kTileQ - 1) / kTileQ);
    // one workgroup per CU at a time (LDS): two rounds of them, so that the tail of the grid is short
    const uint32_t nsplit = exact_block_splits(2u, cus, ntiles, nblocks);
    es.block_splits = nsplit;
    SweepArgs sa{(const uint4 *)ix.lists_bf16.p, io.filter ? io.filter->xnorm_img.p : ix.xnorm_img.p, (const uint4 *)fw.qimg.p,
                 (const float4 *)ix.lists.blocks.p, Qd, fw.block_ord.p, fw.block_cnt.p, io.filter ? io.filter->allow.p : nullptr,
                 fw.thr.p, fw.bound.p, fw.cnt.p, fw.ovf.p, fw.cand.p, fw.counters.p,
                 (uint32_t)nq, dim, ix.dq, nc, nblocks, nsplit, cap, ix.lists_lo_zero ? 0u : 1u};
    const bool resident = dim <= kNarrowDim;
    const int lds = (int)(flat_lds_words(resident, nc) * 16u);
    const void *fn = resident ? (const void *)flat_sweep_kernel<true> : (const void *)flat_sweep_kernel<false>;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
      return fail(VI_ERR_DEVICE, "cannot reserve %d bytes of LDS for the exact search's sweep", lds);
    if (resident) hipLaunchKernelGGL(flat_sweep_kernel<true>, dim3(ntiles, nsplit), dim3(256), lds, st, sa);
    else hipLaunchKernelGGL(flat_sweep_kernel<false>, dim3(ntiles, nsplit), dim3(256), lds, st, sa);
    VI_HIP(hipGetLastError());
    if (timing) {
      VI_HIP(hipStreamSynchronize(st));
      es.ms_sweep = (float)(now_ms() - t1);
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
        hipLaunchKernelGGL(flat_keys_kernel, dim3((1u << logL) / 256u, m), dim3(256), 0, st, sa, fw.rows.p + r0, logL, fw.keys.p);
        VI_HIP(hipGetLastError());
        VI_TRY(sort_rows_u64(fw.keys.p, m, logL, st));
        hipLaunchKernelGGL(flat_take_kernel, dim3(m), dim3(64), 0, st, o, (const uint64_t *)fw.keys.p, logL, fw.rows.p + r0);
        VI_HIP(hipGetLastError());
      }
      VI_HIP(hipStreamSynchronize(st));  // (`rows` is read by its upload until here)
    }
  }

  // ---- 3. finish ----
  uint32_t p2 = kWave;
  while (p2 < cap) p2 <<= 1;
  const int lds_finish = (int)(p2 * sizeof(uint64_t));
  if (hipFuncSetAttribute((const void *)flat_finish_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_finish) != hipSuccess)
    return fail(VI_ERR_DEVICE, "cannot reserve %d bytes of LDS for the exact search's sort", lds_finish);
  hipLaunchKernelGGL(flat_finish_kernel, dim3((uint32_t)nq), dim3(64), lds_finish, st, o, (const uint64_t *)fw.cand.p, fw.cnt.p, fw.ovf.p, cap, fw.counters.p);
  VI_HIP(hipGetLastError());
  unsigned long long h_count[kCounters] = {};
  VI_HIP(hipMemcpyAsync(h_count, fw.counters.p, sizeof(h_count), hipMemcpyDeviceToHost, st));
  if (!io.on_device) {
    VI_HIP(hipMemcpyAsync(io.D, o.D, nq * k * sizeof(float), hipMemcpyDeviceToHost, st));
    VI_HIP(hipMemcpyAsync(io.I, o.I, nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    if (io.ord) VI_HIP(hipMemcpyAsync(io.ord, o.ord, nq * k * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (io.counts) VI_HIP(hipMemcpyAsync(io.counts, o.counts, nq * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  }
  VI_HIP(hipStreamSynchronize(st));
  es.survivors = h_count[kCountSurvivors];
  es.candidates = h_count[kCountCandidates];
  const double t3 = now_ms();
  es.ms_finish = timing ? (float)(t3 - t2) : 0.0f;
  es.ms_total = timing ? (float)(t3 - t0) : 0.0f;
  g_last_stats = es;
  return VI_OK;
}

}  // namespace

vi_exact_stats exact_last_stats() { return g_last_stats; }

vi_status device_index_search_exact(const DeviceIndex &ix, const ExactIO &io) {
  g_last_stats = vi_exact_stats{};
  if (io.nq == 0) return VI_OK;
  if (ix.stripe_world > 1) return fail(VI_ERR_INVALID_INPUT, "exact search needs the whole index on one handle");
  if (ix.order != VI_ORDER_SCALAR) return fail(VI_ERR_INVALID_INPUT, "exact search needs an index whose distances are VI_ORDER_SCALAR");
  if (ix.dim < 4 || (ix.dim & 3) || ix.dim > kMaxMfmaDim)
    return fail(VI_ERR_INVALID_INPUT, "exact search needs a dimension that is a multiple of 4 and at most %u, not %u", kMaxMfmaDim, ix.dim);
  if (ix.lists.nblocks * 64ull >= (1ull << kPosBits))
    return fail(VI_ERR_INVALID_INPUT, "exact search needs an index of fewer than 2^%u slots", kPosBits);
  if (ix.nvec_resident >= (1ull << 32)) return fail(VI_ERR_INVALID_INPUT, "ordinals must fit 32 bits");  // (implied by the slot limit)
  if (!(ix.xmax2 < 1.0e30f)) return fail(VI_ERR_INVALID_INPUT, "exact search needs stored vectors of squared norm below 1e30");
  if (ix.lists.nblocks && (!ix.ext_ids.p || !ix.lists_bf16.p)) return fail(VI_ERR_INVALID_INPUT, "this index keeps no external ids or ranking images");
  if (io.filter && io.filter->owner_serial != ix.serial) return fail(VI_ERR_INVALID_INPUT, "the filter was made for another index");
  const vi_status s = with_search_context(ix, [&](SearchContext &ctx) { return exact_in_context(ix, ctx, io); });
  if (s != VI_OK) (void)hipGetLastError();  // (a failed allocation is this call's failure, not the next call's)
  return s;
}

}  // namespace vi
