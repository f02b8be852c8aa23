// probe_prune.hip — adaptive probing: the device step that shortens every query's probe row by the rule of
// probe_rules.hpp, between a coarse step and a list phase.  One kernel, one wave per query, any row length.  Its three
// callers: the engines' pipelines (prune_staged_probes: the one-call entries vi_indexer_search_adaptive*), and the
// multi-GPU seam vi_indexer_prune_probes_device (device_index_prune_probes).  A pruned row is a row whose tail is the
// empty marker: what every list phase already accepts from a caller (adopt_probes).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "device_index.hpp"
#include "device_math.hpp"
#include "grouping.hpp"
#include "probe_rules.hpp"
#include "search_internal.hpp"

namespace vi {

namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kMaxPruneRow = 8192u * 32u;  // two words of LDS per 32 probes of a row: 64 KiB

// euclidean_distance_squared(q, centroid l) in the reference's order (device_math.hpp: sq_add, one chain from dimension 0
// up): the bits the coarse step sorted by.  The centroid is lane l % 64 of block l / 64 of the lane-interleaved table; the
// query row is the same for the whole wave, its loads are scalar.
__device__ __forceinline__ float centroid_distance(const float4 *__restrict__ cent, uint32_t dq, uint32_t dim,
                                                   const float *__restrict__ qv, uint32_t l) {
  const float4 *c = cent + (size_t)(l >> 6) * dq * kWave + (l & 63u);
  const uint32_t full = dim >> 2, rem = dim & 3u;
  float acc = 0.0f;
  for (uint32_t qd = 0; qd < full; ++qd) {
    const float4 v = c[(size_t)qd * kWave];
    sq_add(acc, qv[4 * qd], v.x);
    sq_add(acc, qv[4 * qd + 1], v.y);
    sq_add(acc, qv[4 * qd + 2], v.z);
    sq_add(acc, qv[4 * qd + 3], v.w);
  }
  if (rem) {  // (the table is padded to whole quads: quad `full` exists)
    const float4 v = c[(size_t)full * kWave];
    sq_add(acc, qv[4 * full], v.x);
    if (rem > 1) sq_add(acc, qv[4 * full + 1], v.y);
    if (rem > 2) sq_add(acc, qv[4 * full + 2], v.z);
  }
  return acc;
}

__device__ __forceinline__ uint32_t wave_inclusive_u32(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < kWave; o <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)v, o);
    if (lane >= o) v += up;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_inclusive_u64(uint64_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t o = 1; o < kWave; o <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o);
    if (lane >= o) v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_read_u64(uint64_t v, int lane) {
  return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), lane) << 32) | (uint32_t)__shfl((int)(uint32_t)v, lane);
}

struct ProbePruneArgs {
  const float *Q;             // nq x dim
  const float4 *cent;         // the coarse table, lane-interleaved blocks
  const uint32_t *list_len;   // full lengths (an unpartitioned index), read under max_codes only
  uint32_t dim, dq, nlists, P;
  uint32_t *probes, *order;   // nq x P each, rewritten in place
  ProbeRule rule;
  const uint32_t *limit;      // p_explicit per query, or null
  uint32_t *n_kept;           // p per query, or null
  uint32_t *counts;           // [2][nq]: found and p per query, for probe_totals_kernel
  uint32_t nq;
};

// One wave per query.  A lane owns a probe; rows longer than a wave go through 64 probes at a time with the counts
// carried.  Pass 1 counts (real probes, probes within the ratio, the first place where the budget is met), pass 2 marks
// the old ranks of the kept probes in a bitmap in LDS and scans its words, pass 3 rewrites the row.  A word that names no
// list counts as the marker (rows of the library's own never hold one; a caller's rows are validated first) and a rank
// outside the row marks nothing, so no word of a row can send an access outside the table or the bitmap.
__global__ void __launch_bounds__(64) probe_prune_kernel(ProbePruneArgs a) {
  extern __shared__ uint32_t prune_lds[];
  const uint32_t q = blockIdx.x, lane = threadIdx.x, P = a.P, words = (P + 31u) / 32u;
  uint32_t *seen = prune_lds, *before = prune_lds + words;
  uint32_t *row = a.probes + (size_t)q * P, *ord = a.order + (size_t)q * P;
  const float *__restrict__ qv = a.Q + (size_t)q * a.dim;
  const bool ratio_on = a.rule.ratio2 != 0.0f, codes_on = a.rule.max_codes != 0;
  for (uint32_t w = lane; w < words; w += kWave) seen[w] = 0u;

  uint32_t found = 0, n_ratio = 0, p_codes = 0;  // p_codes: 0 until the budget is met
  uint64_t codes = 0;
  float t = 0.0f;
  for (uint32_t r0 = 0; r0 < P; r0 += kWave) {
    const uint32_t r = r0 + lane;
    const uint32_t l = r < P ? row[r] : kProbeMarker;
    const bool real = l < a.nlists;
    const uint32_t lc = real ? l : 0u;
    found += (uint32_t)__popcll(__ballot(real));
    if (ratio_on) {
      float d = 0.0f;
      if (real) d = centroid_distance(a.cent, a.dq, a.dim, qv, l);  // (places past the row and markers gather nothing)
      if (r0 == 0) t = probe_threshold(a.rule.ratio2, __shfl(d, 0));  // (an empty row: no lane is real, t is not used)
      n_ratio += (uint32_t)__popcll(__ballot(real && probe_within_ratio(d, t)));
    }
    if (codes_on && p_codes == 0) {
      const uint64_t incl = codes + wave_inclusive_u64(real ? (uint64_t)a.list_len[lc] : 0ull, lane);
      const uint64_t met = __ballot(real && probe_budget_met(incl, a.rule.max_codes));
      if (met) p_codes = r0 + (uint32_t)__ffsll((unsigned long long)met);
      codes = wave_read_u64(incl, 63);
    }
  }
  const uint32_t p = probe_keep_count(found, ratio_on ? n_ratio : found, p_codes ? p_codes : found,
                                      a.limit ? a.limit[q] : kProbeNoLimit, a.rule.min_probe);
  __syncthreads();
  for (uint32_t r = lane; r < p; r += kWave) {
    const uint32_t g = ord[r];
    if (g < P) atomicOr(&seen[g >> 5], 1u << (g & 31u));
  }
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t w0 = 0; w0 < words; w0 += kWave) {
    const uint32_t w = w0 + lane;
    const uint32_t c = w < words ? (uint32_t)__popc(seen[w]) : 0u;
    const uint32_t incl = wave_inclusive_u32(c, lane);
    if (w < words) before[w] = run + incl - c;
    run += (uint32_t)__shfl((int)incl, 63);
  }
  __syncthreads();
  for (uint32_t r = lane; r < P; r += kWave) {
    const bool keep = r < p;
    const uint32_t l = row[r], g = ord[r];
    row[r] = keep ? l : kProbeMarker;
    ord[r] = keep ? probe_closed_rank(seen, before, g < P ? g : 0u) : kProbeMarker;
  }
  if (lane == 0) {
    if (a.n_kept) a.n_kept[q] = p;
    a.counts[q] = found;
    a.counts[a.nq + q] = p;
  }
}

// totals[0] = sum of found, totals[1] = sum of p over the batch: one workgroup.  (Not two atomics per query in the
// kernel above: every wave of the batch would queue at the same two addresses.)
__global__ void __launch_bounds__(1024) probe_totals_kernel(const uint32_t *counts, uint32_t nq, unsigned long long *totals) {
  __shared__ unsigned long long part[2][16];
  unsigned long long s[2] = {0ull, 0ull};
  for (uint32_t i = threadIdx.x; i < nq; i += 1024u) { s[0] += counts[i]; s[1] += counts[nq + i]; }
#pragma unroll
  for (int w = 0; w < 2; ++w) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
      s[w] += ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(s[w] >> 32), o) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)s[w], o);
    if ((threadIdx.x & 63u) == 0u) part[w][threadIdx.x >> 6] = s[w];
  }
  __syncthreads();
  if (threadIdx.x < 2u) {
    unsigned long long t = 0ull;
    for (int i = 0; i < 16; ++i) t += part[threadIdx.x][i];
    totals[threadIdx.x] = t;
  }
}

thread_local PruneStats t_last;

// the kernel over nq rows on st, and the two sums of its counts on their way to run.totals (read once st is synchronised)
vi_status launch_probe_prune(const DeviceIndex &ix, SearchWorkspace &ws, hipStream_t st, PruneRun &run, const float *Qd, uint64_t nq,
                             uint32_t P, uint32_t *probes, uint32_t *order, const uint32_t *limit_dev, uint32_t *n_kept_dev) {
  if (ix.order != VI_ORDER_SCALAR) return fail(VI_ERR_INVALID_INPUT, "adaptive probing needs an index of the scalar summation order");
  if (P > kMaxPruneRow) return fail(VI_ERR_INVALID_INPUT, "adaptive probing takes rows of at most %u probes", kMaxPruneRow);
  VI_TRY(ws.prune_totals.reserve(2));
  VI_TRY(ws.prune_counts.reserve(2 * nq));
  // (the sums land in page-locked memory: a copy into the caller's stack is staged by the runtime and stalls the queue)
  if (!ws.prune_pinned) VI_HIP(hipHostMalloc((void **)&ws.prune_pinned, 2 * sizeof(uint64_t)));
  ProbePruneArgs a{Qd, (const float4 *)ix.centroids.blocks.p, ix.list_len.p, ix.dim, ix.dq, (uint32_t)ix.nlists, P, probes, order,
                   ProbeRule{run.rule->min_probe, run.rule->ratio2, run.rule->max_codes}, limit_dev, n_kept_dev,
                   ws.prune_counts.p, (uint32_t)nq};
  run.pending = st;
  run.totals = ws.prune_pinned;
  VI_TRY(run.span.begin(0, st));
  hipLaunchKernelGGL(probe_prune_kernel, dim3((uint32_t)nq), dim3(kWave), 2u * ((P + 31u) / 32u) * sizeof(uint32_t), st, a);
  VI_HIP(hipGetLastError());
  VI_TRY(run.span.end(0, st));
  hipLaunchKernelGGL(probe_totals_kernel, dim3(1), dim3(1024), 0, st, ws.prune_counts.p, (uint32_t)nq,
                     (unsigned long long *)ws.prune_totals.p);
  VI_HIP(hipGetLastError());
  VI_HIP(hipMemcpyAsync(ws.prune_pinned, ws.prune_totals.p, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  return VI_OK;
}

}  // namespace

vi_status prune_begin(PruneRun &run, const ProbePrune *rule, bool host) {
  t_last = PruneStats{};
  run.rule = rule;
  run.host = host;
  const char *e = getenv("VI_PRUNE_TIMING");
  return run.span.create(e && *e && *e != '0');
}

// (the caller has synchronised the run's stream)
void prune_finish(PruneRun &run) {
  if (!run.pending) return;
  run.pending = nullptr;
  t_last.probes_in = run.totals[0];
  t_last.probes_kept = run.totals[1];
  t_last.ms_prune = run.span.ms(0);
}

PruneStats prune_last_stats() { return t_last; }
void prune_reset_stats() { t_last = PruneStats{}; }

// the engines' hook behind their coarse step: ws.probes / ws.gorder pruned in place; the per-list histogram of the coarse
// step counted again from the shortened rows (histogram); the pairs' ranks of the coarse select no longer stand
vi_status prune_staged_probes(SearchBatch &b, bool histogram) {
  if (!b.prune) return VI_OK;
  PruneRun &run = *b.prune;
  SearchWorkspace &ws = b.ws();
  const uint32_t *limit = run.rule->n_probe_q;
  uint32_t *kept = run.rule->n_kept;
  if (run.host) {
    if (limit) {
      VI_TRY(ws.prune_limit.reserve(b.nq));
      VI_HIP(hipMemcpyAsync(ws.prune_limit.p, limit, b.nq * sizeof(uint32_t), hipMemcpyHostToDevice, b.st()));
      limit = ws.prune_limit.p;
    }
    if (kept) {
      VI_TRY(ws.prune_kept.reserve(b.nq));
      kept = ws.prune_kept.p;
    }
  }
  VI_TRY(launch_probe_prune(b.ix, ws, b.st(), run, b.Qd, b.nq, b.P, ws.probes.p, ws.gorder.p, limit, kept));
  if (run.host && kept) VI_HIP(hipMemcpyAsync(run.rule->n_kept, kept, b.nq * sizeof(uint32_t), hipMemcpyDeviceToHost, b.st()));
  b.pair_rank_valid = false;
  if (histogram) VI_TRY(launch_probe_histogram(b.ix, ws, ws.probes.p, (uint32_t)(b.nq * b.P), b.P, b.st()));
  return VI_OK;
}

vi_status device_index_prune_probes(const DeviceIndex &ix, const float *Qd, uint64_t nq, uint32_t P, uint32_t *probes, uint32_t *order,
                                    const ProbePrune &rule) {
  PruneRun run;
  VI_TRY(prune_begin(run, &rule, false));
  if (nq == 0 || P == 0) return VI_OK;
  if (nq * (uint64_t)P > 0x7FFFFFFFull) return fail(VI_ERR_INVALID_INPUT, "batch too large: split nq");
  VI_HIP(hipSetDevice(ix.device));
  // (a context of the searches' pool for its stream and workspace; no search ran: the handle's search stats stay)
  ContextLease lease(ix.search_contexts, make_context<SearchContext>, [] {});
  if (!lease.ctx) return VI_ERR_DEVICE;  // (the message is make_context's)
  SearchContext &ctx = *lease.ctx;
  VI_TRY(validate_probe_rows(ix, ctx.ws, probes, order, nq, P, ctx.stream));
  VI_TRY(launch_probe_prune(ix, ctx.ws, ctx.stream, run, Qd, nq, P, probes, order, rule.n_probe_q, rule.n_kept));
  VI_HIP(hipStreamSynchronize(ctx.stream));
  prune_finish(run);
  return VI_OK;
}

}  // namespace vi
