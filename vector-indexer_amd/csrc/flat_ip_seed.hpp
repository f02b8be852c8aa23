// flat_ip_seed.hpp — the score-seeded ladder in front of the exact inner-product search's final sweep (flat_ip_seed.hip;
// DESIGN.md §4x).  flat_ip.hip prepares every query (bound from the L2 seed, frame terms, image), calls ip_seed_ladder,
// and sweeps with the thresholds the ladder left.  The ladder only ever raises a bound, so it never changes a result.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "select_device.hpp"

namespace vi {

constexpr uint32_t kIpSeedMaxLevels = 8;  // (strides[] of vi_exact_ip_seed_stats)

// the ladder's counters, behind the final sweep's own in one array that flat_ip_prepare_kernel clears
enum {
  kSeedCountSurvivors = 0,                       // [level] pairs evaluated in the chain
  kSeedCountCandidates = kIpSeedMaxLevels,       // [level] those with s >= t_q
  kSeedCountTightened = 2 * kIpSeedMaxLevels,    // rows whose t_q some level raised
  kSeedCountLevelOverflow,                       // (row, level) pairs that collected more than cand_cap scores
  kIpSeedCounters
};

// Per query, what flat_ip_prepare_kernel computes once and flat_ip_tighten_kernel reads at every level: [nq] floats each.
//   thr   the sound rank threshold of the final sweep (-inf: the overflow path answers the query)
//   tq    the score a candidate must reach
//   sthr  the margin-free threshold -2 t_q + 2 q.mu of the sampled levels: +inf while the query has no bound yet,
//         -inf for a query no level may bound (distrusted magnitude)
//   t0    the L2 seed's t_q (a row counts as tightened the first time it leaves it)
//   qn, E the QueryFrame terms; qm, am  q.mu and sum |q_i mu_i| (ip_centre_terms)
struct IpQueryTerms {
  float *thr, *tq, *sthr, *t0, *qn, *E, *qm, *am;
  static constexpr uint32_t kArrays = 8;
  static IpQueryTerms at(float *base, uint64_t nq) {
    return IpQueryTerms{base, base + nq, base + 2 * nq, base + 3 * nq, base + 4 * nq, base + 5 * nq, base + 6 * nq, base + 7 * nq};
  }
};

// The schedule.  ratio r: the largest power of two <= cap / (2 k), clamped to [2, 4].  Strides r^m > ... > r, coarsest
// first: m is the smallest with ceil(nblocks / r^m) * 64 <= cap (or one block, where cap < 64); no level where nblocks * 64 <= cap; never more than
// kIpSeedMaxLevels — a longer ladder loses its coarsest levels.
struct IpSeedSchedule {
  uint32_t ratio = 0, levels = 0;
  uint32_t strides[kIpSeedMaxLevels] = {};
};
IpSeedSchedule ip_seed_schedule(uint64_t nblocks, uint64_t cap, uint64_t k);

struct IpLadderArgs {
  SelectCommon c;         // the frame of the block images (Q, dim, dq, blocks, gamma, mu, allow unused)
  float vmax_raw;         // max ||v|| over the stored vectors, uncentred, rounded up
  const uint4 *img;       // the lists' bf16 image (rank_images.hip)
  const uint4 *qimg;      // the batch's image of -2 q (split_query_image, not centred)
  const uint32_t *block_cnt;
  const uint64_t *allow;  // one allow word per block, or null
  IpQueryTerms t;
  uint32_t *cnt, *ovf;
  uint32_t *keys;         // [nq][cap] score keys of one level (the final sweep's candidate array, not yet in use)
  unsigned long long *counters;  // [kIpSeedCounters], zero on entry
  uint32_t nq, k, nc, nblocks, cap;
  int cus;
};
// every level of `s` on stream `st`: flat_ip_seed_kernel over the level's sample, then flat_ip_tighten_kernel.  On return
// (nothing is synchronised) cnt is zero for every query and thr / tq / ovf are what the final sweep reads.
vi_status ip_seed_ladder(const IpLadderArgs &a, const IpSeedSchedule &s, hipStream_t st);

}  // namespace vi
