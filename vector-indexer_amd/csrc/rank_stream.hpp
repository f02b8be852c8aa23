// rank_stream.hpp — the streaming list-rank kernel (rank_stream.hip) as mfma_search.hip's pipeline launches it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace vi {

struct RankStreamArgs {
  const uint4 *img;     // bf16 hi/lo image of the lists: per block nc chunks x [plane][half] x 64 columns x 16 B
  const float *xnorm;   // squared norms in image-column order
  const uint4 *qimg;    // -2 q of the batch split hi / lo: per query [plane][chunk][half] x 16 B (split_queries_kernel)
  const uint4 *sdesc;   // per work item {queries, first block, 32-vector tiles, first record tile} (item_cols_kernel)
  uint32_t nitems;
  const uint32_t *qcol;  // per (item, column of the group): the query (item_cols_kernel), ~0: none
  const uint32_t *grec;  // per (item, column): index of the group record of lane half 0, ~0: none
  uint32_t *queue;       // work counter, zero at launch
  float4 *gval;         // group records (their place words are written by group_place_kernel)
  float4 *brec;         // pair records, wave order (scan.hpp: seg_records)
  unsigned long long *prof;  // diagnostic: the counter block of phase clocks below (kRankStreamProfWords), or null
  uint32_t xmode;       // ablation knob (VI_FILTER_XMODE): 1 tiles not re-read, 2 no ranking epilogue, 8 no record store
};
// 64-bit words of the counter block `prof` points at: 32 of totals (zero at launch, word 16 all ones: a minimum), then
// 4 per workgroup
constexpr uint32_t kRankStreamProfWords = 32 + 4 * 1024;
// (VI_STREAM_PROF) the block's phase clocks to stderr, read back behind the kernel on st: synchronises.  dump_path (or
// null: VI_STREAM_PROF_DUMP): a file for the per-workgroup clocks
vi_status print_rank_stream_profile(const uint64_t *prof_dev, const char *dump_path, hipStream_t st);

// rank_mode 1: bf16 x 3; 2: the stored vectors are bf16-exact (hi planes only); qlo: the batch's queries have a lo plane
// gq: queries per work item the grouping formed, 128 or 256
vi_status launch_rank_stream(const RankStreamArgs &a, uint32_t nc, uint32_t nitems, int rank_mode, bool qlo, uint32_t gq, hipStream_t st);

// 8-bit descriptors (every stored value an integer in 0..255) against queries of integers in 0..254: the same work items
// ranked with exact int8 products, in the frame shifted by 127 (rank_images.hip: i8_image_kernel; mfma_search.hip: split_queries_kernel).
// Rank value of (q, v): 2 r with r = h(v) - q'.v', q' = q - 127, v' = v - 127, h(v) = ceil(|v'|^2 / 2) — an integer with
// |v'|^2 - 2 q'.v' <= 2 r <= |v'|^2 - 2 q'.v' + 1, stored as a float (exact below 2^24).
struct RankStreamI8Args {
  const uint4 *img;      // A = 127 - v as int8 (0 on padded dimensions): per block nc32 chunks x [half] x 64 columns x 16 B
  const int *hnorm;      // h(v) in image-column order (pad slots: kI8PadNorm)
  const uint4 *qimg;     // B = q - 127 as int8 (0 on padded dimensions): per query nc32 x [half] x 16 B (split_queries_kernel)
  const uint4 *sdesc;    // as RankStreamArgs
  uint32_t nitems;
  const uint32_t *qcol;
  const uint32_t *grec;
  uint32_t *queue;
  float4 *gval;
  float4 *brec;
};
constexpr int kI8PadNorm = 1 << 28;  // above every h(v) (< 2^21 for D <= 128); 2 r stays below 2^31

// nc32: chunks of 32 dimensions (1..4)
vi_status launch_rank_stream_i8(const RankStreamI8Args &a, uint32_t nc32, uint32_t nitems, uint32_t gq, hipStream_t st);

}  // namespace vi
