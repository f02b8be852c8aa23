// rank_block.hpp — the block-synchronous rank kernels (rank_block.hip: filter_kernel for D <= 128, lists and the coarse
// table; rank_wide_kernel for 128 < D <= 1536) as mfma_search.hip's pipeline launches them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"

namespace vi {

struct RankBlockArgs {
  const float4 *blocks;  // f32 blocks, or the bf16 hi/lo image of the same size (BF16 kernels)
  const float *xnorm;
  uint32_t dq, dim;
  const float *Q;
  const uint32_t *first_block, *list_len, *item_start, *seg_start, *pairs;
  uint32_t nlists, P, segb0;
  const uint32_t *qoff, *rel;  // group-record offsets (lists) ...
  uint32_t rec_stride;         // ... or a fixed number of records per slot when qoff is null (coarse table)
  const uint32_t *tile_start;  // pair records: first record tile (2 * GQ records) of each list
  const uint4 *items;          // list phase: the work items' descriptors (item_desc_kernel), or null: derived here
  float4 *gval;                // group records: the four smallest sub-block minima of a (pair, segment, lane half)
  uint32_t *gmeta;             // ... and where the record belongs: probe rank | segment << 6 | lane half << 13
  float4 *brec;                // pair records: the sub-block minima of two blocks
  const uint4 *qimg;  // bf16 ranking: -2 q of the batch split hi / lo once per search (split_queries_kernel)
  uint32_t direct;  // coarse table only: records = the minima of the 8-row sub-blocks of every block, no group records
  uint32_t xmode;  // experiment knob (VI_FILTER_XMODE): 1 = do not restage tiles, 2 = no ranking epilogue
};

// dq: quads per vector (a multiple of 4, <= 32); rank_mode 0: f32 MFMA, 1: bf16 x 3, 2: hi planes only (the kernel's RANK);
// gq: queries per work item, 32 (lists only) or 128; a.qoff null: the coarse table's instance.  nitems 0: nothing launched
vi_status launch_rank_block(const RankBlockArgs &a, uint32_t dq, uint32_t nitems, int rank_mode, uint32_t gq, hipStream_t st);

struct RankWideArgs {
  const uint4 *img;      // bf16 hi/lo image of the lists: per block nc chunks x [plane][half] x 64 columns x 16 B
  const float *xnorm;    // squared norms in image-column order
  const uint4 *qimg;     // query-major image of the batch: [query][nc][plane][half] x 16 B of -2 q split hi / lo
  uint32_t nc;           // 16-dim chunks per vector
  const uint32_t *first_block, *list_len, *item_start, *seg_start, *pairs, *item_list;
  uint32_t P, segb0;
  const uint32_t *qoff, *rel, *tile_start;
  float4 *gval;
  uint32_t *gmeta;
  float4 *brec;
};

// reserves the kernel's dynamic LDS on the device that launches; nitems 0: nothing launched
vi_status launch_rank_wide(const RankWideArgs &a, uint32_t nitems, hipStream_t st);

}  // namespace vi
