// flat_common.hpp — the device pieces the flat (exact, whole-index) calls share: flat_search.hip (k-NN),
// flat_range.hip (radius), flat_join.hip (the radius self-join), flat_knn.hip (the k-NN
// self-join), flat_ip.hip (inner-product k-NN) and flat_ip_range.hip (inner-product threshold
// search).  Each translation unit compiles
// its own copy (unnamed namespace): the reference chain of one pair, the rank threshold of a radius and of a score, the
// inner-product result key, the bf16 image of one query, the per-block ordinals and the way back from an ordinal to its block.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.hpp"
#include "list_layout.hpp"
#include "mfma_bf16.hpp"
#include "select_device.hpp"

namespace vi {
namespace {

// the reference's sum (src/utils.rs:28-30) of one (query row, stored vector) pair: one sequential f32 chain, no fused
// multiply-add (the file is compiled with -ffp-contract=off), written without packed instructions
__device__ __forceinline__ float exact_scalar(const float *qrow, const float4 *xv, uint32_t dim) {
  float acc = 0.0f;
  for (uint32_t qd = 0; qd < (dim >> 2); ++qd) {
    const float4 x = xv[(size_t)qd * kWave];
    const float4 q = *reinterpret_cast<const float4 *>(qrow + 4 * qd);
    sq_add(acc, q.x, x.x); sq_add(acc, q.y, x.y); sq_add(acc, q.z, x.z); sq_add(acc, q.w, x.w);
  }
  return acc;
}

// the inner product of one (query row, stored vector) pair as the exact inner-product search defines it (flat_ip.hip,
// DESIGN §4v): s = 0; s = s + q[i] * v[i] for i ascending, multiply and add rounded separately (no fused multiply-add).
// The chain starts at +0 and x + (-x) rounds to +0, so it never yields -0
__device__ __forceinline__ float ip_scalar(const float *qrow, const float4 *xv, uint32_t dim) {
  float acc = 0.0f;
  for (uint32_t qd = 0; qd < (dim >> 2); ++qd) {
    const float4 x = xv[(size_t)qd * kWave];
    const float4 q = *reinterpret_cast<const float4 *>(qrow + 4 * qd);
    acc = acc + q.x * x.x; acc = acc + q.y * x.y; acc = acc + q.z * x.z; acc = acc + q.w * x.w;
  }
  return acc;
}

// The rank threshold of radius r >= 0 for the query of frame f: a record with reference distance <= r has a true rank
// value <= r - qn up to the rounding of the reference's own sum (w, as the radius select forms it); rank_threshold adds the
// rank arithmetic's margins.  A radius beyond the point where the bound means anything, or a distrusted query: no bound,
// every admitted record is evaluated
__device__ __forceinline__ float radius_rank_threshold(const SelectCommon &c, const QueryFrame &f, float r) {
  float thr = INFINITY;
  if (r < 1.0e37f) {
    const float w = ((float)(c.dim >> 6) + 9.0f) * 6.1e-8f * (fabsf(r) + f.qn);
    thr = rank_threshold(c, f, (r - f.qn) + w);
  }
  return thr;
}

// ---- inner product (flat_ip.hip, flat_ip_range.hip) ----
// A result key: the score's bits mapped so that unsigned order is DESCENDING score order, above the record's list-order
// ordinal: an ascending u64 sort is "score descending, ordinal ascending".  The map flips the sign bit of a non-negative
// score and every bit of a negative one (ascending order), then complements.  ip_scalar never yields -0, so equal scores
// have equal bits; no finite or infinite score maps to all ones, which stays "no record".
__device__ __forceinline__ uint64_t ip_key(float s, uint32_t ordinal) {
  const uint32_t b = __float_as_uint(s), up = (b & 0x80000000u) ? ~b : b ^ 0x80000000u;
  return ((uint64_t)~up << 32) | ordinal;
}
__device__ __forceinline__ float ip_key_score(uint64_t key) {
  const uint32_t up = ~(uint32_t)(key >> 32);
  return __uint_as_float((up & 0x80000000u) ? up ^ 0x80000000u : ~up);
}

// one wave: q.mu and sum |q_i mu_i| of the query row against the centre of the block images (both 0 where c.mu is null)
__device__ __forceinline__ void ip_centre_terms(const SelectCommon &c, const float *row, int lane, float &qm, float &am) {
  qm = 0.0f; am = 0.0f;
  if (c.mu)
    for (uint32_t e = lane; e < c.dim; e += kWave) {
      const float t = row[e] * c.mu[e];
      qm += t; am += fabsf(t);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { qm += __shfl_xor(qm, o); am += __shfl_xor(am, o); }
}

// The rank threshold of score t: thr = -2 t + 2 q.mu + margins, rounded outwards.  A record is wanted if its
// chain score s~ >= t.  f: the frame of the query with mu = nullptr (the UNCENTRED ||q||^2 and budget E); c: the frame of
// the block images (gamma, mu); qm, am: ip_centre_terms; vmax_raw: max ||v|| over the stored vectors, uncentred, rounded up.
//   |s~ - q.v| <= gamma sum |q_i v_i| <= gamma ||q|| max ||v||  (gamma = (D+2)u' >= the chain's (D+1)u'), so a wanted
//   record has -2 q.v <= -2 t + 2 gamma ||q|| max ||v||; the true swept value is p = -2 q.v' = -2 q.v + 2 q.mu;
//   qm is q.mu within gamma sum |q_i mu_i| (am, itself within a factor 1 + gamma); the swept value is p within
//   E = e_scale (||q||^2 (1 + gamma) + 2 max ||v'||^2): §2b's bf16 x 3 budget for an accumulator that starts at zero,
//   the rounding of v - mu included;
//   forming -2 t + 2 qm and adding the margin rounds three times at magnitudes <= 2 |t| + 2 |qm| + margin.
// The caller decides what a non-finite or huge value means (no bound).
__device__ __forceinline__ float ip_rank_threshold(const SelectCommon &c, const QueryFrame &f, float qm, float am, float vmax_raw, float t) {
  const float qnorm = sqrtf(f.qn * (1.0f + c.gamma)) * 1.0001f;
  const float mk = -2.0f * t + 2.0f * qm, mag = 2.0f * fabsf(t) + 2.0f * fabsf(qm);
  const float margin = f.E + 2.0f * c.gamma * qnorm * vmax_raw + 2.02f * c.gamma * am + c.gamma * mag;
  return mk + margin * 1.001f + 1e-30f;
}

// ---- per block: the list-order ordinal of its first record and the records it holds (1..64) ----
__global__ void flat_blocks_kernel(const uint32_t *first_block, const uint32_t *list_len, const uint64_t *prefix, uint32_t nlists,
                                   uint32_t nblocks, uint32_t *block_ord, uint32_t *block_cnt) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nblocks) return;
  const uint32_t l = list_of_block(first_block, nlists, b);
  const uint32_t pos0 = (b - first_block[l]) * 64u, len = list_len[l];
  block_ord[b] = (uint32_t)prefix[l] + pos0;
  block_cnt[b] = len > pos0 ? min(64u, len - pos0) : 0u;
}

// one wave: query q of the frame c -> its bf16 image of nc chunks,
// qimg[query][plane hi / lo][chunk][half] x 16 B of -2 (q - mu): the layout every rank kernel reads
__device__ __forceinline__ void split_query_image(const SelectCommon &c, uint32_t q, uint32_t nc, int lane, uint4 *qimg) {
  const float *row = c.Q + (size_t)q * c.dim;
  for (uint32_t p = lane; p < 2u * nc; p += kWave) {  // piece (chunk ch, half h): dimensions 16 ch + 8 h ..
    const uint32_t ch = p >> 1, h = p & 1u, e = 16u * ch + 8u * h;
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f), v1 = v0;
    if (e < c.dim) v0 = *reinterpret_cast<const float4 *>(row + e);  // dim % 4 == 0
    if (e + 4 < c.dim) v1 = *reinterpret_cast<const float4 *>(row + e + 4);
    if (c.mu) {
      if (e < c.dim) { const float4 m = *reinterpret_cast<const float4 *>(c.mu + e); v0.x -= m.x; v0.y -= m.y; v0.z -= m.z; v0.w -= m.w; }
      if (e + 4 < c.dim) { const float4 m = *reinterpret_cast<const float4 *>(c.mu + e + 4); v1.x -= m.x; v1.y -= m.y; v1.z -= m.z; v1.w -= m.w; }
    }
    uint4 hi, lo;
    split8(v0, v1, -2.0f, hi, lo);
    qimg[(size_t)q * 4 * nc + 2 * ch + h] = hi;
    qimg[(size_t)q * 4 * nc + 2 * nc + 2 * ch + h] = lo;
  }
}

// the block of a list-order ordinal: block_ord[b] <= ordinal < block_ord[b + 1] (every block holds a record)
__device__ __forceinline__ uint32_t block_of_ordinal(const uint32_t *block_ord, uint32_t nblocks, uint32_t ordinal) {
  uint32_t lo = 0, hi = nblocks;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (block_ord[mid] <= ordinal) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace
}  // namespace vi
