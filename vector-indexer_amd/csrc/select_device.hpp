// select_device.hpp — what the select kernels of the MFMA engine share (select.hip: top-k; range_select.hip: radius):
// the frame the rank records live in (SelectCommon), a query's probes in registers, the exact reference distance of one
// (query row, stored vector) pair per lane in its four forms, and where a sub-block's rows sit in their block.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "device_math.hpp"
#include "mfma_bf16.hpp"
#include "scan.hpp"
#include "search_internal.hpp"
#include "select.hpp"
#include "slot_filter.hpp"
#include "wave_sort.hpp"

namespace vi {

constexpr int kWave = 64;

struct SelectCommon {
  const float *Q;
  uint32_t dim, dq;
  const float4 *blocks;
  const float4 *gval;
  const uint32_t *gmeta;
  const float4 *brec;
  float gamma, e_scale, xmax2;
  float e_abs;  // absolute rank error added to the margin (int8 ranking: 1), else 0
  uint32_t gq;  // queries per rank work item (a record tile holds 2 * gq pair records)
  unsigned long long *dbg;  // [6] exact re-evaluations, [7] groups whose pair records were read, [8..] see select_body
  uint32_t image_order;     // the rank kernel multiplied the permuted bf16 image (subblock_vector)
  const uint4 *hi_nat;      // bf16-exact lists: natural-order hi plane for the exact re-evaluation (hi_natural_kernel), else null
  const uint4 *u8_nat;      // 8-bit descriptors: one byte per dimension (u8_natural_kernel), else null
  uint32_t wave_order;      // pair records in the streaming kernel's wave order (scan.hpp: seg_records), else pair order
  uint32_t xmode;           // ablation knob (VI_SELECT_XMODE, wrong results): 1 no exact evaluation, 2 no stage 2, 4 no stage 1b
  uint32_t dbg_mask;        // counters of the queries with (q & dbg_mask) == 0 only (VI_FILTER_STATS=4: every 64th — ten thousand
                            // waves adding to the same few addresses are most of the kernel's time, which the stage clocks then measure)
  const float *mu;          // centre of the ranking images (rank values are those of q - mu against v - mu), or null
  uint32_t trunc;           // real-valued lists ranked from their hi planes: 1 queries hi + lo, 2 queries' hi plane only; 0 otherwise
  float rho_max, vmax;      // ... max |v - hi(v)| and max |v| over the lists (rounded up)
  const uint64_t *allow;    // filtered search (the FILT instantiations of both list selects): one allow word per block (slot_filter.hpp)
};

// the query's probes, one per lane r < P
struct ProbeRegs {
  uint32_t rel, ng;   // first group record (relative to the query's) / number of group records of the probe
  uint32_t boff;      // pair record of (segment 0, pair 0, lane half 0) of the probe; + 2*gq per pair
                      // (pair p of segment s = s * seg_records(segb) + p), + gq for half 1
  uint32_t len, fb;   // list length and first block
  uint32_t segb;      // blocks per segment
  uint32_t g;         // candidate-order rank (shard visiting order)
};

// Loads with the address space spelled out.  The exact-evaluation pieces below are real functions (noinline), so their
// pointer arguments are generic and every access through them compiles to flat_load: the query row in LDS then goes through
// the vector-memory address pipe — the unit the gathers of stored vectors saturate — and every wait covers both counters.
typedef float vf4 __attribute__((ext_vector_type(4)));
typedef uint32_t vu4 __attribute__((ext_vector_type(4)));
typedef float vf2 __attribute__((ext_vector_type(2)));
// a - b on two floats in one instruction (v_pk_add_f32 with the second operand negated: every component rounds as
// v_sub_f32 does; the compiler turns a vector subtraction back into two scalar ones)
__device__ __forceinline__ vf2 pk_sub_f32(vf2 a, vf2 b) {
  vf2 d;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
// acc += (q - x)^2 over four consecutive dimensions in the reference's order: differences and squares two at a time
// (packed instructions: each component rounds exactly as the scalar instruction does), the sum one term after the other
__device__ __forceinline__ void sq_add4(float &acc, const float4 &q, const float4 &x) {
  const vf2 qa = {q.x, q.y}, qb = {q.z, q.w}, xa = {x.x, x.y}, xb = {x.z, x.w};
  const vf2 ta = pk_sub_f32(qa, xa), tb = pk_sub_f32(qb, xb);
  const vf2 sa = ta * ta, sb = tb * tb;
  acc = acc + sa.x; acc = acc + sa.y; acc = acc + sb.x; acc = acc + sb.y;
}
#define VI_AS_LDS __attribute__((address_space(3)))
#define VI_AS_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ float4 lds_f4(const float *p) {
  const vf4 v = *(const VI_AS_LDS vf4 *)(const VI_AS_LDS float *)p;
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint4 lds_u4(const uint32_t *p) {
  const vu4 v = *(const VI_AS_LDS vu4 *)(const VI_AS_LDS uint32_t *)p;
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float4 glb_f4(const float4 *p) {
  const vf4 v = *(const VI_AS_GLOBAL vf4 *)(const VI_AS_GLOBAL float *)reinterpret_cast<const float *>(p);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint4 glb_u4(const uint4 *p) {
  const vu4 v = *(const VI_AS_GLOBAL vu4 *)(const VI_AS_GLOBAL uint32_t *)reinterpret_cast<const uint32_t *>(p);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// exact distance of one (query row, stored vector) pair, one lane per pair (src/utils.rs:28-30).  The query row sits
// in LDS (every lane reads the same address: a broadcast, no vector-memory slot), so all eight loads in flight per
// lane are the stored vector's.  STRIDE, in 16-byte quads, from one quad of the vector to the next: kWave in a 64-vector
// block, 1 for a vector stored as dim consecutive floats (coarse table, rows_from_blocks_kernel)
template <uint32_t STRIDE>
__device__ __forceinline__ float exact_pair(const float *qrow, const float4 *xv, uint32_t dim) {
  float acc = 0.0f;
  const uint32_t nquad = dim >> 2;
  uint32_t qd = 0;
  for (; qd + 8 <= nquad; qd += 8) {
    float4 x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = glb_f4(xv + (size_t)(qd + i) * STRIDE);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float4 qq = lds_f4(qrow + 4 * (qd + i));
      sq_add4(acc, qq, x[i]);
    }
  }
  for (; qd < nquad; ++qd) {
    const float4 qq = lds_f4(qrow + 4 * qd);
    const float4 xx = glb_f4(xv + (size_t)qd * STRIDE);
    sq_add4(acc, qq, xx);
  }
  return acc;
}

// the same sum from the natural-order bf16 hi plane of bf16-exact vectors (hi_natural_kernel): x = bf16 << 16 exactly,
// so every term and the sequential order are those of exact_pair; 16 bytes carry 8 dimensions
__device__ __forceinline__ float exact_pair_bf16(const float *qrow, const uint4 *xh, uint32_t dim) {
  float acc = 0.0f;
  const uint32_t npiece = (dim + 7u) >> 3;  // (dim % 4 == 0: the last piece may hold 4 dimensions)
  auto piece = [&](const uint4 &x, uint32_t p) {
    const float4 q0 = lds_f4(qrow + 8 * p);
    sq_add4(acc, q0, make_float4(__uint_as_float(x.x << 16), __uint_as_float(x.x & 0xFFFF0000u), __uint_as_float(x.y << 16),
                                 __uint_as_float(x.y & 0xFFFF0000u)));
    if (8 * p + 4 < dim) {
      const float4 q1 = lds_f4(qrow + 8 * p + 4);
      sq_add4(acc, q1, make_float4(__uint_as_float(x.z << 16), __uint_as_float(x.z & 0xFFFF0000u), __uint_as_float(x.w << 16),
                                   __uint_as_float(x.w & 0xFFFF0000u)));
    }
  };
  uint32_t p = 0;
  for (; p + 8 <= npiece; p += 8) {
    uint4 x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = glb_u4(xh + (size_t)(p + i) * kWave);
#pragma unroll
    for (int i = 0; i < 8; ++i) piece(x[i], p + i);
  }
  for (; p + 4 <= npiece; p += 4) {  // (a half round: D = 96 has 6 / 12 pieces)
    uint4 x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = glb_u4(xh + (size_t)(p + i) * kWave);
#pragma unroll
    for (int i = 0; i < 4; ++i) piece(x[i], p + i);
  }
  for (; p < npiece; ++p) piece(glb_u4(xh + (size_t)p * kWave), p);
  return acc;
}

// ... and from one byte per dimension (u8_natural_kernel): x = (float)byte exactly
__device__ __forceinline__ float exact_pair_u8(const float *qrow, const uint4 *xb, uint32_t dim) {
  float acc = 0.0f;
  const uint32_t npiece = (dim + 15u) >> 4;  // (dim % 4 == 0: the last piece may hold 4, 8 or 12 dimensions)
  auto word = [&](uint32_t w, uint32_t e) {   // 4 dimensions starting at e
    const float4 q = lds_f4(qrow + e);
    sq_add4(acc, q, make_float4((float)(w & 0xFFu), (float)((w >> 8) & 0xFFu), (float)((w >> 16) & 0xFFu), (float)(w >> 24)));
  };
  auto piece = [&](const uint4 &x, uint32_t p) {
    const uint32_t e = 16 * p;
    word(x.x, e);
    if (e + 4 < dim) word(x.y, e + 4);
    if (e + 8 < dim) word(x.z, e + 8);
    if (e + 12 < dim) word(x.w, e + 12);
  };
  uint32_t p = 0;
  for (; p + 8 <= npiece; p += 8) {
    uint4 x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = glb_u4(xb + (size_t)(p + i) * kWave);
#pragma unroll
    for (int i = 0; i < 8; ++i) piece(x[i], p + i);
  }
  for (; p + 4 <= npiece; p += 4) {  // (a half round: D = 96 has 6 / 12 pieces)
    uint4 x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = glb_u4(xb + (size_t)(p + i) * kWave);
#pragma unroll
    for (int i = 0; i < 4; ++i) piece(x[i], p + i);
  }
  for (; p < npiece; ++p) piece(glb_u4(xb + (size_t)p * kWave), p);
  return acc;
}

// 8-bit descriptors AND an integer-valued query in 0..255 (SIFT queries are): every term (q - x)^2 of the reference's
// sum (src/utils.rs:28-30) is an integer <= 255^2 and every partial sum an integer <= D 255^2 < 2^24 (D <= 256), so the
// sequential f32 sum never rounds: its value IS the integer sum, whatever the order.  It is formed with byte dot
// products: |q|^2 + |x|^2 - 2 q.x, four dimensions per v_dot4_u32_u8 — 90 instructions per distance instead of 512.
// qb: the query as bytes (LDS, D / 4 words, zero padded to whole 16-byte pieces); qn = |q|^2.
__device__ __forceinline__ float exact_pair_u8_int(const uint32_t *qb, uint32_t qn, const uint4 *xb, uint32_t dim) {
  const uint32_t npiece = (dim + 15u) >> 4;
  uint32_t dot = 0u, xx = 0u;
  auto piece = [&](const uint4 &x, uint32_t p) {
    const uint4 q = lds_u4(qb + 4 * p);
    dot = __builtin_amdgcn_udot4(q.x, x.x, dot, false); xx = __builtin_amdgcn_udot4(x.x, x.x, xx, false);
    dot = __builtin_amdgcn_udot4(q.y, x.y, dot, false); xx = __builtin_amdgcn_udot4(x.y, x.y, xx, false);
    dot = __builtin_amdgcn_udot4(q.z, x.z, dot, false); xx = __builtin_amdgcn_udot4(x.z, x.z, xx, false);
    dot = __builtin_amdgcn_udot4(q.w, x.w, dot, false); xx = __builtin_amdgcn_udot4(x.w, x.w, xx, false);
  };
  uint32_t p = 0;
  for (; p + 8 <= npiece; p += 8) {
    uint4 x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = glb_u4(xb + (size_t)(p + i) * kWave);
#pragma unroll
    for (int i = 0; i < 8; ++i) piece(x[i], p + i);
  }
  for (; p < npiece; ++p) piece(glb_u4(xb + (size_t)p * kWave), p);
  return (float)(qn + xx - 2u * dot);  // (an integer below 2^24: exact)
}

// The layout the rank kernels write, read back: vector (within its 64-vector block) of row e (0..15) of sub-block (tile t,
// lane half hh).  The bf16 images are built so that it is 32t + 16hh + e (slot_filter.hpp: image_column — every kernel
// that multiplies an image: filter_kernel RANK 1 / 2, rank_wide_kernel, rank_stream.hip); the f32 MFMA (filter_kernel
// RANK 0, VI_FILTER_BF16=0) multiplies the f32 blocks as they are, where the 16 registers of a lane of half hh hold rows
// (e&3) + 8(e>>2) + 4hh of the tile
__device__ __forceinline__ uint32_t subblock_vector(uint32_t e, uint32_t t, uint32_t hh, bool image_order) {
  return image_order ? 32u * t + 16u * hh + e : 32u * t + (e & 3u) + 8u * (e >> 2) + 4u * hh;
}

constexpr uint32_t kPickCap = 256;     // sub-blocks waiting for their 16 exact distances (per wave)
constexpr uint32_t kSubBits = 21;      // request key = (probe rank << 22) | (sub-block of the list << 1) | lane half
constexpr uint32_t kCacheG = 256;      // group records (values + probe/segment/half) kept in LDS per wave

// the frame of a list or table ranked with the batch's arithmetic (b.kn), records in b's workspace; the launchers adjust it per phase
inline SelectCommon select_common(const SearchBatch &b, const float4 *blocks, float xmax2, uint32_t gq, bool wave_order = false, int trunc = 0) {
  const DeviceIndex &ix = b.ix;
  const EngineKnobs &kn = b.kn;
  const double u = 1.01 * std::ldexp(1.0, -24);
  SelectCommon c{};
  c.Q = b.Qd; c.dim = ix.dim; c.dq = ix.dq; c.blocks = blocks;
  c.gval = (const float4 *)b.ws().gval.p; c.gmeta = (const uint32_t *)b.ws().gpos.p;
  c.brec = (const float4 *)b.ws().brec.p;
  c.gamma = (float)((ix.dim + 2.0) * u);
  // |ranked value - (||v||^2 - 2 q.v)| <= e_scale (||q||^2 + 2 max||v||^2):
  //   f32 MFMA : (D+2) u'  accumulation of D products + the norm
  //   bf16 x 3 : 2^-15 for the dropped lo.lo product and the two split residuals (bf16 keeps 8 significant bits:
  //              |x - hi| <= 2^-8 |x|, |x - hi - lo| <= 2^-17 |x|; 2 (|ql.vl| + |qr.v| + |q.vr|) <= 2 (2^-16 + 2 * 2^-17)
  //              |q||v| <= 2^-15 (|q|^2 + |v|^2) — round 2 budgeted 3 * 2^-18 here, 2.7 times too little), and
  //              (3D+2) * 2u' for the f32 accumulation of 3D exact bf16 products (2u': also covers an accumulator that truncates)
  const double acc = kn.rank_bf16 ? (3.0 * ix.dim + 2.0) * 2.0 * u + 1.01 * std::ldexp(1.0, -15) : (ix.dim + 2.0) * u;
  //   (real-valued lists ranked from their bf16 hi planes alone: SelectCommon::trunc, added per query in select_body)
  // centred images (DeviceIndex::centered): v - mu and q - mu are rounded before they are split — the ranked pair sits
  // within 2^-24 (|q'| + |v'|) of the true one, its distance within 4 * 2^-24 (|q'|^2 + |v'|^2) of the true distance
  const bool centred = ix.centered && kn.rank_bf16;
  c.e_scale = (float)(acc + (centred ? 6.0 * u : 0.0));
  c.e_abs = 0.0f;
  c.trunc = (uint32_t)trunc;
  c.rho_max = (float)(std::sqrt((double)ix.rho2_max) * 1.0001);
  c.vmax = (float)(std::sqrt((double)xmax2) * 1.0001);
  c.xmax2 = xmax2;
  c.mu = centred ? ix.centre.p : nullptr;
  c.gq = gq;
  c.image_order = kn.rank_bf16 ? 1u : 0u;
  c.wave_order = wave_order ? 1u : 0u;
  c.hi_nat = nullptr;
  c.u8_nat = nullptr;
  c.allow = nullptr;
  // per-wave counters go to two addresses: 2 same-address atomics per query cost more than the whole select, so
  // they are a diagnostic (VI_FILTER_STATS=1), not part of the normal path
  c.dbg = kn.stats ? (unsigned long long *)b.ws().stats.p : nullptr;
  c.dbg_mask = kn.stats_mask;
  c.xmode = kn.select_xmode;
  return c;
}

// ... of the list phase as ranked per SelectFrame: what both list selects (top-k, radius) start from
inline SelectCommon list_select_common(const SearchBatch &b, const SelectFrame &f) {
  const DeviceIndex &ix = b.ix;
  SelectCommon c = select_common(b, (const float4 *)ix.lists.blocks.p, b.kn.rank_bf16 && ix.centered ? ix.xmax2_c : ix.xmax2, f.gq,
                                 f.wave_order, f.approx);
  if (b.kn.stats_coarse) c.dbg = nullptr;
  c.hi_nat = (const uint4 *)ix.lists_hi_nat.p;
  c.u8_nat = (const uint4 *)ix.lists_u8_nat.p;
  if (f.rank_i8) {  // rank values 2 r within [m', m' + 1] of m' = |q - v|^2 - |q - 127|^2: the margins of that frame, an absolute error of 1
    c.mu = ix.i8_centre.p;
    c.e_scale = 0.0f;
    c.e_abs = 1.0f;
    c.xmax2 = ix.i8_xmax2;
    c.vmax = (float)(std::sqrt((double)ix.i8_xmax2) * 1.0001);
  }
  return c;
}

}  // namespace vi
