// select_device.hpp — what the select kernels of the MFMA engine share (select.hip: top-k; range_select.hip: radius):
// the frame the rank records live in (SelectCommon), the exact reference distance of one (query row, stored vector) pair
// per lane in its four forms, where a sub-block's rows sit in their block, and — once, for every select — the soundness
// core of DESIGN §2b: the query in that frame with its error bound (QueryFrame, query_frame), the threshold (*) built
// from it (rank_threshold), a query's probes in registers (ListProbes, load_probe_regs) and the walk over its records
// (GroupRecords, scan_pair_records, the pick queue: push_sub / drain_pick).  All inlined: the callers keep the counters
// and what is done with a value; the noinline exact-evaluation pieces stay with their kernels.
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

// ---- the query in the frame its rank records live in ----
struct QueryFrame {
  float qn;         // ||q'||^2, q' = q - mu where the images are centred: the margins live where the rank values do
  float E;          // |recorded rank value - true one| <= E for every vector the query probes
  uint32_t qn_int;  // q_bytes: ||q||^2 as an integer
  bool q_bytes;     // 8-bit lists, D <= 256 and the query integer-valued in 0..255: exact_pair_u8_int applies
  bool distrust;    // a query so large that the rank arithmetic may have overflowed (inf - inf = NaN, and NaN fails every
                    // guard of the selects): trust no rank value, re-evaluate everything the query probes
};

// One wave: the frame of query q.  STAGE: the row goes to qlds for the exact evaluations (visible to the wave after the
// next wave_lds_sync) and, under q_bytes, its byte form to qbytes (null: the caller has no use for it)
template <bool STAGE>
__device__ __forceinline__ QueryFrame query_frame(const SelectCommon &c, uint32_t q, int lane, float *qlds, uint32_t *qbytes) {
  QueryFrame f;
  float qn = 0.0f, qres = 0.0f;
  bool q_bytes = c.u8_nat != nullptr && qbytes != nullptr && c.dim <= 256u;
  for (uint32_t e = lane; e < c.dim; e += kWave) {
    const float v = c.Q[(size_t)q * c.dim + e];
    if (STAGE) qlds[e] = v;
    const float vc = c.mu ? v - c.mu[e] : v;
    qn += vc * vc;
    const float im = -2.0f * vc, ir = im - __uint_as_float(bf16_rn(im) << 16);  // what the hi plane of the query image leaves out
    qres += ir * ir;
    q_bytes = q_bytes && v >= 0.0f && v <= 255.0f && v == floorf(v);
  }
  f.q_bytes = __ballot(!q_bytes) == 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { qn += __shfl_xor(qn, o); qres += __shfl_xor(qres, o); }
  f.qn = qn;
  f.qn_int = 0u;
  if (STAGE && f.q_bytes) {  // the query as bytes, zero padded to whole 16-byte pieces (exact_pair_u8_int), and |q|^2 as an integer
    const uint32_t nw = ((c.dim + 15u) >> 4) * 4u;
    for (uint32_t w = lane; w < nw; w += kWave) {
      uint32_t word = 0u;
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b) {
        const uint32_t e = 4u * w + b;
        const uint32_t v = e < c.dim ? (uint32_t)c.Q[(size_t)q * c.dim + e] : 0u;
        word |= v << (8u * b);
        f.qn_int += v * v;
      }
      qbytes[w] = word;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) f.qn_int += (uint32_t)__shfl_xor((int)f.qn_int, o);
  }
  f.E = c.e_scale * (qn * (1.0f + c.gamma) + 2.0f * c.xmax2) + c.e_abs;
  // hi planes of real-valued lists: the image (-2q) . v is ranked as (-2q) . hi(v) [trunc 1] or hi(-2q) . hi(v) [trunc 2];
  // |(-2q) . (v - hi v)| <= 2 |q| rho_max, and |(-2q - hi(-2q)) . v| <= |query residual| max|v|  (|hi(-2q)| <= 2 |q| (1 + 2^-8))
  if (c.trunc) f.E += 1.02f * (2.0f * sqrtf(qn) * c.rho_max * (1.0f + 0.00391f) + (c.trunc == 2u ? sqrtf(qres) * c.vmax : 0.0f));
  f.distrust = !(qn < 1.0e30f);
  return f;
}

// (*) of select.hip: with mk an upper bound, in the query's frame, of the rank values wanted, every vector wanted has a
// recorded value at or below this.  Anything non-finite or huge, or a distrusted query, means "no bound"
__device__ __forceinline__ float rank_threshold(const SelectCommon &c, const QueryFrame &f, float mk) {
  if (f.distrust || !(mk < 1.0e37f)) return INFINITY;
  const float scale = fmaxf(mk + f.qn, 0.0f) + f.E;
  return mk + (2.0f * f.E + 3.0f * c.gamma * scale) * 1.001f + 1e-30f;
}

// ---- a query's probes, as the grouping left them (both list selects) ----
struct ListProbes {
  const uint32_t *qoff, *qtot, *rel, *pair_pos, *tile_start;
  const uint32_t *probes, *gorder, *first_block, *list_len;
  uint32_t segb0;
};

inline ListProbes list_probes(const SearchBatch &b) {
  const SearchWorkspace &ws = b.ws();
  return ListProbes{ws.qoff.p, ws.qtot.p, ws.pair_rel.p, ws.pair_pos.p, ws.tile_start.p, ws.probes.p, ws.gorder.p,
                    b.ix.list_first_block.p, b.ix.list_len.p, b.kn.segb0};
}

// lane r < P: probe r of query q (its list to *mylist, kNoPos for none)
__device__ __forceinline__ ProbeRegs load_probe_regs(const ListProbes &lp, uint32_t gq, uint32_t q, uint32_t P, int lane,
                                                     uint32_t *mylist = nullptr) {
  ProbeRegs pr{0u, 0u, 0u, 0u, 0u, 1u, kNoPos};
  uint32_t list = kNoPos;
  if ((uint32_t)lane < P) {
    const size_t s = (size_t)q * P + lane;
    list = lp.probes[s];
    pr.g = lp.gorder[s];
    pr.rel = lp.rel[s];
    if (list != kNoPos) {
      pr.len = lp.list_len[list];
      pr.fb = lp.first_block[list];
      const uint32_t pp = lp.pair_pos[s];  // where the pair sits among the pairs of its list
      const uint32_t nseg = list_segments(pr.len, lp.segb0, &pr.segb);
      pr.ng = 2u * nseg;
      pr.boff = (lp.tile_start[list] + (pp / gq) * nseg * seg_records(pr.segb)) * (2u * gq) + (pp % gq);
    }
  }
  if (mylist) *mylist = list;
  return pr;
}

// ---- the record walk of one wave: the query's G group records at gbase, the pair records of the groups it flags, and
//      the sub-blocks those flag for their 16 exact distances ----
// The first kCacheG group records in LDS, read in one round of loads (the passes over them would otherwise each pay the
// global-memory latency per 64 groups); the rest are read where they lie.  The cache is read with its address space spelled
// out: through the generic pointers a wave keeps both 64-bit addresses live across the whole walk, where the kernels
// have no registers to spare (resource table)
struct GroupRecords {
  const SelectCommon &c;
  size_t gbase;
  uint32_t G;
  float4 *tcache;
  uint32_t *lcache;

  __device__ __forceinline__ void fill(int lane) const {
    float4 t4[kCacheG / kWave];
#pragma unroll
    for (uint32_t ch = 0; ch < kCacheG / kWave; ++ch) {
      const uint32_t gidx = ch * kWave + lane;
      t4[ch] = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
      if (gidx < G) t4[ch] = c.gval[gbase + gidx];
    }
    uint32_t l4[kCacheG / kWave];
#pragma unroll
    for (uint32_t ch = 0; ch < kCacheG / kWave; ++ch) {
      const uint32_t gidx = ch * kWave + lane;
      l4[ch] = 0u;
      if (gidx < G) l4[ch] = c.gmeta[gbase + gidx];  // probe rank | segment << 6 | lane half << 13
    }
#pragma unroll
    for (uint32_t ch = 0; ch < kCacheG / kWave; ++ch) {
      const uint32_t gidx = ch * kWave + lane;
      if (ch * kWave < G) {
        tcache[gidx] = t4[ch];
        lcache[gidx] = l4[ch];
      }
    }
    wave_lds_sync();
  }
  __device__ __forceinline__ float4 group_values(uint32_t gidx, bool live) const {
    float4 T = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    if (live) T = gidx < kCacheG ? lds_f4((const float *)(tcache + gidx)) : c.gval[gbase + gidx];
    return T;
  }
  __device__ __forceinline__ void group_place(uint32_t gidx, bool live, uint32_t &r, uint32_t &seg, uint32_t &hh) const {
    uint32_t L = 0u;
    if (live) L = gidx < kCacheG ? *(const VI_AS_LDS uint32_t *)(lcache + gidx) : c.gmeta[gbase + gidx];
    r = L & 63u; seg = (L >> 6) & 127u; hh = L >> 13;
  }
};

// The pair records of the groups flagged `want` (probe rank r, segment seg, lane half hh: group_place), four groups per
// round (16 lanes x one pair record = the 64 sub-block minima of a 32-block segment half).  Every lane calls;
// visit(ok, value, j, probe rank, sub-block of the list, lane half) sees component j of every record, ok false where
// there is no value
template <class Visit>
__device__ __forceinline__ void scan_pair_records(const SelectCommon &c, const ProbeRegs &pr, int lane, bool want, uint32_t r, uint32_t seg,
                                                  uint32_t hh, uint32_t &n_scanned, Visit visit) {
  uint64_t m = __ballot(want);
  const uint32_t slot = (uint32_t)lane >> 4, pi = (uint32_t)lane & 15u;
  while (m) {
    int src = 0;
    uint32_t taken = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
      if (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1ull;
        if (slot == i) src = b;
        ++taken;
      }
    const bool mine = slot < taken;
    n_scanned += taken;
    const uint32_t rr = (uint32_t)__shfl((int)r, src), sg = (uint32_t)__shfl((int)seg, src);
    const uint32_t h2 = (uint32_t)__shfl((int)hh, src);
    const uint32_t segb = (uint32_t)__shfl((int)pr.segb, (int)rr), ln = (uint32_t)__shfl((int)pr.len, (int)rr);
    const uint32_t boff = (uint32_t)__shfl((int)pr.boff, (int)rr);
    const uint32_t nblk = (ln + kWave - 1) / kWave;
    const uint32_t bs = sg * segb, be = min(nblk, bs + segb);
    // records of the segment: pair order (record p = blocks 2p, 2p + 1; component j = sub-block 4p + j), or the streaming
    // kernel's wave order (record p, component j = 32-vector tile 16 (p >> 2) + 4 j + (p & 3))
    const uint32_t ntile = be > bs ? 2u * (be - bs) : 0u;
    const uint32_t npairs = !mine ? 0u : (c.wave_order ? 4u * ((ntile + 15u) / 16u) : (ntile + 3u) / 4u);
    uint32_t mx = npairs;  // wave maximum: segments of very long lists hold more than 16 records
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    for (uint32_t p0 = 0; p0 < mx; p0 += 16u) {
      const uint32_t p = p0 + pi;
      const bool live = p < npairs;
      float4 B = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
      if (live) B = c.brec[(size_t)boff + 2u * c.gq * (sg * seg_records(segb) + p) + c.gq * h2];
      const float bv[4] = {B.x, B.y, B.z, B.w};
#pragma unroll
      for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t tl = c.wave_order ? 16u * (p >> 2) + 4u * j + (p & 3u) : 4u * p + j;  // tile of the segment
        const bool ok = live && tl < ntile;  // (a record's unused components, and records no wave wrote, are not read as values)
        visit(ok, bv[j], j, rr, 2u * bs + tl, h2);
      }
    }
  }
}

// sub-blocks waiting in `pick`: four per round, 16 lanes (= the 16 rows of the sub-block) each;
// exact(live, probe rank, position) takes one (query, stored vector) pair per lane
template <class Exact>
__device__ __forceinline__ void drain_pick(const SelectCommon &c, const uint32_t *pick, uint32_t &npick, int lane, Exact exact) {
  while (npick > 0) {
    const uint32_t cnt = npick >= 4u ? 4u : npick;
    npick -= cnt;
    const uint32_t rq = (uint32_t)lane >> 4;
    const bool live = rq < cnt;
    const uint32_t ck = live ? pick[npick + rq] : 0u;
    const uint32_t r = ck >> (kSubBits + 1), sub = (ck >> 1) & ((1u << kSubBits) - 1u), hh = ck & 1u;
    exact(live, r, (sub >> 1) * kWave + subblock_vector((uint32_t)lane & 15u, sub & 1u, hh, c.image_order != 0u));
  }
}

// every lane calls; the lanes that `want` queue their sub-block, after drain() has made room where the queue is full
template <class Drain>
__device__ __forceinline__ void push_sub(uint32_t *pick, uint32_t &npick, uint32_t &n_sub, int lane, bool want, uint32_t r, uint32_t sub,
                                         uint32_t hh, Drain drain) {
  const uint64_t m = __ballot(want);
  if (!m) return;
  const uint32_t cnt = (uint32_t)__popcll(m);
  n_sub += cnt;
  if (npick + cnt > kPickCap) drain();
  if (want) pick[npick + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (r << (kSubBits + 1)) | (sub << 1) | hh;
  npick += cnt;
  wave_lds_sync();
}

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
