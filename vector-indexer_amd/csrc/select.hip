// select.hip — the select phase of the MFMA engine: from the records the rank kernels leave (rank_block.hip,
// rank_stream.hip) to the exact top-k, for the lists (select_kernel) and for the coarse table (coarse_select_kernel,
// coarse_select_direct_kernel).  Only the records are shared with the rank kernels; what a record holds and where it
// sits is described there and in scan.hpp.
//
//   select       one wave per query reads its group records (4 values per 1024 scanned vectors).
//                With m_K the K-th smallest recorded value, every vector of the true top-K has
//                    m <= thr = m_K + 2E + 3 gamma (m_K + ||q||^2 + E)            (*)
//                    gamma = (D+2) u'                      rounding of the reference's sequential sum
//                    E     = e (||q||^2 + 2 max||v||^2), e = rank arithmetic (select_common)
//                because the K recorded minima below m_K belong to K different vectors, which already bound the
//                K-th reference distance.  A vector with m <= thr sits in a sub-block whose minimum is <= thr, and a
//                sub-block with minimum <= thr sits in a group with T0 <= thr: the pair records of exactly those
//                groups are read, and every sub-block whose minimum is <= thr is re-evaluated as a whole — 16
//                reference distances (exact sequential f32, src/utils.rs:28-30), four sub-blocks per wave
//                instruction.  The top-K of those under the reference's stable order (distance, shard visiting
//                order, position) is the answer, bit for bit (tests/test_search_gpu.py).  Groups whose T3 is below
//                the first bound hide neighbours behind their four listed minima; their pair records tighten the
//                bound before anything is re-evaluated.
//
// The coarse quantizer (ivf_index.rs:205-220) is the same computation with the centroid table as one list probed by
// every query and K = n_probe.
#include "select.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

#include "select_device.hpp"
#include "wave_select.hpp"

namespace vi {
namespace {

// ------------------------------------------------------------------------------------------
// select
// ------------------------------------------------------------------------------------------
// The select kernels are latency-sensitive code executed once per query; inlining the two heavy pieces at
// every call site made them ~150 KB each and instruction-fetch bound.  They are real functions with their state
// passed and returned in registers.
template <class Top>
__device__ __attribute__((noinline)) Top offer_bulk_fn(Top s, float dist, uint32_t pos, int K) {
  s.offer_bulk(dist, pos, K);
  return s;
}

// exact distance of (qrow, xv) on live lanes, then offer (distance, key) to `sel`
template <class Top>
__device__ __attribute__((noinline)) Top exact_batch_fn(Top sel, const float *qrow, const float4 *xv, uint32_t dim, bool live,
                                                        uint32_t key, int K) {
  float d = INFINITY;
  if (live) d = exact_pair<kWave>(qrow, xv, dim);
  sel.offer_bulk(d, live ? key : kNoPos, K);
  return sel;
}

template <class Top>
__device__ __attribute__((noinline)) Top exact_batch_u8_fn(Top sel, const float *qrow, const uint4 *xb, uint32_t dim, bool live, uint32_t key,
                                                           int K) {
  float d = INFINITY;
  if (live) d = exact_pair_u8(qrow, xb, dim);
  sel.offer_bulk(d, live ? key : kNoPos, K);
  return sel;
}

template <class Top>
__device__ __attribute__((noinline)) Top exact_batch_u8_int_fn(Top sel, const uint32_t *qb, uint32_t qn, const uint4 *xb, uint32_t dim, bool live,
                                                               uint32_t key, int K) {
  float d = INFINITY;
  if (live) d = exact_pair_u8_int(qb, qn, xb, dim);
  sel.offer_bulk(d, live ? key : kNoPos, K);
  return sel;
}

template <class Top>
__device__ __attribute__((noinline)) Top exact_batch_row_fn(Top sel, const float *qrow, const float4 *xr, uint32_t dim, bool live,
                                                            uint32_t key, int K) {
  float d = INFINITY;
  if (live) d = exact_pair<1>(qrow, xr, dim);
  sel.offer_bulk(d, live ? key : kNoPos, K);
  return sel;
}

// Up to 64 rows of a row-major table (one per lane, `cnt` of them live) against the query, with the ROWS FETCHED BY THE
// WHOLE WAVE: a lane reading its own row asks the texture unit for 64 different cache lines per load instruction (one
// 16-byte piece of each) — 2 048 line requests for 64 rows of 128 floats, and the address pipe, not the arithmetic, set
// the pace of the coarse select.  Here four lanes fetch 64 consecutive bytes of a row (16 rows per instruction, 512
// requests in all) straight into LDS (LDS-DMA: no registers in between, two chunks of 16 dimensions in flight), and
// every lane then runs the reference's chain (utils.rs:28-30) over its own row as before.  A DMA instruction writes
// lane l's 16 bytes at LDS offset 16 l, so a row's four pieces sit 64 bytes apart from the next row's — a lane per row
// reading piece p would hit the same banks eight times over; lane l therefore fetches piece (l & 3) ^ ((l >> 3) & 3)
// and row r reads its piece p from slot 4 r + (p ^ ((r >> 1) & 3)): conflict free.
// dim % 16 == 0; stage: kStageFloats floats of LDS per wave (a ring of two chunks); the waits are counted by hand
// (the copies are inline asm, invisible to the compiler's own counting: mfma_bf16.hpp).
constexpr uint32_t kStageFloats = 2048;
template <class Top>
__device__ __attribute__((noinline)) Top exact_batch_rows_staged_fn(Top sel, const float *qrow, const float4 *rows, uint32_t nrows, uint32_t dim,
                                                                    uint32_t cnt, uint32_t pos, int K, float *stage) {
  const uint32_t lane = threadIdx.x & 63u, r0 = lane >> 2, piece = (lane & 3u) ^ ((lane >> 3) & 3u);
  const uint32_t nquad = dim >> 2, nch = nquad >> 2;
  const VI_AS_LDS vf4 *xq = (const VI_AS_LDS vf4 *)(const VI_AS_LDS float *)qrow;
  const uint32_t sbase = (uint32_t)(size_t)(VI_AS_LDS float *)stage;
  const float4 *src[4];  // piece `piece` of the rows r0 + 16 j (rows beyond cnt: the last live one again)
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j)
    src[j] = rows + (size_t)min((uint32_t)__shfl((int)pos, (int)min(r0 + 16u * j, cnt - 1u)), nrows - 1u) * nquad + piece;
  auto issue = [&](uint32_t c) {  // chunk c -> ring slot c & 1: four copies of 1 KiB
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) glds16_at(src[j] + 4u * c, sbase + (c & 1u) * 4096u + j * 1024u);
  };
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (whatever the caller left in flight: the counts below are this function's)
  issue(0u);
  if (nch > 1u) issue(1u);
  const uint32_t swz = (lane >> 1) & 3u;
  float acc = 0.0f;
#pragma unroll 1
  for (uint32_t c = 0; c < nch; ++c) {
    if (c + 1u < nch) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const VI_AS_LDS vf4 *rd = (const VI_AS_LDS vf4 *)((const VI_AS_LDS float *)stage + (c & 1u) * 1024u + lane * 16u);
    const vf4 x0 = rd[0u ^ swz], x1 = rd[1u ^ swz], x2 = rd[2u ^ swz], x3 = rd[3u ^ swz];
    const vf4 q0 = xq[4u * c], q1 = xq[4u * c + 1u], q2 = xq[4u * c + 2u], q3 = xq[4u * c + 3u];
    // (differences and squares four at a time — packed f32 instructions round every component as the scalar ones do;
    //  the sum stays the reference's sequential chain)
#define VI_PK_QUAD(QQ, XX)                                                         \
  {                                                                                \
    const vf2 ta = pk_sub_f32(QQ.xy, XX.xy), tb = pk_sub_f32(QQ.zw, XX.zw);        \
    const vf2 sa = ta * ta, sb = tb * tb;                                          \
    acc = acc + sa.x; acc = acc + sa.y; acc = acc + sb.x; acc = acc + sb.y;        \
  }
    VI_PK_QUAD(q0, x0) VI_PK_QUAD(q1, x1) VI_PK_QUAD(q2, x2) VI_PK_QUAD(q3, x3)
#undef VI_PK_QUAD
    if (c + 2u < nch) {  // the slot's values are in registers (the chain above consumed them): refill it
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      issue(c + 2u);
    }
  }
  const bool live = lane < cnt && pos < nrows;
  sel.offer_bulk(live ? acc : INFINITY, live ? pos : kNoPos, K);
  return sel;
}

template <class Top>
__device__ __attribute__((noinline)) Top exact_batch_bf16_fn(Top sel, const float *qrow, const uint4 *xh, uint32_t dim, bool live,
                                                             uint32_t key, int K) {
  float d = INFINITY;
  if (live) d = exact_pair_bf16(qrow, xh, dim);
  sel.offer_bulk(d, live ? key : kNoPos, K);
  return sel;
}


// One wave: top-K of query q under (exact distance, (g << 26) | position) from its G group records at gbase.
// Leaves the result in `sel` (entry e of lane i = result 64e + i, key kNoPos when there are fewer than K).
// Top = FastTopK (K <= 64) or FastTop128 (K <= 128: the Faiss-style harness asks for 100 neighbours), wave_sort.hpp.
// FILT: a vector is offered only if its allow bit is set — the rank kernels saw the excluded slots with the pad norm, so
// they sit in no bound; a sub-block queued for its allowed members is re-evaluated without the others.
template <class Top, bool FILT = false>
__device__ __forceinline__ void select_body(const SelectCommon &c, uint32_t q, size_t gbase, uint32_t G, uint32_t P,
                                            const ProbeRegs &pr, uint32_t K, int lane, uint32_t *pick, float4 *tcache,
                                            uint32_t *lcache, float *qlds, Top &sel, uint32_t *qbytes = nullptr) {
  const uint64_t below = (1ull << lane) - 1ull;
  const QueryFrame f = query_frame<true>(c, q, lane, qlds, qbytes);
  uint32_t npick = 0, n_exact = 0, n_scanned = 0, n_full = 0, n_sub = 0;
  Top s1;
  float thr = INFINITY;
  sel.init();
  const float *qrow = qlds;  // (visible to the wave after the wave_lds_sync of stage 0)
  auto exact_offer = [&](bool live, uint32_t r, uint32_t pos) {  // one (probe rank, position) per lane
    const uint32_t fb = (uint32_t)__shfl((int)pr.fb, (int)r);
    const uint32_t g = (uint32_t)__shfl((int)pr.g, (int)r);
    const uint32_t len = (uint32_t)__shfl((int)pr.len, (int)r);
    live = live && pos < len && !(c.xmode & 1u);
    if constexpr (FILT) {  // slot = (fb + pos / 64) * 64 + pos % 64: the word is shared by the 16 lanes of a sub-block
      const uint32_t p = live ? pos : 0u;
      live = live && ((c.allow[fb + p / kWave] >> (p % kWave)) & 1ull) != 0ull;
    }
    n_exact += (uint32_t)__popcll(__ballot(live));
    if (c.u8_nat && f.q_bytes)
      sel = exact_batch_u8_int_fn(sel, qbytes, f.qn_int, c.u8_nat + ((size_t)(fb + (live ? pos : 0u) / kWave) * (c.dq / 4)) * kWave + (pos % kWave),
                                  c.dim, live, (g << kPosBits) | pos, (int)K);
    else if (c.u8_nat)
      sel = exact_batch_u8_fn(sel, qrow, c.u8_nat + ((size_t)(fb + (live ? pos : 0u) / kWave) * (c.dq / 4)) * kWave + (pos % kWave), c.dim,
                              live, (g << kPosBits) | pos, (int)K);
    else if (c.hi_nat)
      sel = exact_batch_bf16_fn(sel, qrow, c.hi_nat + ((size_t)(fb + (live ? pos : 0u) / kWave) * (c.dq / 2)) * kWave + (pos % kWave),
                                c.dim, live, (g << kPosBits) | pos, (int)K);
    else
      sel = exact_batch_fn(sel, qrow, c.blocks + ((size_t)(fb + (live ? pos : 0u) / kWave) * c.dq) * kWave + (pos % kWave),
                           c.dim, live, (g << kPosBits) | pos, (int)K);
  };
  auto drain = [&]() { drain_pick(c, pick, npick, lane, exact_offer); };
  // The pair records of the groups flagged `want`.  mode 0: the minima go to the running top-K of rank values (s1);
  // mode 1: every sub-block whose minimum is at or below thr is queued for exact evaluation.
  auto scan_groups = [&](bool want, uint32_t r, uint32_t seg, uint32_t hh, int mode) {
    scan_pair_records(c, pr, lane, want, r, seg, hh, n_scanned, [&](bool ok, float v, uint32_t j, uint32_t rr, uint32_t sub, uint32_t h2) {
      if (mode == 0) s1 = offer_bulk_fn(s1, ok ? v : INFINITY, ok ? j : kNoPos, (int)K);
      else push_sub(pick, npick, n_sub, lane, ok && !(v > thr), rr, sub, h2, drain);  // (!(v > thr): a NaN minimum is expanded, never skipped)
    });
  };

  // (diagnostic, VI_FILTER_STATS: s_memtime ticks per stage, summed over the queries into the stage clocks of ws.stats, kStatClocks)
  unsigned long long tk = c.dbg ? __builtin_amdgcn_s_memtime() : 0ull, tks[6] = {0, 0, 0, 0, 0, 0};
  auto lap = [&](int i) {
    if (c.dbg) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      tks[i] += now - tk;
      tk = now;
    }
  };
  // ---- stage 0: the first 256 group records go to LDS ----
  const GroupRecords gr{c, gbase, G, tcache, lcache};
  gr.fill(lane);
  lap(0);
  // ---- stage 1a: threshold (*) from the K-th smallest value of the group records (key = 4*group + slot);
  //      the groups' smallest values first: they shut the door on most of the others ----
  bool any_full = false;
  {
    s1.init();
    // The K-th smallest of the 4 G recorded values, with its keys.  Offering all of them costs a 64-lane sort per 64 values
    // (16 sorts at G = 256).  Instead: every lane's smallest group minimum belongs to a different sub-block, so the K-th
    // smallest of the 64 lane minima (ONE sort) bounds the K-th smallest of all; the values at or below that bound —
    // K to 2 K of them as a rule — are compacted through LDS and offered in one or two rounds.
    float U = INFINITY;
    if (K <= 64u) {
      float lm = INFINITY;
      for (uint32_t gb = 0; gb < G; gb += kWave) {
        const uint32_t gidx = gb + lane;
        lm = fminf(lm, gr.group_values(gidx, gidx < G).x);
      }
      uint64_t kk = pack_key(lm, (uint32_t)lane);
      wave_sort_u64(kk, lane);
      U = sortable_f32((uint32_t)(readlane_u64(kk, (int)K - 1) >> 32));  // (+inf or NaN: no bound, everything is offered)
    }
    uint32_t ncand = 0;
    bool overflow = !(U < INFINITY);
    if (!overflow) {
      for (uint32_t gb = 0; gb < G && !overflow; gb += kWave) {
        const uint32_t gidx = gb + lane;
        const bool live = gidx < G;
        const float4 T = gr.group_values(gidx, live);
        const float tv[4] = {T.x, T.y, T.z, T.w};
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const bool pass = live && !(tv[j] > U);
          const uint64_t m = __ballot(pass);
          if (!m) continue;
          const uint32_t cnt = (uint32_t)__popcll(m);
          if (ncand + cnt > kPickCap / 2u) { overflow = true; break; }
          if (pass) {
            const uint32_t at = ncand + (uint32_t)__popcll(m & below);
            pick[2u * at] = __float_as_uint(tv[j]);
            pick[2u * at + 1u] = 4u * gidx + j;
          }
          ncand += cnt;
        }
      }
      wave_lds_sync();
    }
    if (!overflow) {
      for (uint32_t c0 = 0; c0 < ncand; c0 += kWave) {
        const bool live = c0 + lane < ncand;
        const float v = live ? __uint_as_float(pick[2u * (c0 + lane)]) : INFINITY;
        s1 = offer_bulk_fn(s1, v, live ? pick[2u * (c0 + lane) + 1u] : kNoPos, (int)K);
      }
      wave_lds_sync();  // (pick is reused by the stages below)
    } else {
      s1.init();
      for (uint32_t gb = 0; gb < G; gb += kWave) {
        const uint32_t gidx = gb + lane;
        const bool live = gidx < G;
        s1 = offer_bulk_fn(s1, gr.group_values(gidx, live).x, live ? 4u * gidx : kNoPos, (int)K);
      }
      for (uint32_t gb = 0; gb < G; gb += kWave) {
        const uint32_t gidx = gb + lane;
        const bool live = gidx < G;
        const float4 T = gr.group_values(gidx, live);
        s1 = offer_bulk_fn(s1, T.y, live ? 4u * gidx + 1u : kNoPos, (int)K);
        s1 = offer_bulk_fn(s1, T.z, live ? 4u * gidx + 2u : kNoPos, (int)K);
        s1 = offer_bulk_fn(s1, T.w, live ? 4u * gidx + 3u : kNoPos, (int)K);
      }
    }
    thr = rank_threshold(c, f, s1.kth((int)K));
    for (uint32_t gb = 0; gb < G; gb += kWave) {  // is any group's 4th value at or below it?
      const uint32_t gidx = gb + lane;
      const float4 T = gr.group_values(gidx, gidx < G);
      any_full = any_full || __ballot(gidx < G && T.w <= thr) != 0ull;  // (distrust: thr = inf, stage 1b is moot)
    }
  }
  lap(1);
  // ---- stage 1b: neighbours concentrated in few groups hide behind the 4 listed minima and leave the bound
  //      loose; the pair records of those groups list every sub-block minimum.  Their values REPLACE the
  //      group's own (which are among them, so they must not be counted twice): drop the group's entries from
  //      the running top-K, then offer its pair records ----
  if (any_full && !f.distrust && !(c.xmode & 4u)) {
    {
      bool keep[2] = {false, false};
#pragma unroll
      for (int e = 0; e < Top::kEntries; ++e) {
        const uint32_t key = s1.ent_p(e);
        const bool mine = key != kNoPos && (uint32_t)(64 * e + lane) < K;  // entries beyond the K-th are not needed
        keep[e] = mine && !(gr.group_values(mine ? (key >> 2) : 0u, true).w <= thr);
      }
      s1.rebuild(keep[0], keep[1], (int)K);  // the survivors close ranks
    }
    for (uint32_t gb = 0; gb < G; gb += kWave) {
      const uint32_t gidx = gb + lane;
      const bool live = gidx < G;
      uint32_t r, seg, hh;
      gr.group_place(gidx, live, r, seg, hh);
      scan_groups(live && gr.group_values(gidx, live).w <= thr, r, seg, hh, 0);
    }
    thr = fminf(thr, rank_threshold(c, f, s1.kth((int)K)));
  }
  lap(2);
  // ---- stage 2: exact re-evaluation of every sub-block whose minimum is at or below thr; such a sub-block sits in a
  //      group whose smallest minimum is at or below thr ----
  for (uint32_t gb = 0; gb < G; gb += kWave) {
    const uint32_t gidx = gb + lane;
    const bool live = gidx < G;
    uint32_t r, seg, hh;
    gr.group_place(gidx, live, r, seg, hh);
    const float4 T = gr.group_values(gidx, live);
    n_full += (uint32_t)__popcll(__ballot(live && T.w <= thr));
    scan_groups(live && !(T.x > thr) && !(c.xmode & 2u), r, seg, hh, 1);
  }
  lap(3);
  drain();
  lap(4);
  if (c.dbg && lane == 0 && (q & c.dbg_mask) == 0u) {
#pragma unroll
    for (int i = 0; i < 5; ++i) atomicAdd(&c.dbg[kStatClocks + i], tks[i]);
    atomicAdd(&c.dbg[kStatSelExact], (unsigned long long)n_exact);
    atomicAdd(&c.dbg[kStatSelScanned], (unsigned long long)n_scanned);
    atomicAdd(&c.dbg[kStatSelQueriesFull], (unsigned long long)(any_full ? 1u : 0u));
    atomicAdd(&c.dbg[kStatSelFullGroups], (unsigned long long)n_full);
    atomicAdd(&c.dbg[kStatSelSubBlocks], (unsigned long long)n_sub);
  }
}

struct SelectArgs {
  SelectCommon c;
  uint32_t nq, P, k;
  ListProbes lp;
  const uint64_t *ext_ids;
  float *D;
  int64_t *I;
  uint64_t *tie, *slots;
  uint32_t *counts;
};

// one wave per query: top-k over its probed lists in the reference's stable order (ivf_index.rs:264-274)
template <class Top, bool FILT = false>
__global__ void __launch_bounds__(256, 4) select_kernel(SelectArgs a) {
  __shared__ uint32_t s_pick[4][kPickCap], s_lcache[4][kCacheG];
  __shared__ float4 s_tcache[4][kCacheG];
  __shared__ __attribute__((aligned(16))) uint32_t s_qbytes[4][64];  // the 4 queries as bytes (8-bit lists, D <= 256)
  extern __shared__ __attribute__((aligned(16))) float s_qrows[];  // the 4 query rows of the workgroup: 4 x dim floats
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x * 4 + wave;
  if (q >= a.nq) return;
  uint32_t mylist;
  const ProbeRegs pr = load_probe_regs(a.lp, a.c.gq, q, a.P, lane, &mylist);
  Top sel;
  select_body<Top, FILT>(a.c, q, a.lp.qoff[q], a.lp.qtot[q], a.P, pr, a.k, lane, s_pick[wave], s_tcache[wave],
                   s_lcache[wave], s_qrows + (size_t)wave * a.c.dim, sel, s_qbytes[wave]);
  // entry e of lane i holds result 64e + i: map the candidate-order rank g back to the probe rank r
  uint32_t found = 0;
  // probe rank of candidate-order rank g: lane r pushes r to lane g(r) (the ranks of a query's probes are a permutation of
  // 0 .. found-1; lanes without a probe push to themselves, at or above found) — one crossbar push instead of a readlane
  // and a compare per probe and result entry
  const uint32_t inv = (uint32_t)__builtin_amdgcn_ds_permute((int)(4u * (mylist != kNoPos ? pr.g : (uint32_t)lane)), lane);
#pragma unroll
  for (int e = 0; e < Top::kEntries; ++e) {
    const uint32_t key = sel.ent_p(e), idx = 64u * (uint32_t)e + (uint32_t)lane;
    const uint32_t g = key >> kPosBits, pos = key & kPosMask;
    const uint32_t r = (uint32_t)__shfl((int)inv, (int)(g & 63u));
    const bool have = idx < a.k && key != kNoPos;
    found += (uint32_t)__popcll(__ballot(have));
    const uint32_t fbk = (uint32_t)__shfl((int)pr.fb, (int)r);
    if (idx < a.k) {
      const size_t o = (size_t)q * a.k + idx;
      if (have) {
        const uint64_t gslot = (uint64_t)fbk * kWave + pos;
        a.D[o] = sel.ent_d(e);
        a.I[o] = (int64_t)a.ext_ids[gslot];
        if (a.tie) a.tie[o] = ((uint64_t)g << 32) | pos;
        if (a.slots) a.slots[o] = gslot;
      } else {
        a.D[o] = INFINITY;
        a.I[o] = -1;
        if (a.tie) a.tie[o] = ~0ull;
        if (a.slots) a.slots[o] = ~0ull;
      }
    }
  }
  if (a.counts && lane == 0) a.counts[q] = found;
}

struct CoarseSelectArgs {
  SelectCommon c;  // blocks = centroid table
  uint32_t nq, P, nlists, segb, recs;  // recs = group records per query
  const uint32_t *list_shard, *list_len;
  uint32_t *probes, *gorder, *cnt;
  const float4 *cent_rows;  // the table row-major (rows_from_blocks_kernel) for single-row re-evaluation
  // record counts of the list phase (what pair_groups_kernel computes otherwise)
  uint32_t list_segb0;
  uint32_t *rel, *qtot;
  uint32_t staged;  // single rows fetched by the whole wave through LDS (exact_batch_rows_staged_fn, D % 16 == 0), else a row per lane
  uint32_t *pair_rank;  // where the pair stands among the pairs of its (list, sub-bin) — the value its histogram
                        // increment returns — so that the grouping's scatter needs no atomics of its own; or null
};

// The tail of both coarse selects, one probe per lane r < P: lane r's selected list `mylist` (kNoPos from `found` on) goes
// out with its candidate-order rank (shard visiting order; lane_order: the lane itself, an ablation), is counted in the
// per-list histogram as coarse_merge_kernel counts it, and leaves what that increment returned in pair_rank; then the
// record offsets of the list phase: 2 group records per (probe, segment), scanned over the wave into rel, their total
// into qtot (group_prepare_kernel turns the per-query totals into offsets)
__device__ __forceinline__ void write_probe_row(const CoarseSelectArgs &a, uint32_t q, int lane, uint32_t mylist, uint32_t found,
                                                bool lane_order) {
  const uint32_t g = lane_order ? (uint32_t)lane : probe_candidate_order(lane, found, mylist, a.list_shard);
  if ((uint32_t)lane < a.P) {
    a.probes[(size_t)q * a.P + lane] = mylist;
    a.gorder[(size_t)q * a.P + lane] = g;
    if (mylist != kNoPos && a.list_len[mylist] > 0) {
      const uint32_t before = atomicAdd(&a.cnt[subbin_index(mylist, q & (kSubBins - 1), a.nlists)], 1u);
      if (a.pair_rank) a.pair_rank[(size_t)q * a.P + lane] = before;
    }
  }
  uint32_t ng = 0;
  if (mylist != kNoPos) {
    uint32_t sb;
    ng = 2u * list_segments(a.list_len[mylist], a.list_segb0, &sb);
  }
  const uint32_t ig = wave_incl_scan_u32(ng);
  if ((uint32_t)lane < a.P) a.rel[(size_t)q * a.P + lane] = ig - ng;
  if (lane == 63) a.qtot[q] = ig;
}

// one wave per query: the P nearest centroids in (distance, centroid index) order (the reference's stable
// sort, ivf_index.rs:205-220), then shard visiting order + histogram as in coarse_merge_kernel
__global__ void __launch_bounds__(256, 4) coarse_select_kernel(CoarseSelectArgs a) {
  __shared__ uint32_t s_pick[4][kPickCap], s_lcache[4][kCacheG];
  __shared__ float4 s_tcache[4][kCacheG];
  __shared__ __attribute__((aligned(16))) float s_q[4][kNarrowDim];  // (the coarse step runs here only for D <= 128)
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x * 4 + wave;
  if (q >= a.nq) return;
  ProbeRegs pr{0u, 0u, 0u, 0u, 0u, 1u, 0u};
  if (lane == 0) {
    pr.ng = a.recs; pr.len = a.nlists; pr.segb = a.segb;
    pr.boff = (q / a.c.gq) * (a.recs / 2u) * seg_records(a.segb) * (2u * a.c.gq) + (q % a.c.gq);  // pairs = iota: the query's own position
  }
  FastTopK sel;
  select_body<FastTopK>(a.c, q, (size_t)q * a.recs, a.recs, 1u, pr, a.P, lane, s_pick[wave], s_tcache[wave],
              s_lcache[wave], s_q[wave], sel);
  const uint32_t found = (uint32_t)__popcll(__ballot((uint32_t)lane < a.P && sel.ent_p(0) != kNoPos));
  const uint32_t mylist = (uint32_t)lane < found ? sel.ent_p(0) : kNoPos;
  write_probe_row(a, q, lane, mylist, found, false);
}

// The coarse table up to 256 blocks (16 384 centroids): the rank kernel leaves two records per (block, lane half) —
// (minimum with its row, second minimum) of its four 8-row sub-blocks — and this kernel reads ALL of a query's records at
// once (<= 16 per lane): the P-th smallest minimum bounds the P-th distance (the minima belong to different centroids);
// a sub-block whose minimum is at or below the threshold (*) contributes that ONE row to the exact re-evaluation, or
// all 8 when its second minimum is at or below the threshold too.  No group records, no refinement rounds: at P = 32
// about 40 exact distances per query decide the probe list.
__global__ void __launch_bounds__(256) coarse_select_direct_kernel(CoarseSelectArgs a) {
  __shared__ uint32_t s_pick[4][kPickCap];
  __shared__ __attribute__((aligned(16))) float s_q[4][kNarrowDim];  // (the coarse step runs here only for D <= 128)
  __shared__ __attribute__((aligned(16))) float s_stage[4][kStageFloats];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  const uint32_t q = blockIdx.x * 4 + wave;
  if (q >= a.nq) return;
  const SelectCommon &c = a.c;
  uint32_t *pick = s_pick[wave];
  float *qlds = s_q[wave];
  const uint64_t below = (1ull << lane) - 1ull;
  // (diagnostic, VI_FILTER_STATS=2: s_memtime ticks per stage, summed over the queries into the stage clocks of ws.stats, kStatClocks)
  unsigned long long tk = c.dbg ? __builtin_amdgcn_s_memtime() : 0ull, tks[6] = {0, 0, 0, 0, 0, 0};
  auto lap = [&](int i) {
    if (c.dbg) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      tks[i] += now - tk;
      tk = now;
    }
  };
  const QueryFrame f = query_frame<true>(c, q, lane, qlds, nullptr);
  wave_lds_sync();
  lap(0);
  const uint32_t K = a.P, nblk = (a.nlists + kWave - 1) / kWave, nrec = 4u * nblk;  // records: (block, tile, lane half)
  constexpr uint32_t kPer = kDirectBlocks * 4 / kWave;  // records per lane
  // (min of sub-block 0 with its row, its second min, the same of sub-block 1)
  auto record = [&](uint32_t i) {
    const uint32_t rec = i * kWave + lane;  // block rec >> 2, tile (rec >> 1) & 1, lane half rec & 1
    float4 r = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    if (rec < nrec) r = c.brec[(size_t)q * nrec + rec];
    return r;
  };
  // bound of the K-th distance: every lane's smallest minimum belongs to a different centroid, so K centroids are at
  // or below the K-th smallest of the 64 lane minima — one 64-lane sort instead of a running top-K over all the minima
  // (K <= 64; the bound sits a few ranks above the exact K-th minimum, which costs a few more single-row evaluations)
  float lm = INFINITY;
  float rb1[kPer][2], rb2[kPer][2];  // (kept for the flags below: 16 registers; a second read from L2 was a round trip per query)
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i) {
    rb1[i][0] = rb1[i][1] = rb2[i][0] = rb2[i][1] = INFINITY;
    if (i * kWave < nrec) {
      const float4 r = record(i);
      lm = min3_raw(lm, r.x, r.z);
      rb1[i][0] = r.x; rb2[i][0] = r.y; rb1[i][1] = r.z; rb2[i][1] = r.w;
    }
  }
  FastTopK s1;
  s1.init();
  s1 = offer_bulk_fn(s1, lm, (uint32_t)lane, (int)K);
  const float thr = rank_threshold(c, f, s1.kth((int)K));
  lap(1);
  FastTopK sel;
  sel.init();
  uint32_t npick = 0;
  // sub-block s (0/1) of record rec: its first row is register 8s of tile t of lane half h
  auto sub_row = [&](uint32_t rec, uint32_t s, uint32_t e) {
    return (rec >> 2) * kWave + subblock_vector(8u * s + e, (rec >> 1) & 1u, rec & 1u, c.image_order != 0u);
  };
  uint32_t n_single = 0, n_whole = 0;  // (VI_FILTER_STATS=2: rows evaluated alone / whole 8-row sub-blocks)
  auto drain_singles = [&]() {
    while (npick > 0) {
      const uint32_t cnt = npick >= (uint32_t)kWave ? (uint32_t)kWave : npick;
      npick -= cnt;
      n_single += cnt;
      bool live = (uint32_t)lane < cnt;
      const uint32_t pos = live ? pick[npick + lane] : 0u;
      if (a.staged) {  // one centroid per lane, the rows fetched by the whole wave
        if (!(c.xmode & 1u)) sel = exact_batch_rows_staged_fn(sel, qlds, a.cent_rows, a.nlists, c.dim, cnt, pos, (int)K, s_stage[wave]);
      } else {  // one centroid per lane, each its own whole cache lines
        live = live && pos < a.nlists && !(c.xmode & 1u);
        sel = exact_batch_row_fn(sel, qlds, a.cent_rows + (size_t)(live ? pos : 0u) * (c.dim / 4), c.dim, live, pos, (int)K);
      }
    }
  };
  // Which rows go to the exact evaluation: of a sub-block whose minimum is at or below thr the row of that minimum, all
  // eight when its second minimum is too.  A lane counts the rows of its eight sub-blocks, one scan over the wave gives
  // every lane its place in the list, one LDS round writes them (a ballot, a count and an LDS round per sub-block column
  // and kind — sixteen of each — were a fifth of the kernel).  More rows than the list holds (a distrusted query flags
  // everything): the ballot loop below, which drains the list as it fills.
  bool listed = false;
  if (!(c.xmode & 16u)) {
    // 2 bits per sub-block in cls: 0 none, 1 the row of the minimum, 2 all eight; 4 bits per sub-block for that row,
    // sub-blocks 0-15 in rows_lo and 16-31 in rows_hi (the word is chosen at compile time in the flag loop: a runtime
    // index into a register array would put it in scratch)
    constexpr uint32_t kSub = 2u * kPer, kSubPerWord = 16u;  // sub-blocks per lane; per rows word
    static_assert(2u * kSub <= 64u, "cls holds 2 bits for each of a lane's sub-blocks");
    static_assert(kSub <= 2u * kSubPerWord && 4u * kSubPerWord <= 64u, "rows_lo / rows_hi hold 4 bits for each sub-block");
    uint64_t cls = 0, rows_lo = 0, rows_hi = 0;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPer; ++i)
      if (i * kWave < nrec) {
        const uint32_t rec = i * kWave + lane;
#pragma unroll
        for (uint32_t s2 = 0; s2 < 2; ++s2) {
          const uint32_t sb = 2u * i + s2;
          const bool cand = rec < nrec && !(rb1[i][s2] > thr);
          const bool all8 = cand && (!(rb2[i][s2] > thr) || f.distrust);
          const uint64_t k = all8 ? 2u : (cand ? 1u : 0u);
          cls |= k << (2u * sb);
          const uint64_t row = __float_as_uint(rb1[i][s2]) & 7u;
          if (sb < kSubPerWord) rows_lo |= row << (4u * sb);
          else rows_hi |= row << (4u * (sb - kSubPerWord));
          mine += all8 ? 8u : (cand ? 1u : 0u);
        }
      }
    const uint32_t incl = wave_incl_scan_u32(mine);
    const uint32_t total = readlane_u(incl, 63);
    if (total <= kPickCap) {
      uint32_t at = incl - mine;
      uint64_t left = cls;
      // (a lane flags 0.7 of its 8 sub-blocks on average: as many rounds as the busiest lane has flags — three or four —
      //  each lane taking its next flagged sub-block, instead of eight rounds of mostly idle lanes)
      while (__ballot(left != 0u)) {
        if (left != 0u) {
          const uint32_t sb = (uint32_t)__builtin_ctzll(left) >> 1;
          const uint32_t k = (uint32_t)(left >> (2u * sb)) & 3u, rec = (sb >> 1) * kWave + (uint32_t)lane;
          left &= ~(3ull << (2u * sb));
          if (k == 1u) {
            const uint64_t rows = sb < kSubPerWord ? rows_lo : rows_hi;
            pick[at] = sub_row(rec, sb & 1u, (uint32_t)(rows >> (4u * (sb % kSubPerWord))) & 7u);
            at += 1u;
          } else {
#pragma unroll
            for (uint32_t e = 0; e < 8u; ++e) pick[at + e] = sub_row(rec, sb & 1u, e);
            at += 8u;
            n_whole += 1u;  // (per lane here; summed below when the counters are on)
          }
        }
      }
      npick = total;
      listed = true;
      wave_lds_sync();
      if (c.dbg) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n_whole += (uint32_t)__shfl_xor((int)n_whole, o);
      }
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < kPer; ++i)
    if (i * kWave < nrec && !(c.xmode & 16u) && !listed) {
      const uint32_t rec = i * kWave + lane;
      const float4 Ri = record(i);
      const float b1[2] = {Ri.x, Ri.z}, b2[2] = {Ri.y, Ri.w};
#pragma nounroll  // (a cold path: unrolled, its inlined exact rounds would double the kernel's code)
      for (uint32_t s2 = 0; s2 < 2; ++s2) {
        const bool cand = rec < nrec && !(b1[s2] > thr);
        const bool all8 = cand && (!(b2[s2] > thr) || f.distrust);
        const bool one = cand && !all8;
        uint64_t m = __ballot(one);
        if (m) {
          const uint32_t cnt = (uint32_t)__popcll(m);
          if (npick + cnt > kPickCap) drain_singles();
          if (one) pick[npick + (uint32_t)__popcll(m & below)] = sub_row(rec, s2, __float_as_uint(b1[s2]) & 7u);
          npick += cnt;
          wave_lds_sync();
        }
        m = __ballot(all8);
        if (m) {  // all 8 rows of the sub-block: into the same list (they used to wait for rounds of their own — a second exact
          // round and a second merge per query for 1.6 sub-blocks on average, a third of the kernel's instructions)
          // (32 lanes at a time: their 256 rows fill the list exactly — a distrusted query flags every sub-block)
#pragma unroll
          for (uint32_t half = 0; half < 2u; ++half) {
            const uint64_t mh = m & (half ? 0xFFFFFFFF00000000ull : 0x00000000FFFFFFFFull);
            if (!mh) continue;
            const uint32_t cnt = 8u * (uint32_t)__popcll(mh);
            if (npick + cnt > kPickCap) drain_singles();
            if (all8 && ((uint32_t)lane >> 5) == half) {
              const uint32_t at = npick + 8u * (uint32_t)__popcll(mh & below);
#pragma unroll
              for (uint32_t e = 0; e < 8u; ++e) pick[at + e] = sub_row(rec, s2, e);
            }
            npick += cnt;
            n_whole += cnt >> 3;
            wave_lds_sync();
          }
        }
      }
    }
  lap(2);
  drain_singles();
  lap(3);
  const uint32_t found = (uint32_t)__popcll(__ballot((uint32_t)lane < a.P && sel.ent_p(0) != kNoPos));
  const uint32_t mylist = (uint32_t)lane < found ? sel.ent_p(0) : kNoPos;
  write_probe_row(a, q, lane, mylist, found, (c.xmode & 32u) != 0u);
  lap(4);
  if (c.dbg && lane == 0 && (q & 63u) == 0u) {  // (every 64th query: 70 000 same-address atomics would be most of the kernel)
    for (int i = 0; i < 5; ++i) atomicAdd(&c.dbg[kStatClocks + i], tks[i]);
    atomicAdd(c.dbg + kStatSelExact, (unsigned long long)n_single);
    atomicAdd(c.dbg + kStatSelScanned, (unsigned long long)n_whole);
  }
}

}  // namespace

vi_status launch_list_select(SearchBatch &b, uint64_t k, const SelectFrame &f, const SelectOutputs &out) {
  const DeviceIndex &ix = b.ix;
  hipStream_t st = b.st();
  SelectArgs a{list_select_common(b, f), (uint32_t)b.nq, b.P, (uint32_t)k, list_probes(b), ix.ext_ids.p, out.D, out.I, out.tie, out.slots,
               out.counts};
  const size_t qsm = 4ull * ix.dim * sizeof(float);
  const dim3 grid((uint32_t)((b.nq + 3) / 4));
  if (b.flt) {  // an instantiation of its own: the unfiltered one keeps its registers and its four workgroups per CU
    a.c.allow = b.flt->allow.p;
    if (k <= 64) hipLaunchKernelGGL((select_kernel<FastTopK, true>), grid, dim3(256), qsm, st, a);
    else hipLaunchKernelGGL((select_kernel<FastTop128, true>), grid, dim3(256), qsm, st, a);
  } else if (k <= 64) {
    hipLaunchKernelGGL(select_kernel<FastTopK>, grid, dim3(256), qsm, st, a);
  } else {
    hipLaunchKernelGGL(select_kernel<FastTop128>, grid, dim3(256), qsm, st, a);
  }
  VI_HIP(hipGetLastError());
  return VI_OK;
}

vi_status launch_coarse_select(SearchBatch &b, uint32_t segb, uint32_t recs, bool direct) {
  const DeviceIndex &ix = b.ix;
  const EngineKnobs &kn = b.kn;
  SearchWorkspace &ws = b.ws();
  const uint32_t nq = (uint32_t)b.nq, P = b.P;
  hipStream_t st = b.st();
  // (both coarse selects keep what their histogram increment returns: the grouping's scatter ranks the pairs with it)
  VI_TRY(ws.pair_rank.reserve(b.nq * P));
  b.pair_rank_valid = true;
  CoarseSelectArgs a{select_common(b, (const float4 *)ix.centroids.blocks.p, kn.rank_bf16 && ix.centered ? ix.cent_xmax2_c : ix.cent_xmax2,
                                   kGroupQ), (uint32_t)nq, P, (uint32_t)ix.nlists, segb, recs, ix.list_shard.p, ix.list_len.p, ws.probes.p,
                     ws.gorder.p, ws.cnt.p, (const float4 *)ix.cent_rows.p, kn.segb0, ws.pair_rel.p, ws.qtot.p,
                     (ix.dim & 15u) ? 0u : 1u, ws.pair_rank.p};
  if (!kn.stats_coarse) a.c.dbg = nullptr;  // '2': count the coarse step
  a.c.xmode = kn.coarse_xmode;
  if (direct) a.c.e_scale += (float)(1.01 * std::ldexp(1.0, -20));  // the row index rides in 3 mantissa bits of the minima
  if (direct) hipLaunchKernelGGL(coarse_select_direct_kernel, dim3((uint32_t)((nq + 3) / 4)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(coarse_select_kernel, dim3((uint32_t)((nq + 3) / 4)), dim3(256), 0, st, a);
  VI_HIP(hipGetLastError());
  return VI_OK;
}

}  // namespace vi
