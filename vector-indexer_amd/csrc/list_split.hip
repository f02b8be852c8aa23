// list_split.hip — the split step of vi_indexer_rebalance (include/vi_amd.h, step 1b): every planned pair (donor list,
// receiver list) of one iteration at once.  The members of a donor are two-means'ed in place — nothing is copied out of
// the old index's resident blocks, no record is touched — and the two centres come back as the centroids of the donor and
// of the receiver.  Members are described as list_means_kernel takes them (ListMembers, device_index.hpp): a list's own
// blocks in their order (cur == nullptr: the first iteration of a call), or the ordinals cur[seg[l] .. seg[l + 1])
// through refine_slot_of_ordinal.  Every rule that is plain arithmetic is rebalance_rules.hpp's.
//
//   split_farthest_kernel  lane = member, grid = pairs x chunks of 256 members.  The member's distance to one centre — the scalar
//                          chain of the coarse step, column after column — the key "distance bits above the inverted
//                          position", the wave's maximum of it by shuffles, one 64-bit atomicMax per wave into the pair's
//                          word.  Launched for seed a (centre = the donor's new centroid) and again for seed b (centre =
//                          the member seed a's key names; the block of the pair's first members writes it out as ca).
//   split_side_kernel      the same shape with two centres and two chains: one byte per member, 1 = cb strictly nearer.
//                          In the first inner iteration cb is the member seed b's key names, and is written out.
//   split_means_kernel     list_means_kernel's shape — one wave per (pair, 64 columns), 64 members at a time through the
//                          LDS tile, lane = column on the way out — with two accumulators: a member is added to the
//                          chain of its side and skipped by the other, so each side's chain runs over its own members
//                          only, in list order.  It writes the two counts, the two centres in place (each wave owns its
//                          columns of them) and a word that says whether any bit of them changed.  A side without a
//                          member leaves both centres as they are.
// A centre is read as an LDS broadcast, 1024 columns of it at a time, so any dimension fits the static 4 / 8 KiB.  On the
// identity path a wave's 64 members are one old block and every load instruction is one contiguous 1 KiB row of it.
// The inner loop is the host's (device_split_lists): one read-back of three words per pair after every inner iteration
// decides which pairs go on; a pair that has stopped is passed over by the kernels (active[pair] == 0).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_index.hpp"
#include "rebalance_rules.hpp"
#include "refine_rules.hpp"
#include "search_internal.hpp"

namespace vi {
namespace {

constexpr int kWave = 64;
constexpr uint32_t kSplitThreads = 256;               // members of one block of the farthest and side kernels
constexpr uint32_t kCenQuads = 256;                   // quads of a centre staged in LDS at a time
constexpr uint32_t kMeanCols = 64;                    // as list_means_kernel's
constexpr uint32_t kMeanQuads = kMeanCols / 4;
constexpr uint32_t kMeanStride = kMeanCols + 4;

struct SplitArgs {
  ListMembers m;
  uint32_t npairs, chunks;                 // chunks: blocks of kSplitThreads members per pair in the farthest and side grids
  const uint32_t *donor;                   // per pair: its donor list
  const uint32_t *active;                  // per pair: 0 = passed over
  const uint32_t *side_off;                // per pair: first byte of its members' sides
  float *cen_a, *cen_b;                    // npairs x dim: ca and cb
  uint8_t *side;
  uint32_t *counts;                        // per pair: members of side 0, of side 1
  uint32_t *changed;                       // per pair: non-zero once a bit of ca or cb changed
};

// the members of pair p's donor d — never more than the host planned side bytes for
__device__ inline uint32_t member_count(const SplitArgs &a, uint32_t p, uint32_t d) {
  const ListMembers &m = a.m;
  return min(m.cur ? m.seg[d + 1] - m.seg[d] : m.old_len[d], a.side_off[p + 1] - a.side_off[p]);
}
__device__ inline uint64_t member_slot(const ListMembers &m, uint32_t l, uint32_t pos) {
  return m.cur ? refine_slot_of_ordinal(m.prefix, m.first_block, m.nlists, m.cur[m.seg[l] + pos]) : refine_slot(m.first_block[l], pos);
}
// quad 0 of a slot's vector; quad q lies q * 64 float4 further on
__device__ inline const float4 *slot_quads(const ListMembers &m, uint64_t slot) { return m.blocks + ((slot >> 6) * m.dq) * kWave + (slot & 63u); }

// quads [q0, q0 + nq) of a centre into LDS, zero beyond dim: of `row` (dim floats) ...
__device__ inline void stage_row(float *lds, const float *row, uint32_t q0, uint32_t nq, uint32_t dim) {
  for (uint32_t i = threadIdx.x; i < nq * 4u; i += kSplitThreads) {
    const uint32_t col = q0 * 4u + i;
    lds[i] = col < dim ? row[col] : 0.0f;
  }
}
// ... or of the vector at `member`; `out` (optional): the row the same values are written to
__device__ inline void stage_member(float *lds, const float4 *member, float *out, uint32_t q0, uint32_t nq, uint32_t dim) {
  const float *base = reinterpret_cast<const float *>(member);
  for (uint32_t i = threadIdx.x; i < nq * 4u; i += kSplitThreads) {
    const uint32_t col = q0 * 4u + i;
    float v = 0.0f;
    if (col < dim) {
      v = base[(size_t)(col >> 2) * (kWave * 4u) + (col & 3u)];
      if (out) out[col] = v;
    }
    lds[i] = v;
  }
}

// the chain goes on over quads [q0, q0 + nq) of the member at src against the staged centre.  Columns beyond dim are
// +0.0 on both sides (the blocks are zero padded up to dq, the staged centre above): they add +0.0 to a chain that is
// never negative, which changes no bit of it.
__device__ inline float chain_quads(float acc, const float4 *src, const float *cen, uint32_t q0, uint32_t nq) {
#pragma unroll 4
  for (uint32_t q = 0; q < nq; ++q) {
    const float4 v = src[(size_t)(q0 + q) * kWave];
    const float4 c = *reinterpret_cast<const float4 *>(&cen[4u * q]);
    acc = rebalance_dist_add(acc, v.x, c.x);
    acc = rebalance_dist_add(acc, v.y, c.y);
    acc = rebalance_dist_add(acc, v.z, c.z);
    acc = rebalance_dist_add(acc, v.w, c.w);
  }
  return acc;
}

__global__ void __launch_bounds__(kSplitThreads) split_farthest_kernel(SplitArgs a, const uint64_t *from_key, uint64_t *key_out) {
  __shared__ __attribute__((aligned(16))) float cen[kCenQuads * 4];
  const uint32_t p = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks, d = a.donor[p], dim = a.m.dim, dq = a.m.dq;
  const uint32_t count = member_count(a, p, d), base = chunk * kSplitThreads;
  if (base >= count) return;  // (block-uniform)
  const uint32_t pos = base + threadIdx.x;
  const bool valid = pos < count;
  const float4 *src = slot_quads(a.m, valid ? member_slot(a.m, d, pos) : 0);  // (read only where valid)
  const float *row = from_key ? nullptr : a.cen_a + (size_t)p * dim;
  const float4 *seed = from_key ? slot_quads(a.m, member_slot(a.m, d, min(rebalance_key_pos(from_key[p]), count - 1))) : nullptr;
  float *out = from_key && chunk == 0 ? a.cen_a + (size_t)p * dim : nullptr;  // seed a becomes ca
  float acc = 0.0f;
  for (uint32_t q0 = 0; q0 < dq; q0 += kCenQuads) {  // (block-uniform)
    const uint32_t nq = min(kCenQuads, dq - q0);
    __syncthreads();  // the staged columns have been read before the next are laid in
    if (from_key) stage_member(cen, seed, out, q0, nq, dim); else stage_row(cen, row, q0, nq, dim);  // (uniform)
    __syncthreads();
    if (valid) acc = chain_quads(acc, src, cen, q0, nq);
  }
  unsigned long long key = valid ? rebalance_far_key(acc, pos) : 0ull;
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_xor(key, off, kWave);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) atomicMax(reinterpret_cast<unsigned long long *>(key_out + p), key);
}

__global__ void __launch_bounds__(kSplitThreads) split_side_kernel(SplitArgs a, const uint64_t *key_b) {
  __shared__ __attribute__((aligned(16))) float cen[2][kCenQuads * 4];
  const uint32_t p = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
  if (!a.active[p]) return;
  const uint32_t d = a.donor[p], dim = a.m.dim, dq = a.m.dq;
  const uint32_t count = member_count(a, p, d), base = chunk * kSplitThreads;
  if (base >= count) return;  // (block-uniform)
  const uint32_t pos = base + threadIdx.x;
  const bool valid = pos < count;
  const float4 *src = slot_quads(a.m, valid ? member_slot(a.m, d, pos) : 0);  // (read only where valid)
  const float *row_b = key_b ? nullptr : a.cen_b + (size_t)p * dim;
  const float4 *seed = key_b ? slot_quads(a.m, member_slot(a.m, d, min(rebalance_key_pos(key_b[p]), count - 1))) : nullptr;
  float *out = key_b && chunk == 0 ? a.cen_b + (size_t)p * dim : nullptr;  // seed b becomes cb
  float da = 0.0f, db = 0.0f;
  for (uint32_t q0 = 0; q0 < dq; q0 += kCenQuads) {  // (block-uniform)
    const uint32_t nq = min(kCenQuads, dq - q0);
    __syncthreads();
    stage_row(cen[0], a.cen_a + (size_t)p * dim, q0, nq, dim);
    if (key_b) stage_member(cen[1], seed, out, q0, nq, dim); else stage_row(cen[1], row_b, q0, nq, dim);  // (uniform)
    __syncthreads();
    if (valid) {
      da = chain_quads(da, src, cen[0], q0, nq);
      db = chain_quads(db, src, cen[1], q0, nq);
    }
  }
  if (valid) a.side[(size_t)a.side_off[p] + pos] = (uint8_t)rebalance_side(da, db);
}

__global__ void __launch_bounds__(kWave) split_means_kernel(SplitArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[kWave * kMeanStride];
  const uint32_t p = blockIdx.x;
  if (!a.active[p]) return;
  const uint32_t lane = threadIdx.x, d = a.donor[p], dim = a.m.dim, dq = a.m.dq;
  const uint32_t q0 = blockIdx.y * kMeanQuads, col = blockIdx.y * kMeanCols + lane;
  const uint32_t count = member_count(a, p, d);
  const uint8_t *side = a.side + a.side_off[p];
  float acc0 = 0.0f, acc1 = 0.0f;
  uint32_t n1 = 0;
  for (uint32_t base = 0; base < count; base += kWave) {  // (wave-uniform)
    const uint32_t m = min((uint32_t)kWave, count - base);
    const bool valid = lane < m;
    const float4 *src = slot_quads(a.m, valid ? member_slot(a.m, d, base + lane) : 0);
#pragma unroll
    for (uint32_t c = 0; c < kMeanQuads; ++c)
      if (q0 + c < dq) {  // (uniform)
        const float4 v = valid ? src[(size_t)(q0 + c) * kWave] : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(&tile[lane * kMeanStride + 4u * c]) = v;
      }
    const uint64_t on1 = __ballot(valid && side[base + lane] != 0);  // bit v: member base + v is on side 1
    n1 += (uint32_t)__popcll(on1);
    __syncthreads();
    if (col < dim)
      for (uint32_t v = 0; v < m; ++v) {  // (the branch is wave-uniform) the other side's chain skips the member
        const float x = tile[v * kMeanStride + lane];
        if ((on1 >> v) & 1ull) acc1 = refine_chain_add(acc1, x); else acc0 = refine_chain_add(acc0, x);
      }
    __syncthreads();  // the tile has been read out before the next members are laid in
  }
  const uint32_t n0 = count - n1;
  if (blockIdx.y == 0 && lane == 0) {
    a.counts[2 * p] = n0;
    a.counts[2 * p + 1] = n1;
  }
  if (rebalance_side_empty(n0, n1) || col >= dim) return;  // an empty side: ca and cb stay
  float *pa = a.cen_a + (size_t)p * dim + col, *pb = a.cen_b + (size_t)p * dim + col;
  const float ca = refine_mean(acc0, n0), cb = refine_mean(acc1, n1);
  const bool differs = rebalance_float_bits(ca) != rebalance_float_bits(*pa) || rebalance_float_bits(cb) != rebalance_float_bits(*pb);
  *pa = ca;
  *pb = cb;
  if (__ballot(differs) && lane == 0) a.changed[p] = 1u;  // (every writer writes the same value)
}

}  // namespace

vi_status device_split_lists(const ListMembers &m, const std::vector<RebalancePair> &pairs, const uint64_t *len_host, uint32_t split_iters,
                             float *table_host, hipStream_t st, SplitStats *stats) {
  const uint32_t np = (uint32_t)pairs.size(), dim = m.dim;
  if (np == 0) return VI_OK;
  std::vector<uint32_t> donor(np), side_off(np + 1, 0), active(np, 1u);
  std::vector<float> h_a((size_t)np * dim), h_b((size_t)np * dim);
  uint64_t longest = 0, members = 0;
  for (uint32_t p = 0; p < np; ++p) {
    const uint32_t d = pairs[p].donor;
    if (d >= m.nlists || pairs[p].receiver >= m.nlists || len_host[d] < 2) return fail(VI_ERR_OTHER, "rebalance: a pair of the plan names no list");
    donor[p] = d;
    members += len_host[d];
    longest = std::max(longest, len_host[d]);
    side_off[p + 1] = (uint32_t)members;  // (the members of distinct donors: at most the records of the index, below 2^32)
    std::copy(table_host + (size_t)d * dim, table_host + (size_t)(d + 1) * dim, h_a.begin() + (size_t)p * dim);
  }
  DevBuf<uint32_t> d_donor, d_active, d_off, d_words;   // d_words: per pair the two counts, then per pair `changed`
  DevBuf<float> d_a, d_b;
  DevBuf<uint64_t> d_keys;                              // key a of every pair, then key b
  DevBuf<uint8_t> d_side;
  VI_TRY(upload(d_donor, donor.data(), np, st));
  VI_TRY(upload(d_active, active.data(), np, st));
  VI_TRY(upload(d_off, side_off.data(), np + 1, st));
  VI_TRY(upload(d_a, h_a.data(), (size_t)np * dim, st));
  VI_TRY(d_b.reserve((size_t)np * dim));
  VI_TRY(d_keys.reserve(2 * (size_t)np));
  VI_TRY(d_words.reserve(3 * (size_t)np));
  VI_TRY(d_side.reserve(members));
  VI_HIP(hipMemsetAsync(d_keys.p, 0, 2 * (size_t)np * 8, st));
  VI_HIP(hipMemsetAsync(d_b.p, 0, (size_t)np * dim * 4, st));
  const uint64_t chunks = (longest + kSplitThreads - 1) / kSplitThreads;
  if (chunks * np > 0x7FFFFFFFull) return fail(VI_ERR_OTHER, "rebalance: the donors of one round are too long for one launch");
  const SplitArgs a{m, np, (uint32_t)chunks, d_donor.p, d_active.p, d_off.p, d_a.p, d_b.p, d_side.p, d_words.p, d_words.p + 2 * (size_t)np};
  const dim3 grid_members((uint32_t)(chunks * np));
  const dim3 grid_cols(np, (dim + kMeanCols - 1) / kMeanCols);
  const uint64_t row_bytes = (uint64_t)dim * 4, gather_bytes = m.cur ? 4 : 0;
  EventSpans<1> ev;
  VI_TRY(ev.create(true));
  auto span = [&](auto &&launches) -> vi_status {  // the kernels of one step between two events; synchronises st
    VI_TRY(ev.begin(0, st));
    launches();
    VI_HIP(hipGetLastError());
    VI_TRY(ev.end(0, st));
    VI_HIP(hipStreamSynchronize(st));
    stats->ms_kernels += ev.ms(0);
    return VI_OK;
  };

  // ---- seeds: a = the member farthest from the donor's centre, b = the member farthest from a ----
  std::vector<uint64_t> keys(2 * (size_t)np);
  VI_TRY(span([&] {
    hipLaunchKernelGGL(split_farthest_kernel, grid_members, dim3(kSplitThreads), 0, st, a, (const uint64_t *)nullptr, d_keys.p);
    hipLaunchKernelGGL(split_farthest_kernel, grid_members, dim3(kSplitThreads), 0, st, a, (const uint64_t *)d_keys.p, d_keys.p + np);
  }));
  VI_HIP(hipMemcpyAsync(keys.data(), d_keys.p, keys.size() * 8, hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  stats->split_bytes += 2 * members * (row_bytes + gather_bytes);
  uint32_t going = 0;
  for (uint32_t p = 0; p < np; ++p) {
    if (rebalance_key_pos(keys[p]) >= len_host[donor[p]] || rebalance_key_pos(keys[np + p]) >= len_host[donor[p]])
      return fail(VI_ERR_OTHER, "rebalance: a seed lies outside its list");
    active[p] = rebalance_skip(keys[np + p]) ? 0u : 1u;
    going += active[p];
  }
  stats->pairs_planned += np;
  stats->splits_skipped += np - going;
  stats->splits_done += going;
  const std::vector<uint32_t> split = active;  // the pairs whose centres are taken over

  // ---- inner iterations ----
  std::vector<uint32_t> words(3 * (size_t)np);
  for (uint32_t it = 0; it < split_iters && going; ++it) {
    VI_HIP(hipMemcpyAsync(d_active.p, active.data(), np * 4, hipMemcpyHostToDevice, st));
    VI_HIP(hipMemsetAsync(d_words.p, 0, 3 * (size_t)np * 4, st));
    VI_TRY(span([&] {
      hipLaunchKernelGGL(split_side_kernel, grid_members, dim3(kSplitThreads), 0, st, a, it == 0 ? (const uint64_t *)(d_keys.p + np) : nullptr);
      hipLaunchKernelGGL(split_means_kernel, grid_cols, dim3(kWave), 0, st, a);
    }));
    VI_HIP(hipMemcpyAsync(words.data(), d_words.p, words.size() * 4, hipMemcpyDeviceToHost, st));
    VI_HIP(hipStreamSynchronize(st));
    for (uint32_t p = 0; p < np; ++p) {
      if (!active[p]) continue;
      const uint64_t len = len_host[donor[p]];
      stats->inner_iterations += 1;
      stats->split_bytes += 2 * len * (row_bytes + gather_bytes) + 2 * len + 4 * row_bytes;
      if (words[2 * p] + (uint64_t)words[2 * p + 1] != len) return fail(VI_ERR_OTHER, "rebalance: the sides of a split do not cover its list");
      if (rebalance_side_empty(words[2 * p], words[2 * p + 1]) || words[2 * (size_t)np + p] == 0) {
        active[p] = 0;
        --going;
      }
    }
  }

  // ---- the two centres of every split pair into the table ----
  VI_HIP(hipMemcpyAsync(h_a.data(), d_a.p, h_a.size() * 4, hipMemcpyDeviceToHost, st));
  VI_HIP(hipMemcpyAsync(h_b.data(), d_b.p, h_b.size() * 4, hipMemcpyDeviceToHost, st));
  VI_HIP(hipStreamSynchronize(st));
  for (uint32_t p = 0; p < np; ++p) {
    if (!split[p]) continue;
    std::copy(h_a.begin() + (size_t)p * dim, h_a.begin() + (size_t)(p + 1) * dim, table_host + (size_t)pairs[p].donor * dim);
    std::copy(h_b.begin() + (size_t)p * dim, h_b.begin() + (size_t)(p + 1) * dim, table_host + (size_t)pairs[p].receiver * dim);
  }
  return VI_OK;
}

}  // namespace vi
