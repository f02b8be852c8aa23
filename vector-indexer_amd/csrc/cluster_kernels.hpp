// cluster_kernels.hpp — the kernels around a radius clustering's link step, shared by the probed clustering
// (cluster_radius.hip) and the exact one (flat_join.hip): the access policy of the union-find on the device, the reset of
// the per-slot state, the core bits and the labels with their counts.  Each translation unit compiles its own copy
// (unnamed namespace).  The rules themselves are cluster_rules.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cluster_rules.hpp"
#include "list_layout.hpp"

namespace vi {
namespace {

struct AgentAccess {  // the link kernel's policy: relaxed, agent scope, never a plain access
  static __device__ __forceinline__ uint32_t load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ void store(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  static __device__ __forceinline__ uint32_t cas(uint32_t *p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
  static __device__ __forceinline__ void min(uint32_t *p, uint32_t v) { (void)atomicMin(p, v); }
};

enum Counter : uint32_t { kCountCore = 0, kCountBorder, kCountRoots, kCountHits, kCounters };

__global__ void __launch_bounds__(256) cluster_init_kernel(uint32_t *parent, uint32_t *border, uint32_t *degree, uint32_t nslots) {
  const uint32_t s = blockIdx.x * 256u + threadIdx.x;
  if (s >= nslots) return;
  parent[s] = s;
  border[s] = kNoBorder;
  degree[s] = 0u;
}

// bit (block, lane) = the slot holds a participant (resident, and admitted where there is a filter) that is core
__global__ void __launch_bounds__(256) cluster_core_kernel(ResidentLists L, const uint64_t *allow, const uint32_t *degree,
                                                           uint32_t min_pts, uint64_t *core) {
  for_each_resident_block(L, [&](uint32_t block, uint32_t lane, bool resident, uint32_t, uint32_t) {
    const bool part = resident && (!allow || ((allow[block] >> lane) & 1ull));
    const uint64_t word = __ballot(part && cluster_is_core(degree[block * 64u + lane], min_pts));
    if (lane == 0) core[block] = word;
  });
}

struct LabelArgs {
  ResidentLists L;
  const uint64_t *prefix;     // [nlists] records before each list in list order (ensure_fetch_layout)
  const uint64_t *core;
  const uint32_t *parent, *border, *degree;
  int64_t *labels;            // [N] in list order, or null
  uint32_t *degree_out;       // [N] in list order, or null
  unsigned long long *count;  // [kCounters]
  uint32_t link;              // parent / border / core hold a clustering (else only the degrees are delivered)
};

// slot -> list-order ordinal, as the export numbers its rows
__device__ __forceinline__ uint64_t ordinal_of(const LabelArgs &a, uint32_t slot) {
  const uint32_t blk = slot >> 6, l = list_of_block(a.L.first_block, a.L.nlists, blk);
  return a.prefix[l] + (uint64_t)(blk - a.L.first_block[l]) * 64u + (slot & 63u);
}

// One wave per block of 64 slots; every resident slot writes its label and degree at its own ordinal.  Pad slots write
// nothing: they have no ordinal.  The counts go out with one atomic per wave and counter.
__global__ void __launch_bounds__(256) cluster_label_kernel(LabelArgs a) {
  for_each_resident_block(a.L, [&](uint32_t block, uint32_t lane, bool resident, uint32_t l, uint32_t b) {
    const uint32_t s = block * 64u + lane;
    const uint64_t ord = a.prefix[l] + (uint64_t)b * 64u + lane;
    const bool core = a.link && ((a.core[block] >> lane) & 1ull);
    uint32_t rep = kNoBorder, deg = 0;
    if (resident) {
      deg = a.degree[s];
      if (a.link) rep = cluster_label_slot<AgentAccess>(a.parent, a.border, s, core);
      if (a.labels) a.labels[ord] = rep == kNoBorder ? kLabelNoise : (int64_t)ordinal_of(a, rep);
      if (a.degree_out) a.degree_out[ord] = deg;
    }
    const uint32_t n_core = (uint32_t)__popcll(__ballot(resident && core));
    const uint32_t n_border = (uint32_t)__popcll(__ballot(resident && !core && rep != kNoBorder));
    const uint32_t n_roots = (uint32_t)__popcll(__ballot(resident && core && rep == s));
    unsigned long long hits = deg;
    for (uint32_t off = 32u; off; off >>= 1) hits += __shfl_down(hits, off, 64);
    if (lane == 0) {
      if (n_core) atomicAdd(a.count + kCountCore, (unsigned long long)n_core);
      if (n_border) atomicAdd(a.count + kCountBorder, (unsigned long long)n_border);
      if (n_roots) atomicAdd(a.count + kCountRoots, (unsigned long long)n_roots);
      if (hits) atomicAdd(a.count + kCountHits, hits);
    }
  });
}

}  // namespace
}  // namespace vi
