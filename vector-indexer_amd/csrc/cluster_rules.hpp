// cluster_rules.hpp — the rules by which a radius clustering (cluster_radius.hip) turns the entries of the radius graph
// into labels: the lock-free union-find of its link kernel, the core test and the border choice.  Nothing of HIP is
// included, so a host program can run the very same functions on plain arrays (tests/cluster_rules_check.cpp); the
// kernels call them with an access policy whose every access is an agent-scope relaxed atomic.
//
// An access policy A names how a word of `parent` / `border` is touched:
//   A::load(p)            the word
//   A::store(p, v)        write it
//   A::cas(p, expect, v)  if *p == expect then *p = v; returns what *p held before, either way
//   A::min(p, v)          *p = min(*p, v)
//
// Union by index.  The one invariant is parent[x] <= x, with equality exactly at a root.  A root is only ever changed by
// the CAS of unite, which hooks the LARGER of two roots under the smaller: the invariant holds afterwards, a non-root
// never becomes a root again, and the root of a tree is the minimum of its members.  Slot order is list order, so that
// minimum is the record of the lowest list-order ordinal: the component's representative needs no second pass.
//
// Why stale values cannot hurt.  Once g is an ancestor of x it stays one: parent words of non-roots only ever move to
// other ancestors (the halving store below), and roots only gain a parent.  So whatever age the values find reads have,
// it walks up x's own tree, strictly downwards in index, and ends at a slot that was a root when read.  If that slot has
// been hooked meanwhile the CAS of unite fails — it compares with the slot's own index — and returns the newer parent, from
// which the walk goes on.  A stale ancestor costs a retry, never a wrong hook.  Nothing waits for another thread: a retry
// follows somebody else's successful hook, of which there are fewer than slots.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define VI_CLUSTER_FN __host__ __device__ inline
#else
#define VI_CLUSTER_FN inline
#endif

namespace vi {

constexpr uint32_t kNoBorder = 0xFFFFFFFFu;  // border[s] of a record no core record is adjacent to
constexpr int64_t kLabelNoise = -1;          // VI_LABEL_NOISE

struct PlainAccess {  // one thread, plain arrays: the host's policy
  static uint32_t load(const uint32_t *p) { return *p; }
  static void store(uint32_t *p, uint32_t v) { *p = v; }
  static uint32_t cas(uint32_t *p, uint32_t expect, uint32_t v) {
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
  }
  static void min(uint32_t *p, uint32_t v) {
    if (v < *p) *p = v;
  }
};

// the root of x's tree, with path halving: every slot passed is pointed at its grandparent (an ancestor: see above)
template <class A>
VI_CLUSTER_FN uint32_t cluster_find(uint32_t *parent, uint32_t x) {
  for (;;) {
    const uint32_t p = A::load(parent + x);
    if (p == x) return x;
    const uint32_t g = A::load(parent + p);
    if (g == p) return p;
    A::store(parent + x, g);  // (x is no root and never will be: this races with no hook)
    x = g;                    // g < p < x: strictly down
  }
}

// the same without a store, for a reader after the last hook (cluster_label_kernel)
template <class A>
VI_CLUSTER_FN uint32_t cluster_root(const uint32_t *parent, uint32_t x) {
  for (;;) {
    const uint32_t p = A::load(parent + x);
    if (p == x) return x;
    x = p;
  }
}

// joins the trees of a and b: the larger root goes under the smaller by one CAS; on failure the walk continues from
// what the CAS found there
template <class A>
VI_CLUSTER_FN void cluster_unite(uint32_t *parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = cluster_find<A>(parent, a);
    b = cluster_find<A>(parent, b);
    if (a == b) return;
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t old = A::cas(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;  // hi was hooked by somebody else: old < hi is its parent now
    b = lo;
  }
}

// a participant is core when it and its row together are at least min_pts records (min_pts 0 and 1: every participant)
VI_CLUSTER_FN bool cluster_is_core(uint32_t degree, uint32_t min_pts) { return (uint64_t)degree + 1u >= (uint64_t)min_pts; }

// one entry (a = the row's record, b = a hit of the row, a != b, both participants) of the radius graph.  Both core: one
// cluster.  One core: the other's border candidate, of which the lowest slot wins — whichever of the two rows the pair
// was seen in, so the adjacency is the union of both directions.
template <class A>
VI_CLUSTER_FN void cluster_link(uint32_t *parent, uint32_t *border, uint32_t a, bool a_core, uint32_t b, bool b_core) {
  if (a_core && b_core) cluster_unite<A>(parent, a, b);
  else if (a_core) A::min(border + b, a);
  else if (b_core) A::min(border + a, b);
}

// what the label of slot s is the ordinal of: kNoBorder stands for noise
template <class A>
VI_CLUSTER_FN uint32_t cluster_label_slot(const uint32_t *parent, const uint32_t *border, uint32_t s, bool core) {
  if (core) return cluster_root<A>(parent, s);
  const uint32_t c = A::load(border + s);
  return c == kNoBorder ? kNoBorder : cluster_root<A>(parent, c);
}

}  // namespace vi
