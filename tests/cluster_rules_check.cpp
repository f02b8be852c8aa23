// Stand-alone host check of csrc/cluster_rules.hpp: the union-find, the core test and the border choice of a radius
// clustering, run on plain arrays with the one-thread access policy, against a naive labelling.  Prints one line per
// failed check and exits non-zero if there was one.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

#include "cluster_rules.hpp"

using Edges = std::vector<std::pair<uint32_t, uint32_t>>;
static int failures = 0;

static void fail(const char *what, uint32_t a, uint32_t b, uint32_t c) {
  std::printf("FAILED %s: %u %u %u\n", what, a, b, c);
  ++failures;
}

// label[x] = the minimum member of x's component, by relabelling until nothing changes
static std::vector<uint32_t> naive_components(uint32_t n, const Edges &edges) {
  std::vector<uint32_t> label(n);
  for (uint32_t i = 0; i < n; ++i) label[i] = i;
  for (bool changed = true; changed;) {
    changed = false;
    for (const auto &e : edges) {
      const uint32_t m = std::min(label[e.first], label[e.second]);
      if (label[e.first] != m || label[e.second] != m) { label[e.first] = label[e.second] = m; changed = true; }
    }
  }
  return label;
}

static void check_graph(const char *what, uint32_t n, Edges edges, std::mt19937 &rng) {
  const std::vector<uint32_t> want = naive_components(n, edges);
  for (int round = 0; round < 3; ++round) {
    std::shuffle(edges.begin(), edges.end(), rng);
    std::vector<uint32_t> parent(n);
    for (uint32_t i = 0; i < n; ++i) parent[i] = i;
    for (const auto &e : edges) {
      // either direction, as the two rows of a pair give it
      if (rng() & 1u) vi::cluster_unite<vi::PlainAccess>(parent.data(), e.first, e.second);
      else vi::cluster_unite<vi::PlainAccess>(parent.data(), e.second, e.first);
      for (uint32_t probe = 0; probe < 2; ++probe) {
        const uint32_t x = probe ? e.first : e.second;
        if (parent[x] > x) fail("parent[x] <= x", x, parent[x], 0);
      }
    }
    for (uint32_t x = 0; x < n; ++x) {
      if (parent[x] > x) fail(what, x, parent[x], 1);
      const uint32_t r0 = vi::cluster_root<vi::PlainAccess>(parent.data(), x);
      const uint32_t r1 = vi::cluster_find<vi::PlainAccess>(parent.data(), x);
      if (r0 != want[x] || r1 != want[x]) fail(what, x, r0, want[x]);  // every root is its component's minimum
      if (parent[r1] != r1) fail("a root is its own parent", x, r1, parent[r1]);
    }
  }
}

static Edges chain(uint32_t n, uint32_t base) {
  Edges e;
  for (uint32_t i = 0; i + 1 < n; ++i) e.push_back({base + i, base + i + 1});
  return e;
}

static Edges clique(uint32_t n, uint32_t base) {
  Edges e;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < n; ++j)
      if (i != j) e.push_back({base + i, base + j});  // both directions: 70 x 69 unions on one root
  return e;
}

static Edges star(uint32_t leaves, uint32_t hub, uint32_t first_leaf) {
  Edges e;
  for (uint32_t i = 0; i < leaves; ++i) e.push_back({hub, first_leaf + i});
  return e;
}

int main() {
  std::mt19937 rng(12345);
  check_graph("no edges", 50, {}, rng);
  check_graph("chain of 200", 200, chain(200, 0), rng);
  check_graph("clique of 70", 70, clique(70, 0), rng);
  check_graph("star", 31, star(30, 30, 0), rng);  // the hub is the HIGHEST index: the root is still the minimum
  {
    // two stars joined by a bridge, a chain and a clique beside them, numbered in a shuffled order
    const uint32_t n = 400;
    std::vector<uint32_t> name(n);
    for (uint32_t i = 0; i < n; ++i) name[i] = i;
    std::shuffle(name.begin(), name.end(), rng);
    Edges e = star(30, 0, 1), s2 = star(30, 31, 32), c = chain(200, 63), k = clique(70, 263);
    e.insert(e.end(), s2.begin(), s2.end());
    e.push_back({62, 0});
    e.push_back({62, 31});
    e.insert(e.end(), c.begin(), c.end());
    e.insert(e.end(), k.begin(), k.end());
    for (auto &p : e) p = {name[p.first], name[p.second]};
    check_graph("planted shapes", n, e, rng);
  }
  for (int g = 0; g < 200; ++g) {
    const uint32_t n = 1 + rng() % 300, m = rng() % (2 * n);
    Edges e;
    for (uint32_t i = 0; i < m; ++i) e.push_back({(uint32_t)(rng() % n), (uint32_t)(rng() % n)});  // (self loops included)
    check_graph("random graph", n, e, rng);
  }

  // the core test: degree + 1 >= min_pts, without wrapping
  if (!vi::cluster_is_core(0, 0) || !vi::cluster_is_core(0, 1) || vi::cluster_is_core(0, 2)) fail("core: degree 0", 0, 0, 0);
  if (!vi::cluster_is_core(3, 4) || vi::cluster_is_core(3, 5)) fail("core: degree 3", 3, 0, 0);
  if (!vi::cluster_is_core(0xFFFFFFFFu, 0xFFFFFFFFu) || !vi::cluster_is_core(0xFFFFFFFFu, 1)) fail("core: wrap", 0, 0, 0);
  if (vi::cluster_is_core(0xFFFFFFFDu, 0xFFFFFFFFu)) fail("core: just below", 0, 0, 0);

  // the link rule and the label of a slot: cores 1, 2 (one cluster, root 1) and 5 (alone); 7 is a border of 5 and 2
  {
    uint32_t parent[8], border[8];
    for (uint32_t i = 0; i < 8; ++i) { parent[i] = i; border[i] = vi::kNoBorder; }
    const bool core[8] = {false, true, true, false, false, true, false, false};
    const uint32_t pairs[][2] = {{2, 1}, {7, 5}, {2, 7}, {3, 4}, {0, 1}};  // (row's record, hit)
    for (const auto &p : pairs) vi::cluster_link<vi::PlainAccess>(parent, border, p[0], core[p[0]], p[1], core[p[1]]);
    const uint32_t want[8] = {1, 1, 1, vi::kNoBorder, vi::kNoBorder, 5, vi::kNoBorder, 1};  // 7: its lowest core is 2, of cluster 1
    for (uint32_t s = 0; s < 8; ++s) {
      const uint32_t got = vi::cluster_label_slot<vi::PlainAccess>(parent, border, s, core[s]);
      if (got != want[s]) fail("label slot", s, got, want[s]);
    }
    if (border[7] != 2 || border[0] != 1 || border[3] != vi::kNoBorder) fail("border", border[7], border[0], border[3]);
  }
  return failures ? 1 : 0;
}
