"""Inputs for the Lloyd update pass (vi_kmeans_partial_sums_device / launch_segment_sums): make(name) -> (X, labels, k).

A plain module (no fixtures, no GPU): tests/test_update_cases_cpu.py proves on the CPU that every case does what its
line in CASES says, tests/test_kmeans_update_gpu.py runs them through the library.

What the cases are built around (kmeans.hip, list_build.hip):
  * clusters above BIG = 2048 members are summed by segment_big_kernel when 16 <= d <= 512, d % 4 == 0 and X is 16-byte
    aligned, every other cluster by segment_kernel.  The big kernel stages H = 16384 // d rows per chunk and runs three
    chunks per trip of its loop; its grid is min(k, 1024) workgroups striding over the big clusters;
  * segment_kernel adds 32 rows per step (kSegAhead) with a predicated tail;
  * the ids are grouped by label with a stable radix sort: 1..4 passes of 8 bits by the bits of k - 1, tiles of 4096
    points, the per-digit scan of the tile counts taking 256 tiles per step.
A name that contains "big" promises at least one cluster above BIG members.
"""
import numpy as np

BIG = 2048            # kBigCluster
CHUNK_FLOATS = 16384  # kBigChunkFloats
RADIX_TILE = 4096     # kRadixTile

GEOMETRY_DIMS = (16, 20, 24, 32, 96, 100, 128, 500, 512)
KINDS = ("normal", "offset", "scaled", "ints", "negzero", "special")
ORDER_INSENSITIVE_KINDS = ("ints",)  # exact sums: these check membership only
TILE_NS = (1, 63, 64, 65, 4095, 4096, 4097, 8193)
HIER_K, HIER_D, HIER_META_K, HIER_COPIES = 6000, 16, 77, 2600
HIER_SEEDS = (42, 7, 1)


def _rng(name):
    return np.random.default_rng([ord(c) for c in name])


def data(kind, n, d, rng):
    """n x d f32 rows of one data kind"""
    X = rng.standard_normal((n, d)).astype(np.float32)
    if kind == "normal":
        pass
    elif kind == "offset":      # a common offset: every add rounds, the sum grows steadily
        X += np.float32(100.0)
    elif kind == "scaled":      # six decades of row scale: small rows vanish or not by their position in the chain
        X *= (10.0 ** rng.uniform(-3, 3, size=(n, 1))).astype(np.float32)
    elif kind == "ints":        # exact, order-insensitive sums
        X = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    elif kind == "negzero":     # rows of -0.0 among ordinary rows (+0.0 + -0.0 = +0.0, x + -0.0 = x)
        X[rng.random(n) < 0.3] = np.float32(-0.0)
    elif kind == "special":     # a few inf, NaN and subnormal values among ordinary ones
        m = max(3, n // 500)
        X[rng.integers(0, n, m), rng.integers(0, d, m)] = np.float32(np.inf)
        X[rng.integers(0, n, m), rng.integers(0, d, m)] = np.float32(-np.inf)
        X[rng.integers(0, n, m), rng.integers(0, d, m)] = np.float32(np.nan)
        sub = (rng.integers(1, 1 << 23, size=4 * m, dtype=np.uint32) | (rng.integers(0, 2, 4 * m, dtype=np.uint32) << 31))
        X[rng.integers(0, n, 4 * m), rng.integers(0, d, 4 * m)] = sub.view(np.float32)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(X, dtype=np.float32)


def labels_from_counts(counts, rng, layout="random"):
    """labels in which cluster c has exactly counts[c] members"""
    lab = np.repeat(np.arange(len(counts), dtype=np.uint32), np.asarray(counts, dtype=np.int64))
    if layout == "random":
        rng.shuffle(lab)
    elif layout == "reverse":
        lab = lab[::-1].copy()
    elif layout != "sorted":
        raise KeyError(layout)
    return lab


def geometry_counts(d):
    """member counts around the chunk size H of the big kernel, and one long chain.  The first ten are around H itself
    (at d >= 24 most of them are <= BIG and exercise the hand-over to segment_kernel); the rest repeat the pattern at
    multiples j H that lie above BIG for every d, j = q, q + 1, q + 2 with q = ceil((BIG + 2) / H): clusters that end
    exactly on a chunk edge, one row short of it and one row past it, for every number of chunks mod 3 (the loop runs
    three chunks per trip), and the same around 3 q H"""
    H = CHUNK_FLOATS // d
    q = -(-(BIG + 2) // H)
    edges = [j * H + r for j in (q, q + 1, q + 2, 3 * q) for r in (0, -1, 1)]
    return [BIG + 1, H, H - 1, H + 1, 2 * H + 1, 3 * H, 3 * H - 1, 3 * H + 1, 6 * H + 5, 60013] + edges


def _from_counts(name, counts, d, kind="normal", layout="random", rng=None):
    rng = rng or _rng(name)
    lab = labels_from_counts(counts, rng, layout)
    return data(kind, lab.size, d, rng), lab, len(counts)


def _geometry(d):
    return lambda name: _from_counts(name, geometry_counts(d), d)


def _boundary(name):
    return _from_counts(name, [BIG - 1, BIG, BIG + 1, BIG + 2], 32)


def _many(name):
    rng = _rng(name)
    return _from_counts(name, list(rng.integers(BIG + 1, BIG + 60, 1100)), 16, rng=rng)


def _residues(d):
    return lambda name: _from_counts(name, list(range(BIG + 1, BIG + 34)), d)


def _fallback_wide(d):
    return lambda name: _from_counts(name, [BIG + 1, 17, BIG + 15, 0, BIG + 32, 4097, 3000, BIG], d)


KIND_COUNTS = [5000, BIG + 1, 3000, 0, 100, BIG, 1, 4500]
NEGZERO_CLUSTER, NEGZERO_SINGLE = 4, 6


def _kind(kind):
    def f(name):
        X, lab, k = _from_counts(name, KIND_COUNTS, 32, kind)
        if kind == "negzero":  # a cluster of -0.0 rows only, and a single -0.0 member: both sum to +0.0
            X[(lab == NEGZERO_CLUSTER) | (lab == NEGZERO_SINGLE)] = np.float32(-0.0)
        return X, lab, k
    return f


def _layout(layout):
    def f(name):
        rng = _rng(name)
        n, k, d = 40000, 12, 32
        if layout == "round_robin":
            lab = (np.arange(n) % k).astype(np.uint32)
        elif layout == "random":
            lab = rng.integers(0, k, n).astype(np.uint32)
        elif layout == "ends":
            lab = np.where(rng.random(n) < 0.5, 0, k - 1).astype(np.uint32)
        else:
            lab = labels_from_counts([n // k + (c < n % k) for c in range(k)], rng, layout)
        return data("normal", n, d, rng), lab, k
    return f


def _one_cluster(k, c):
    def f(name):
        rng = _rng(name)
        n = 300000
        return data("normal", n, 16, rng), np.full(n, c, dtype=np.uint32), k
    return f


def _tile(n):
    def f(name):
        rng = _rng(name)
        return data("normal", n, 16, rng), rng.integers(0, 3, n).astype(np.uint32), 3
    return f


def _radix(k, n, d):
    def f(name):
        rng = _rng(name)
        lab = rng.integers(0, k, n).astype(np.uint32)
        # both ends of the range, repeated members, and (for k - 1 a power of two) labels that differ in their top
        # digit only: 0 and k - 1, 1 and k - 2 interleaved
        lab[: 64] = np.tile(np.array([k - 1, 0, k - 2, 1], dtype=np.uint32), 16)
        lab[n // 2: n // 2 + 300] = lab[rng.integers(0, n // 2, 300)]
        return data("normal", n, d, rng), lab, k
    return f


CASES = {}  # name -> (builder, what the case is for)
for _d in GEOMETRY_DIMS:
    CASES[f"big_geometry_d{_d}"] = (_geometry(_d), f"chunk geometry at d = {_d}: clusters of 2049, H, H+-1, 2H+1, 3H, 3H+-1, 6H+5 "
                                                  f"and 60013 members, H = {CHUNK_FLOATS // _d} rows per chunk (counts <= 2048 "
                                                  "go to segment_kernel: the hand-over between the two kernels), and of "
                                                  "jH, jH+-1 members at four multiples above 2048 (geometry_counts)")
CASES["big_boundary"] = (_boundary, "clusters of exactly 2047, 2048, 2049 and 2050 members in one call")
CASES["big_many"] = (_many, "1100 clusters above 2048 members at d = 16: the stride loop of the 1024-workgroup grid, and 2.3 M "
                            "points (more than 256 radix tiles: the second step of the tile-count scan)")
CASES["big_fallback_residues_d8"] = (_residues(8), "d = 8 (no split): 2049..2081 members, every residue mod 32 of the 32-row tail")
CASES["big_fallback_unaligned_d32"] = (_residues(32), "d = 32 with X offset by one float (4-byte aligned only: no split), "
                                                      "2049..2081 members")
for _d in (18, 516, 1024):
    CASES[f"big_fallback_d{_d}"] = (_fallback_wide(_d), f"d = {_d} (no split): long chains stay in segment_kernel")
UNALIGNED = ("big_fallback_unaligned_d32",)  # the GPU test uploads these one float past an aligned address
for _kind_name in KINDS:
    CASES[f"big_kind_{_kind_name}"] = (_kind(_kind_name), f"data kind '{_kind_name}', clusters of {KIND_COUNTS} members at d = 32")
for _l in ("sorted", "reverse", "round_robin", "random", "ends"):
    CASES[f"big_layout_{_l}"] = (_layout(_l), f"label layout '{_l}': 40000 points, k = 12, d = 32")
CASES["big_one_cluster_k1"] = (_one_cluster(1, 0), "all 300000 points in one cluster, k = 1")
CASES["big_one_cluster_k7"] = (_one_cluster(7, 4), "all 300000 points in cluster 4 of 7: six empty clusters")
for _n in TILE_NS:
    CASES[f"tile_n{_n}"] = (_tile(_n), f"n = {_n}, around the 4096-point radix tile, k = 3")
CASES["radix_k256"] = (_radix(256, 20000, 4), "k = 256: one radix pass")
CASES["radix_k257"] = (_radix(257, 20000, 4), "k = 257: two radix passes")
CASES["radix_k65536"] = (_radix(65536, 150000, 4), "k = 65536: two radix passes, full")
CASES["radix_k65537"] = (_radix(65537, 150000, 4), "k = 65537: three radix passes")
CASES["radix_k16777217"] = (_radix((1 << 24) + 1, 6000, 1), "k = 2^24 + 1: four radix passes (d = 1: 64 MB of sums)")


def radix_passes(k):
    """8-bit passes group_ids_by_label_device runs for k lists"""
    return (max(1, int(k - 1).bit_length()) + 7) // 8


def make(name):
    X, lab, k = CASES[name][0](name)
    return X, np.ascontiguousarray(lab, dtype=np.uint32), int(k)


def kind_of(name):
    return name[len("big_kind_"):] if name.startswith("big_kind_") else "normal"


def lloyd_case(name):
    """(X, k) for the whole-loop tests: clusters far above BIG members"""
    rng = _rng(name)
    if name == "few_distinct":  # 3 distinct rows, k = 5: clusters run empty (the zero row, then the re-seed)
        rows = rng.standard_normal((3, 32)).astype(np.float32) * 3
        return np.ascontiguousarray(rows[rng.integers(0, 3, 60000)]), 5
    d, k = {"d32_k4": (32, 4), "d100_k6": (100, 6), "d32_k6": (32, 6), "d100_k4": (100, 4)}[name]
    centers = rng.standard_normal((7, d)).astype(np.float32) * 2
    X = centers[rng.integers(0, 7, 60000)] + rng.standard_normal((60000, d)).astype(np.float32)
    return np.ascontiguousarray(X, dtype=np.float32), k


LLOYD_CASES = ("d32_k4", "d100_k6", "d32_k6", "d100_k4", "few_distinct")


def hierarchy_case():
    """(X, Cn): HIER_K centroids at d = HIER_D of which HIER_COPIES are exact copies of one row (they fall into one group
    of build_centroid_hierarchy whatever its seed: above BIG members, and meta rows picked among the copies end with
    empty groups), and 5000 points of which some sit on the duplicated row and some near it"""
    rng = _rng("hierarchy")
    Cn = rng.standard_normal((HIER_K, HIER_D)).astype(np.float32)
    row = rng.standard_normal(HIER_D).astype(np.float32)
    Cn[rng.choice(HIER_K, HIER_COPIES, replace=False)] = row
    X = rng.standard_normal((5000, HIER_D)).astype(np.float32)
    X[:300] = row
    X[300:1500] = row + np.float32(0.05) * rng.standard_normal((1200, HIER_D)).astype(np.float32)
    X[1500:2500] = Cn[rng.integers(0, HIER_K, 1000)] + np.float32(0.1) * rng.standard_normal((1000, HIER_D)).astype(np.float32)
    return np.ascontiguousarray(X, dtype=np.float32), Cn


def f64_reference(X, labels, k):
    """(float64 sums, float64 sums of |x|, counts) of the nonempty clusters only: (ids, S, A, m); NaN / inf propagate"""
    order = np.argsort(labels, kind="stable")
    sl = labels[order]
    starts = np.flatnonzero(np.r_[True, sl[1:] != sl[:-1]]) if sl.size else np.zeros(0, dtype=np.int64)
    ids = sl[starts].astype(np.int64)
    m = np.diff(np.r_[starts, sl.size])
    d = X.shape[1]
    S = np.empty((ids.size, d))
    A = np.empty((ids.size, d))
    step = max(1, (1 << 22) // max(1, sl.size))
    with np.errstate(invalid="ignore", over="ignore"):
        for j0 in range(0, d, step):
            Xs = X[order, j0:j0 + step].astype(np.float64)
            S[:, j0:j0 + step] = np.add.reduceat(Xs, starts, axis=0) if sl.size else 0
            A[:, j0:j0 + step] = np.add.reduceat(np.abs(Xs), starts, axis=0) if sl.size else 0
    return ids, S, A, m
