"""The tie fixture of the radius-merge tests (test_range_merge_cpu.py, test_range_merge_gpu.py) and the numpy helpers both
share: an integer grid with 600 duplicated rows, so that equal distances — inside a rank and across ranks — are the rule,
in 6 lists of 9 - 11 blocks, so that at world 8 every rank still holds a stripe of every list."""
import numpy as np

NLIST = 6
WORLDS = (2, 4, 8)
PROBES = (1, 3)
INF = float("inf")


def tie_data():
    rng = np.random.default_rng(4)
    base = rng.integers(-4, 5, size=(3000, 12)).astype(np.float32)
    X = np.concatenate([base, base[:600]])
    Q = np.concatenate([base[:40], rng.integers(-4, 5, size=(24, 12)).astype(np.float32)])
    return X, Q


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def cut(radius2, D, I, T=None):
    """padded per-query sorted sequences (I < 0: padding) -> CSR (lims, D, I[, tie]) of the entries with d <= radius2"""
    hit = (I >= 0) & (D <= np.float32(radius2))
    lims = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.uint64)
    return (lims, D[hit], I[hit]) if T is None else (lims, D[hit], I[hit], T[hit])


def median_kth(D, I, kth):
    """the median over the queries of the kth candidate's distance (1-based; an actual distance, so the boundary is hit)"""
    d = np.sort(D[I[:, kth - 1] >= 0, kth - 1])
    assert d.size > 0
    return float(d[d.size // 2])


def radii(D, I):
    return {"r10": median_kth(D, I, 10), "r100": median_kth(D, I, 100), "inf": INF}


def empty_rows(parts):
    """(rank, query) rows without an entry"""
    return sum(int((np.diff(p[0].astype(np.int64)) == 0).sum()) for p in parts)


def queries_with_cross_rank_ties(parts):
    """queries in which some distance bit pattern occurs on two or more ranks"""
    nq = parts[0][0].size - 1
    n = 0
    for q in range(nq):
        seen = [np.unique(bits(p[1][int(p[0][q]):int(p[0][q + 1])])) for p in parts]
        u, c = np.unique(np.concatenate(seen), return_counts=True)
        n += bool((c >= 2).any())
    return n


def same(got, want, tie=True):
    """lims, ids, distance bits (and tie keys) equal"""
    assert np.array_equal(np.asarray(got[0]).astype(np.uint64), np.asarray(want[0]).astype(np.uint64)), "lims differ"
    assert np.array_equal(got[2], want[2]), "ids differ"
    assert np.array_equal(bits(got[1]), bits(want[1])), "distance bits differ"
    if tie:
        assert np.array_equal(np.asarray(got[3]).view(np.uint64), np.asarray(want[3]).view(np.uint64)), "tie keys differ"
