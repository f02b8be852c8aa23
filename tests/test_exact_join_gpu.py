"""GPU: the exact radius self-join — vi_indexer_radius_graph_exact and vi_indexer_cluster_radius_exact (host and device form).

The indexes are those of test_exact_search_gpu.py (its Case: lists of 0 / 1 / 64 / 65 and over 128 records).  The reference
is numpy on the export's rows: the reference's sequential f32 chain for every ORDERED pair (row u as the query of column
v, so d(u, v) and d(v, u) are formed independently), np.lexsort by (bits, ordinal) for the graph, and cluster_reference
(cluster_cases.py) on that graph for the labels.  Every comparison is for equality."""
import numpy as np
import pytest

import vector_indexer_py as vip
from cluster_cases import cluster_reference
from hiprt import Hip
from test_exact_search_gpu import NLIST, case, make_rows  # noqa: F401  (case: the fixture that shares the indexes)
from vector_indexer_py import _native as N

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)


def pair_bits(c):
    """bits[u, v] of the reference distance of row u (as the query) to row v, kept on the case"""
    if not hasattr(c, "_pairs"):
        acc = np.zeros((len(c.X), len(c.X)), dtype=np.float32)
        for d in range(c.X.shape[1]):
            t = c.X[:, d:d + 1] - c.X[None, :, d]
            acc = acc + t * t
        c._pairs = acc.view(np.uint32)
    return c._pairs


def expect(c, radius, exclude_self=True, admitted=None):
    """(lims, D bits, I, ordinals) of the whole graph, and its rows as lists of ordinals"""
    bits, n = pair_bits(c), len(c.X)
    adm = np.ones(n, dtype=bool) if admitted is None else admitted
    inside = (bits <= np.float32(radius).view(np.uint32)) & adm[None, :] & adm[:, None] if radius >= 0 else np.zeros((n, n), dtype=bool)
    if exclude_self:
        inside[np.arange(n), np.arange(n)] = False
    rows = [np.flatnonzero(inside[u]) for u in range(n)]
    rows = [r[np.lexsort((r, bits[u, r]))] for u, r in enumerate(rows)]
    lims = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    R = np.concatenate(rows).astype(np.int64)
    D = np.concatenate([bits[u, r] for u, r in enumerate(rows)])
    return (lims, D, c.ext[R].astype(np.int64), R.astype(np.uint64)), rows


def graph(c, radius, exclude_self=True, filter=None, opts=None):
    """(lims, D bits, I, tie) of radius_graph_exact"""
    hip = Hip()
    try:
        res = c.idx.radius_graph_exact(float(radius), exclude_self=exclude_self, filter=filter, opts=opts)
        lims, D, I = res.copy()
        tie = hip.alloc(max(res.total, 1) * 8)
        res.copy_device(tie_ptr=tie)
        out = (lims, D.view(np.uint32), I, hip.download(tie, (res.total,), np.uint64))
        res.free()
        return out
    finally:
        hip.close()


def same(got, want):
    assert all(g.shape == w.shape and (g == w).all() for g, w in zip(got, want))


def check_labels(c, radius, min_pts, rows, filter=None, admitted=None):
    labels, degree = c.idx.cluster_radius_exact(float(radius), min_pts, filter=filter, with_degree=True)
    el, ed, en, counts = cluster_reference(rows, len(c.X), min_pts, admitted)
    assert (labels == el).all() and (degree == ed).all()
    st = c.idx.exact_join_stats()
    assert st["hits"] == counts["hits"] and st["pairs"] * 2 == counts["hits"] and st["rows"] == len(c.X)
    return labels, en


def kth_radius(c, k):
    """the median over the rows of the distance to the k-th other record"""
    return np.median(np.sort(pair_bits(c), axis=1)[:, k].view(np.float32)).astype(np.float32)


# dim 4 / 20: partial chunks of the image; 128: the register-resident limit; 144: the streaming form.  gauss: lo planes;
# sift: 8-bit data, no lo planes; offset: centred images.  Chunks of 192 rows start mid-block and mid-list, are no whole
# number of tiles, and the last one is a bare triangle.
@pytest.mark.parametrize("kind,dim", [("gauss", 4), ("gauss", 20), ("sift", 128), ("offset", 128), ("gauss", 144), ("sift", 144)])
def test_graph_and_labels_equal_the_brute_force(case, kind, dim, monkeypatch):
    c = case(kind, dim)
    monkeypatch.setenv("VI_GRAPH_CHUNK", "192")
    for k in (1, 10):
        r = kth_radius(c, k)
        want, rows = expect(c, r)
        same(graph(c, r), want)
        assert c.idx.exact_join_stats()["sweeps"] == 1 and want[0][-1] >= len(c.X) * k // 2
        for min_pts in (1, 5):
            labels, n_clusters = check_labels(c, r, min_pts, rows)
            assert c.idx.exact_join_stats()["sweeps"] == (1 if min_pts == 1 else 2)
            assert len(np.unique(labels[labels >= 0])) == n_clusters
    want, _ = expect(c, kth_radius(c, 1), exclude_self=False)          # the default chunk; every row holds its own slot once
    same(graph(c, kth_radius(c, 1), exclude_self=False), want)


@pytest.mark.parametrize("dim", [20, 144])
def test_the_radius_is_inclusive_in_both_directions(case, dim):
    c = case("gauss", dim)
    u, bits = 41, pair_bits(c)
    v = int(np.argsort(bits[u], kind="stable")[5])
    r = bits[u, v:v + 1].view(np.float32)[0]
    for radius, inside in ((r, True), (np.nextafter(r, np.float32(0)), False)):
        lims, D, I, tie = got = graph(c, radius)
        same(got, expect(c, radius)[0])
        assert (v in tie[int(lims[u]):int(lims[u + 1])]) == inside and (u in tie[int(lims[v]):int(lims[v + 1])]) == inside


def test_zero_radius_groups_the_exact_copies(tmp_path):
    X = make_rows("gauss", 700, 20, 3)
    idx = vip.build(np.concatenate([X, X]), str(tmp_path), nlist=NLIST, now_secs=1_700_000_000)   # every vector stored twice
    c = type("C", (), {})()
    c.idx = idx
    c.ext, c.X, _, _ = idx.export()
    for exclude, per_row in ((True, 1), (False, 2)):     # exclusion deletes the row's own slot, not the copy
        lims, D, I, tie = got = graph(c, 0.0, exclude_self=exclude)
        same(got, expect(c, 0.0, exclude_self=exclude)[0])
        assert (np.diff(lims) == per_row).all() and (D == 0).all()
    labels, n_clusters = check_labels(c, 0.0, 1, expect(c, 0.0)[1])
    assert n_clusters == 700 and (np.bincount(labels, minlength=1400)[np.unique(labels)] == 2).all()
    from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig
    ix = VectorIndexer.load(VectorIndexerConfig.new(20).with_index_dir(str(tmp_path / "index")).with_shards_dir(str(tmp_path / "shards")))
    assert ix.duplicate_groups(exact=True) == [[int(e) for e in c.ext[labels == r]] for r in np.unique(labels)]


def test_infinite_negative_radius_and_a_pool_that_is_too_small(case):
    c = case("gauss", 20)
    n = len(c.X)
    want, rows = expect(c, INF)
    assert want[0][-1] == n * (n - 1)
    same(graph(c, INF), want)
    assert c.idx.exact_join_stats()["sweeps"] == 1
    same(graph(c, INF, opts={"pool_cap": 64}), want)
    st = c.idx.exact_join_stats()
    assert st["sweeps"] == 2 and st["hits"] == want[0][-1] == st["pool_cap"] and st["pairs"] == n * (n - 1) // 2
    labels, degree = c.idx.cluster_radius_exact(float(INF), 5, with_degree=True)
    assert (labels == 0).all() and (degree == n - 1).all()
    lims, D, I, tie = graph(c, -1.0)
    assert (lims == 0).all() and len(lims) == n + 1 and D.size == 0 and c.idx.exact_join_stats()["sweeps"] == 0
    labels, n_clusters = check_labels(c, -1.0, 1, [[] for _ in range(n)])
    assert n_clusters == n and c.idx.exact_join_stats()["sweeps"] == 0


def test_filters_empty_the_rows_of_the_rest(case, monkeypatch):
    c = case("gauss", 20)
    monkeypatch.setenv("VI_GRAPH_CHUNK", "192")
    for ids, radius in ((c.ext[[0, 70, 500, 900, len(c.ext) - 1]], INF), (c.ext[::2], kth_radius(c, 10))):
        admitted, flt = np.isin(c.ext, ids), c.idx.filter_ids(ids)
        want, rows = expect(c, radius, admitted=admitted)
        lims, D, I, tie = got = graph(c, radius, filter=flt)
        same(got, want)
        assert (np.diff(lims)[~admitted] == 0).all() and admitted[tie.astype(np.int64)].all()
        for min_pts in (0, 3):
            labels, _ = check_labels(c, radius, min_pts, rows, filter=flt, admitted=admitted)
            assert (labels[~admitted] == -1).all()


def test_device_form_degree_only_and_count_only(case):
    c = case("offset", 128)
    n, r = len(c.X), float(kth_radius(c, 10))
    labels, degree = c.idx.cluster_radius_exact(r, 5, with_degree=True)
    hip = Hip()
    try:
        pl, pd = hip.alloc(n * 8), hip.alloc(n * 4)
        n_clusters = c.idx.cluster_radius_exact_device(pl, pd, r, 5)
        assert (hip.download(pl, (n,), np.int64) == labels).all() and (hip.download(pd, (n,), np.uint32) == degree).all()
        assert n_clusters == len(np.unique(labels[labels >= 0])) and c.idx.exact_join_stats()["sweeps"] == 2
        pd2 = hip.alloc(n * 4)
        N.check(N.lib().vi_indexer_cluster_radius_exact_device(c.idx._h, None, r, 5, None, pd2, None))   # only degrees: one sweep
        assert (hip.download(pd2, (n,), np.uint32) == degree).all() and c.idx.exact_join_stats()["sweeps"] == 1
        assert c.idx.cluster_radius_exact_device(0, 0, r, 5) == n_clusters  # only the count
    finally:
        hip.close()


def test_equals_the_probed_calls_at_every_list(case):
    c = case("gauss", 20)
    r, P = float(kth_radius(c, 10)), c.idx.num_centroids
    for min_pts in (1, 5):
        le, de = c.idx.cluster_radius_exact(r, min_pts, with_degree=True)
        lp, dp = c.idx.cluster_radius(r, P, min_pts, with_degree=True)
        assert (le == lp).all() and (de == dp).all()
    e, p = c.idx.radius_graph_exact(r), c.idx.radius_graph(r, P)
    (le, De, Ie), (lp, Dp, Ip) = e.copy(), p.copy()
    e.free()
    p.free()
    assert (le == lp).all()
    for u in range(len(c.X)):
        a, b = slice(int(le[u]), int(le[u + 1])), slice(int(lp[u]), int(lp[u + 1]))
        assert set(zip(De[a].view(np.uint32).tolist(), Ie[a].tolist())) == set(zip(Dp[b].view(np.uint32).tolist(), Ip[b].tolist()))
