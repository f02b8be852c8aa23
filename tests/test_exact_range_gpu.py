"""GPU: exact (flat) radius search over a built index — vi_indexer_range_search_exact, host and device form.

The reference is the one of test_exact_search_gpu.py (its Case: the index's own export() rows and the reference's sequential
f32 chain for every (query, row) pair): the hits of a query are the rows whose distance bits are <= the radius' bits, in
np.lexsort order by (bits, ordinal).  lims, uint32 views of D, ids and ordinals (tie) are compared for equality."""
import numpy as np
import pytest

import vector_indexer_py as vip
from hiprt import Hip
from test_exact_search_gpu import NLIST, Case, case, make_rows  # noqa: F401  (case: the fixture that shares the indexes)

pytestmark = pytest.mark.gpu
INF = np.float32(np.inf)


def expect(c, nq, radii, admitted=None):
    """(lims, D bits, I, ordinals) the call must return for queries [0, nq); radii: one radius or one per query"""
    bits, rows = c.distances(nq), np.arange(len(c.X)) if admitted is None else np.flatnonzero(admitted)
    radii = np.broadcast_to(np.asarray(radii, dtype=np.float32), (nq,))
    hits = []
    for q in range(nq):
        sel = rows[bits[q, rows] <= radii[q].view(np.uint32)] if radii[q] >= 0 else rows[:0]   # (NaN, negative: empty)
        hits.append(sel[np.lexsort((sel, bits[q, sel]))])
    lims = np.concatenate([[0], np.cumsum([len(h) for h in hits])]).astype(np.uint64)
    R = np.concatenate(hits).astype(np.int64)
    D = np.concatenate([bits[q, h] for q, h in enumerate(hits)])
    return lims, D, c.ext[R].astype(np.int64), R.astype(np.uint64)


def run(c, nq, radius2, filter=None, radii=None, opts=None, vectors=False):
    """the device form: (lims, D bits, I, tie[, V])"""
    hip = Hip()
    try:
        rp = hip.upload(np.asarray(radii, dtype=np.float32)) if radii is not None else 0
        res = c.idx.range_search_exact_device(hip.upload(c.Q[:nq].copy()), nq, radius2, filter=filter, radii_ptr=rp, opts=opts)
        lims, D, I, *V = res.copy(include_vectors=vectors)
        tie = hip.alloc(res.total * 8)
        res.copy_device(tie_ptr=tie)
        out = (lims, D.view(np.uint32), I, hip.download(tie, (res.total,), np.uint64), *V)
        res.free()
        return out
    finally:
        hip.close()


def same(got, want):
    assert all(g.shape == w.shape and (g == w).all() for g, w in zip(got, want))


def kth_radius(c, nq, k):
    """the median over the queries of the distance to the k-th neighbour"""
    return np.median(np.sort(c.distances(nq), axis=1)[:, k - 1].view(np.float32)).astype(np.float32)


def small_case(tmp, X, Q):
    c = Case.__new__(Case)
    c.idx = vip.build(X, str(tmp), nlist=NLIST, now_secs=1_700_000_000)
    c.ext, c.X, _, _ = c.idx.export()
    c.Q, c._dist = Q, {}
    return c


# lists of 0 / 1 / 64 / 65 / > 128 records; a single partial chunk (4), a chunk tail (20), the register-resident limit
# (128), the streaming form (144); tile tails 1 / 129 / 300; the three kinds of data
@pytest.mark.parametrize("kind,dim,nq", [
    ("gauss", 4, 1), ("gauss", 20, 129), ("gauss", 128, 300), ("gauss", 144, 129), ("sift", 128, 129), ("sift", 20, 300),
    ("sift", 144, 1), ("offset", 128, 129), ("offset", 20, 1),
])
def test_equals_the_brute_force_at_three_radii(case, kind, dim, nq):
    c = case(kind, dim)
    for k in (1, 10, 100):
        r = kth_radius(c, nq, k)
        got = run(c, nq, float(r))
        same(got, expect(c, nq, r))
        assert got[0][-1] >= nq * k // 2   # (half the queries have their k-th neighbour within the median radius)


@pytest.mark.parametrize("dim", [20, 144])
def test_the_radius_is_inclusive(case, dim):
    c = case("gauss", dim)
    q, bits = 41, c.distances(129)
    row = int(np.argsort(bits[q], kind="stable")[4])
    r = bits[q, row:row + 1].view(np.float32)[0]
    for radius, inside in ((r, True), (np.nextafter(r, np.float32(0)), False)):
        got = run(c, 129, float(radius))
        same(got, expect(c, 129, radius))
        assert (row in got[3][int(got[0][q]):int(got[0][q + 1])]) == inside


def test_zero_and_negative_radius(tmp_path):
    X = make_rows("gauss", 700, 20, 3)
    c = small_case(tmp_path, np.concatenate([X, X]), X[:33].copy())     # every vector stored twice; queries are stored rows
    lims, D, I, tie = got = run(c, 33, 0.0)
    same(got, expect(c, 33, 0.0))
    assert (np.diff(lims) == 2).all() and (D == 0).all() and (tie[0::2] < tie[1::2]).all()
    lims, D, I = c.idx.range_search_exact_sync(c.Q, -1.0)
    assert (lims == 0).all() and D.size == 0 and c.idx.exact_range_stats()["sweeps"] == 0


def test_infinite_radius_and_a_pool_that_is_too_small(case):
    c = case("gauss", 20)
    want = expect(c, 129, INF)
    assert want[0][-1] == 129 * len(c.X)
    same(run(c, 129, float("inf")), want)
    assert c.idx.exact_range_stats()["sweeps"] == 1
    same(run(c, 129, float("inf"), opts={"pool_cap": 64}), want)
    st = c.idx.exact_range_stats()
    assert st["sweeps"] == 2 and st["hits"] == want[0][-1] and st["pool_cap"] == st["hits"]


def test_filters(case):
    c = case("gauss", 20)
    r = kth_radius(c, 129, 100)
    for ids in (c.ext[[0, 70, 500, 900, len(c.ext) - 1]], c.ext[::2]):
        admitted = np.isin(c.ext, ids)
        for radius in (r, INF):
            got = run(c, 129, float(radius), filter=c.idx.filter_ids(ids))
            same(got, expect(c, 129, radius, admitted))
            assert admitted[got[3].astype(np.int64)].all()


def test_per_query_radii_host_and_device(case):
    c = case("offset", 128)
    radii = np.sort(c.distances(129), axis=1)[:, 9].view(np.float32).copy()   # each query's own 10th neighbour
    radii[5], radii[77] = -1.0, np.nan
    want = expect(c, 129, radii)
    n = np.diff(want[0])
    assert n[5] == 0 and n[77] == 0 and (np.delete(n, [5, 77]) >= 10).all()
    same(run(c, 129, 123.0, radii=radii), want)                                # (the scalar is ignored)
    lims, D, I = c.idx.range_search_exact_sync(c.Q[:129], float("nan"), radii=radii)
    same((lims, D.view(np.uint32), I), want[:3])


def test_rows_longer_than_the_lds_sort(tmp_path):
    c = small_case(tmp_path, make_rows("gauss", 9000, 4, 5), make_rows("gauss", 3, 4, 6))
    want = expect(c, 3, INF)
    assert (np.diff(want[0]) == 9000).all()
    same(run(c, 3, float("inf")), want)


def test_stored_vectors_of_the_device_result(case):
    c = case("gauss", 144)
    lims, D, I, tie, V = run(c, 129, float(kth_radius(c, 129, 10)), vectors=True)
    assert len(tie) and (V.view(np.uint32) == c.X[tie.astype(np.int64)].view(np.uint32)).all()


def test_equals_the_probed_engines_at_every_list(case):
    c = case("gauss", 20)
    r = float(kth_radius(c, 129, 100))
    le, De, Ie = c.idx.range_search_exact_sync(c.Q[:129], r)
    lp, Dp, Ip = c.idx.range_search_sync(c.Q[:129], r, c.idx.num_centroids)
    assert (le == lp).all()
    for q in range(129):
        a, b = slice(int(le[q]), int(le[q + 1])), slice(int(lp[q]), int(lp[q + 1]))
        assert set(zip(De[a].view(np.uint32).tolist(), Ie[a].tolist())) == set(zip(Dp[b].view(np.uint32).tolist(), Ip[b].tolist()))
