"""GPU: exact (flat) inner-product threshold search over a built index — vi_indexer_range_search_exact_ip, host and device
form.

The indexes are those of test_exact_search_gpu.py (its Case), the reference scores those of test_exact_ip_gpu.py (its Ip:
the numpy-float32 chain s = s + q[i] * v[i] over the index's own export).  The hits of a query are the rows with
S[q] >= t in an f32 compare, ordered by np.lexsort((rows, -S[q, rows])).  lims, uint32 views of the scores, ids and
ordinals (tie) are compared for equality."""
import numpy as np
import pytest

import vector_indexer_py as vip
from hiprt import Hip
from test_exact_ip_gpu import Ip, ip_of
from test_exact_search_gpu import NLIST, Case, case, make_rows  # noqa: F401  (case: the fixture that shares the indexes)

pytestmark = pytest.mark.gpu
NEG_INF = np.float32(-np.inf)


def expect(ip, nq, t, admitted=None):
    """(lims, S bits, I, ordinals) the call must return for queries [0, nq); t: one threshold or one per query"""
    rows = np.arange(len(ip.X)) if admitted is None else np.flatnonzero(admitted)
    t = np.broadcast_to(np.asarray(t, dtype=np.float32), (nq,))
    hits = []
    for q in range(nq):
        sel = rows[ip.S[q, rows] >= t[q]]     # (NaN: empty)
        hits.append(sel[np.lexsort((sel, -ip.S[q, sel]))])
    lims = np.concatenate([[0], np.cumsum([len(h) for h in hits])]).astype(np.uint64)
    R = np.concatenate(hits).astype(np.int64)
    S = np.concatenate([ip.S[q, h] for q, h in enumerate(hits)]).astype(np.float32)
    return lims, S.view(np.uint32), ip.ext[R].astype(np.int64), R.astype(np.uint64)


def run(ip, nq, min_score, filter=None, min_scores=None, opts=None):
    """the device form: (lims, S bits, I, tie)"""
    hip = Hip()
    try:
        mp = hip.upload(np.asarray(min_scores, dtype=np.float32)) if min_scores is not None else 0
        res = ip.idx.range_search_exact_ip_device(hip.upload(ip.Q[:nq].copy()), nq, min_score, filter=filter, min_scores_ptr=mp, opts=opts)
        lims, S, I = res.copy()
        tie = hip.alloc(max(res.total, 1) * 8)
        res.copy_device(tie_ptr=tie)
        out = (lims, S.view(np.uint32), I, hip.download(tie, (res.total,), np.uint64))
        res.free()
        return out
    finally:
        hip.close()


def same(got, want):
    assert all(g.shape == w.shape and (g == w).all() for g, w in zip(got, want))


def kth_scores(ip, nq, k):
    """each query's k-th largest score"""
    return -np.sort(-ip.S[:nq], axis=1)[:, k - 1]


def small_ip(tmp, X, Q):
    idx = vip.build(X, str(tmp), nlist=NLIST, now_secs=1_700_000_000)
    ext, Xe, _, _ = idx.export()
    return Ip(idx, ext, Xe, Q)


# the nine shapes of the exact radius search: lists of 0 / 1 / 64 / 65 / > 128 records; a single partial chunk (4), a
# chunk tail (20), the register-resident limit (128), the streaming form (144); tile tails 1 / 129 / 300; centred images
# (offset) and no-lo-plane data (sift)
@pytest.mark.parametrize("kind,dim,nq", [
    ("gauss", 4, 1), ("gauss", 20, 129), ("gauss", 128, 300), ("gauss", 144, 129), ("sift", 128, 129), ("sift", 20, 300),
    ("sift", 144, 1), ("offset", 128, 129), ("offset", 20, 1),
])
def test_equals_the_brute_force_at_three_thresholds(case, kind, dim, nq):
    ip = ip_of(case(kind, dim), (kind, dim))
    for k in (1, 10, 100):
        t = np.median(kth_scores(ip, nq, k)).astype(np.float32)
        got = run(ip, nq, float(t))
        same(got, expect(ip, nq, t))
        assert got[0][-1] >= nq * k // 2   # (half the queries have their k-th largest score at or above the median)


@pytest.mark.parametrize("dim", [20, 144])
def test_the_threshold_is_inclusive(case, dim):
    ip = ip_of(case("gauss", dim), ("gauss", dim))
    q = 41
    row = int(np.lexsort((np.arange(len(ip.X)), -ip.S[q]))[4])
    s = ip.S[q, row]
    for t, inside in ((s, True), (np.nextafter(s, np.float32(np.inf)), False)):
        got = run(ip, 129, float(t))
        same(got, expect(ip, 129, t))
        assert (row in got[3][int(got[0][q]):int(got[0][q + 1])]) == inside


def test_negative_scores_and_rows_that_straddle_zero(case):
    ip = ip_of(case("gauss", 128), ("gauss", 128, "neg"), lambda Q: -Q)
    for k in (10, len(ip.X) // 2):     # the 10th largest score; the median score, which is negative for some queries
        t = kth_scores(ip, 129, k)
        want = expect(ip, 129, t)
        same(run(ip, 129, 0.0, min_scores=t), want)
    lo = np.minimum.reduceat(want[1].view(np.float32), want[0][:-1].astype(np.int64))
    assert (lo < 0).any() and (ip.S[:129].max(axis=1) > 0).all()     # rows that hold scores of both signs


def test_an_all_zero_query(tmp_path):
    ip = small_ip(tmp_path, make_rows("gauss", 700, 20, 3), np.zeros((1, 20), dtype=np.float32))
    lims, S, I, tie = got = run(ip, 1, 0.0)
    same(got, expect(ip, 1, 0.0))
    assert lims[1] == 700 and (S == 0).all() and (tie == np.arange(700)).all()     # (bits of +0, ordinal order)
    assert run(ip, 1, float(np.nextafter(np.float32(0), np.float32(1))))[0][1] == 0


def test_minus_infinity_and_a_pool_that_is_too_small(case):
    ip = ip_of(case("gauss", 20), ("gauss", 20))
    want = expect(ip, 129, NEG_INF)
    assert want[0][-1] == 129 * len(ip.X)
    same(run(ip, 129, float("-inf")), want)
    assert ip.idx.exact_ip_range_stats()["sweeps"] == 1
    same(run(ip, 129, float("-inf"), opts={"pool_cap": 64}), want)
    st = ip.idx.exact_ip_range_stats()
    assert st["sweeps"] == 2 and st["hits"] == want[0][-1] and st["pool_cap"] == st["hits"]


def test_per_query_thresholds_host_and_device(case):
    ip = ip_of(case("offset", 128), ("offset", 128))
    t = kth_scores(ip, 129, 10).copy()      # each query's own 10th largest score
    t[5], t[77] = np.nan, np.inf
    want = expect(ip, 129, t)
    n = np.diff(want[0])
    assert n[5] == 0 and n[77] == 0 and (np.delete(n, [5, 77]) >= 10).all()
    same(run(ip, 129, float("-inf"), min_scores=t), want)                       # (the scalar would return everything)
    lims, S, I = ip.idx.range_search_exact_ip_sync(ip.Q[:129], float("nan"), min_scores=t)
    same((lims, S.view(np.uint32), I), want[:3])


def test_filters(case):
    c = case("gauss", 20)
    ip = ip_of(c, ("gauss", 20))
    t = np.median(kth_scores(ip, 129, 100)).astype(np.float32)
    for ids in (c.ext[[0, 70, 500, 900, len(c.ext) - 1]], c.ext[::2]):
        admitted = np.isin(c.ext, ids)
        for thr in (t, NEG_INF):
            got = run(ip, 129, float(thr), filter=c.idx.filter_ids(ids))
            same(got, expect(ip, 129, thr, admitted))
            assert admitted[got[3].astype(np.int64)].all()


def test_rows_longer_than_the_lds_sort(tmp_path):
    ip = small_ip(tmp_path, make_rows("gauss", 9000, 4, 5), make_rows("gauss", 3, 4, 6))
    want = expect(ip, 3, NEG_INF)
    assert (np.diff(want[0]) == 9000).all()
    same(run(ip, 3, float("-inf")), want)


def test_agrees_with_the_top_k_call(case):
    ip = ip_of(case("gauss", 128), ("gauss", 128))
    lims, S, I, tie = run(ip, 129, 0.0, min_scores=kth_scores(ip, 129, 10))
    Sk, Ik, Rk = ip.idx.search_exact_ip_sync(ip.Q[:129], 10, with_ordinals=True)
    first = lims[:-1].astype(np.int64)[:, None] + np.arange(10)
    assert (np.diff(lims) >= 10).all()
    assert (S[first] == Sk.view(np.uint32)).all() and (I[first] == Ik).all() and (tie[first] == Rk).all()
