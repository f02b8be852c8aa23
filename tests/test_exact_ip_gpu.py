"""GPU: exact (flat) inner-product k-NN over a built index — vi_indexer_search_exact_ip, host and device form.

The indexes are those of test_exact_search_gpu.py (its Case: lists of 0 / 1 / 64 / 65 and over 128 records).  The reference
is made on the CPU from the index's own export(): the rows in list order, the score of every (query, row) pair as the
sequential f32 chain s = s + q[i] * v[i] (numpy float32 arithmetic rounds the product and the sum separately, as the
contract says), np.lexsort by (ordinal, descending score), the first k.  Three pairs are checked against a plain Python
loop of np.float32 operations.  Every comparison is for equality: uint32 views of S, ids, ordinals, counts, padding."""
import numpy as np
import pytest

import vector_indexer_py as vip
from test_exact_search_gpu import NLIST, Case, case, make_rows  # noqa: F401  (case: the fixture that shares the indexes)

pytestmark = pytest.mark.gpu

U64_MAX = np.uint64((1 << 64) - 1)
NEG_INF = np.float32(-np.inf).view(np.uint32)


class Ip:
    """queries Q against the exported rows (ext, X) of idx: the reference scores once, the calls checked against them"""

    def __init__(self, idx, ext, X, Q):
        self.idx, self.ext, self.X, self.Q = idx, ext, X, np.ascontiguousarray(Q, dtype=np.float32)
        acc = np.zeros((len(self.Q), len(X)), dtype=np.float32)
        for d in range(X.shape[1]):
            acc = acc + self.Q[:, d:d + 1] * X[None, :, d]
        for q, r in [(0, 0), (len(self.Q) - 1, len(X) - 1), (len(self.Q) // 2, 77)]:
            s = np.float32(0.0)
            for a, b in zip(self.Q[q], X[r]):
                s = np.float32(s + np.float32(a * b))
            assert s.view(np.uint32) == acc[q, r].view(np.uint32)
        self.S = acc

    def expect(self, nq, k, admitted=None):
        """(S bits, I, ord, counts) the call must return; admitted: a mask over the rows"""
        rows = np.arange(len(self.X)) if admitted is None else np.flatnonzero(admitted)
        S = np.full((nq, k), NEG_INF, dtype=np.uint32)
        I, R = np.full((nq, k), -1, dtype=np.int64), np.full((nq, k), U64_MAX, dtype=np.uint64)
        m = min(k, len(rows))
        for q in range(nq):
            top = rows[np.lexsort((rows, -self.S[q, rows]))[:m]]
            S[q, :m], I[q, :m], R[q, :m] = self.S[q, top].view(np.uint32), self.ext[top].astype(np.int64), top
        return S, I, R, np.full(nq, m, dtype=np.uint64)

    def check(self, nq, k, filter=None, admitted=None, opts=None):
        S, I, R = self.idx.search_exact_ip_sync(self.Q[:nq], k, filter=filter, opts=opts, with_ordinals=True)
        eS, eI, eR, _ = self.expect(nq, k, admitted)
        assert (S.view(np.uint32) == eS).all() and (I == eI).all() and (R == eR).all()
        return S, I, R


_ips = {}


def ip_of(c, key, transform=lambda Q: Q):
    """the Ip of a shared Case under a transform of its queries, made once"""
    if key not in _ips:
        _ips[key] = Ip(c.idx, c.ext, c.X, transform(c.Q))
    return _ips[key]


# the nine shapes of the exact L2 search: every chunk tail, the resident / streaming boundary (128 / 144), tile tails
# 1 / 129 / 300, k 1 / 10 / 128; offset: centred block images against the uncentred query; sift: no lo.hi plane
@pytest.mark.parametrize("kind,dim,nq,k", [
    ("gauss", 4, 1, 1), ("gauss", 20, 129, 10), ("gauss", 128, 300, 128), ("gauss", 144, 129, 10),
    ("sift", 128, 129, 10), ("sift", 20, 300, 1), ("sift", 144, 1, 128), ("offset", 128, 129, 10), ("offset", 20, 1, 128),
])
def test_exact_ip_equals_the_sorted_brute_force(case, kind, dim, nq, k):
    ip_of(case(kind, dim), (kind, dim)).check(nq, k)


def zero_one(Q):
    Q = Q.copy()
    Q[5] = 0.0
    return Q


# -Q: the L2 seed is the worst there is and most scores are negative; a zero query: every score +0, the overflow path
@pytest.mark.parametrize("name,transform", [("neg", lambda Q: -Q), ("x1000", lambda Q: 1000.0 * Q), ("zero", zero_one)])
def test_query_transforms(case, name, transform):
    ip = ip_of(case("gauss", 128), ("gauss", 128, name), transform)
    _, _, R = ip.check(129, 10)
    if name == "zero":
        assert (R[5] == np.arange(10)).all() and ip.idx.exact_ip_stats()["overflow_rows"] >= 1


def test_rows_of_spread_norms(tmp_path):
    X = make_rows("gauss", 700, 20, 3) * np.random.default_rng(5).choice(np.float32([0.25, 1.0, 4.0]), size=(700, 1))
    idx = vip.build(X, str(tmp_path), nlist=NLIST, now_secs=1_700_000_000)
    ext, Xe, _, _ = idx.export()
    ip = Ip(idx, ext, Xe, make_rows("gauss", 33, 20, 4))
    _, I, _ = ip.check(33, 10)
    assert (I != idx.search_exact_sync(ip.Q, 10)[1]).any()     # (the L2 neighbours are other records)


def test_filters_padding_counts_and_the_device_form(case):
    c = case("gauss", 20)
    ip = ip_of(c, ("gauss", 20))
    five = c.ext[[0, 70, 500, 900, len(c.ext) - 1]]
    for ids, k in [(five, 10), (c.ext[::2], 10), (five, 1)]:     # k above the admitted records pads the rows
        ip.check(129, k, filter=c.idx.filter_ids(ids), admitted=np.isin(c.ext, ids))
    from hiprt import Hip
    hip = Hip()
    try:
        xq, S, I, R, n = hip.upload(ip.Q[:129].copy()), hip.alloc(1290 * 4), hip.alloc(1290 * 8), hip.alloc(1290 * 8), hip.alloc(129 * 8)
        for ids in (five, None):
            flt = None if ids is None else c.idx.filter_ids(ids)
            c.idx.search_exact_ip_device(xq, 129, 10, S, I, R, n, filter=flt)
            got = (hip.download(S, (129, 10), np.uint32), hip.download(I, (129, 10), np.int64),
                   hip.download(R, (129, 10), np.uint64), hip.download(n, (129,), np.uint64))
            for g, e in zip(got, ip.expect(129, 10, None if ids is None else np.isin(c.ext, ids))):
                assert (g == e).all()
    finally:
        hip.close()


def test_options_never_change_a_result(case):
    ip = ip_of(case("gauss", 20), ("gauss", 20))
    ip.check(129, 10, opts={"seed_probe": NLIST})
    ip.check(129, 10, opts={"cand_cap": 10, "seed_probe": 1})
    st = ip.idx.exact_ip_stats()
    assert st["cand_cap"] == 10 and st["seed_probe"] == 1 and st["nq"] == 129 and st["survivors"] >= st["candidates"]


@pytest.mark.parametrize("what", ["copies_of_one_vector", "every_vector_twice"])
def test_ties_go_to_the_lower_ordinal(tmp_path, what):
    X = make_rows("gauss", 700, 20, 3)
    X = np.concatenate([X, np.repeat(X[:1], 601, axis=0)] if what == "copies_of_one_vector" else [X, X])
    idx = vip.build(X, str(tmp_path), nlist=NLIST, now_secs=1_700_000_000)
    ext, Xe, _, _ = idx.export()
    ip = Ip(idx, ext, Xe, np.concatenate([X[:3], make_rows("gauss", 30, 20, 4)]))
    ip.check(33, 128, opts={"cand_cap": 128})
    if what == "copies_of_one_vector":     # 602 equal scores at or above the seed's: more than the candidates hold
        assert idx.exact_ip_stats()["overflow_rows"] >= 1
    ip.check(33, 10)
