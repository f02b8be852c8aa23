"""GPU: exact (flat) k-NN over a built index — vi_indexer_search_exact, host and device form.

The reference is made on the CPU from the index's own export(): the rows in list order, the reference's scalar-order f32
squared L2 of every (query, row) pair, np.lexsort by (distance bits, ordinal), the first k.  The distances are formed for
all pairs at once as the same sequential f32 chain (numpy float32 arithmetic rounds every step as the scalar code does)
and a sample of them is checked against oracle_lib.l2sq_scalar, whose bits they are.  Every comparison is for equality:
uint32 views of D, ids, ordinals, counts, padding."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip

pytestmark = pytest.mark.gpu

U64_MAX = np.uint64((1 << 64) - 1)
NLIST = 8
TRIM = [0, 1, 64, 65]   # lengths four of the lists are cut to; the others stay over 128


def make_rows(kind, n, dim, seed):
    """n rows about NLIST well-separated centres (the same for every seed), so that a build finds a list for each"""
    rng, crng = np.random.default_rng(seed), np.random.default_rng(1)
    which = rng.integers(0, NLIST, size=n)
    if kind == "sift":      # 8-bit descriptors, integers 0..218: the q_bytes forms
        centres = crng.integers(40, 180, size=(NLIST, dim))
        return np.clip(centres[which] + rng.integers(-25, 26, size=(n, dim)), 0, 218).astype(np.float32)
    X = (crng.standard_normal((NLIST, dim)) * 4.0)[which] + rng.standard_normal((n, dim))
    return (X + (60.0 if kind == "offset" else 0.0)).astype(np.float32)   # offset: images about the mean


class Case:
    """an index with list lengths 0, 1, 64, 65 and the rest over 128, its rows in list order and queries of its kind"""

    def __init__(self, kind, dim, tmp):
        X = make_rows(kind, 2600, dim, 7)
        self.idx = vip.build(X, str(tmp), nlist=NLIST, now_secs=1_700_000_000, ext_ids=np.arange(2600, dtype=np.uint64) * 3 + 11)
        ext, _, _, where = self.idx.export()
        lists = (where >> np.uint64(32)).astype(np.int64)
        lens = np.bincount(lists, minlength=self.idx.num_centroids)
        assert (np.sort(lens)[::-1][:len(TRIM)] > 128).all()
        drop = [ext[lists == l][t:] for l, t in zip(np.argsort(lens)[::-1][:len(TRIM)], TRIM)]   # the longest four are cut
        self.idx.remove_ids(np.concatenate(drop))
        self.ext, self.X, _, where = self.idx.export()
        self.lens = np.bincount((where >> np.uint64(32)).astype(np.int64), minlength=self.idx.num_centroids)
        assert set(TRIM) <= set(self.lens.tolist()) and self.lens.max() > 128
        self.Q = make_rows(kind, 300, dim, 8)
        self.Q[:40] = self.X[::max(len(self.X) // 40, 1)][:40]   # some queries are stored rows: distance 0
        self._dist = {}

    def distances(self, nq):
        """bits of the reference distance of queries [0, nq) to every row: one sequential f32 chain per pair"""
        if nq not in self._dist:
            Q, acc = self.Q[:nq], np.zeros((nq, len(self.X)), dtype=np.float32)
            for d in range(self.X.shape[1]):
                t = Q[:, d:d + 1] - self.X[None, :, d]
                acc = acc + t * t
            for q, r in [(0, 0), (nq - 1, len(self.X) - 1), (nq // 2, 77)]:
                assert acc[q, r].view(np.uint32) == O.l2sq_scalar(Q[q], self.X[r]).view(np.uint32)
            self._dist[nq] = acc.view(np.uint32)
        return self._dist[nq]

    def expect(self, nq, k, admitted=None):
        """(D bits, I, ord, counts) the call must return; admitted: a mask over the rows"""
        bits = self.distances(nq)
        rows = np.arange(len(self.X)) if admitted is None else np.flatnonzero(admitted)
        D = np.full((nq, k), np.float32(np.inf).view(np.uint32), dtype=np.uint32)
        I, R = np.full((nq, k), -1, dtype=np.int64), np.full((nq, k), U64_MAX, dtype=np.uint64)
        m = min(k, len(rows))
        for q in range(nq):
            top = rows[np.lexsort((rows, bits[q, rows]))[:m]]
            D[q, :m], I[q, :m], R[q, :m] = bits[q, top], self.ext[top].astype(np.int64), top
        return D, I, R, np.full(nq, m, dtype=np.uint64)

    def check(self, nq, k, filter=None, admitted=None, opts=None):
        D, I, R = self.idx.search_exact_sync(self.Q[:nq], k, filter=filter, opts=opts, with_ordinals=True)
        eD, eI, eR, _ = self.expect(nq, k, admitted)
        assert (D.view(np.uint32) == eD).all() and (I == eI).all() and (R == eR).all()
        return D, I


@functools.lru_cache(maxsize=None)
def _case(kind, dim, tmp):
    return Case(kind, dim, tmp)


@pytest.fixture
def case(tmp_path_factory):
    return lambda kind, dim: _case(kind, dim, tmp_path_factory.getbasetemp() / f"exact_{kind}_{dim}")


# every boundary once: a single partial chunk (4), a chunk tail (20), the LDS-resident limit (128), the streaming form
# (144); tile tails 1 / 129 / 300; k 1 / 10 / 128; the three kinds of data
@pytest.mark.parametrize("kind,dim,nq,k", [
    ("gauss", 4, 1, 1), ("gauss", 20, 129, 10), ("gauss", 128, 300, 128), ("gauss", 144, 129, 10),
    ("sift", 128, 129, 10), ("sift", 20, 300, 1), ("sift", 144, 1, 128), ("offset", 128, 129, 10), ("offset", 20, 1, 128),
])
def test_exact_search_equals_the_sorted_brute_force(case, kind, dim, nq, k):
    case(kind, dim).check(nq, k)


def test_filters_padding_and_counts(case):
    c = case("gauss", 20)
    five = c.ext[[0, 70, 500, 900, len(c.ext) - 1]]
    for ids, k in [(five, 10), (c.ext[::2], 10), (five, 1)]:     # k above the admitted records pads the rows
        admitted = np.isin(c.ext, ids)
        c.check(129, k, filter=c.idx.filter_ids(ids), admitted=admitted)
    # the device form, with counts
    from hiprt import Hip
    hip = Hip()
    try:
        xq, D, I, R, n = hip.upload(c.Q[:129].copy()), hip.alloc(1290 * 4), hip.alloc(1290 * 8), hip.alloc(1290 * 8), hip.alloc(129 * 8)
        c.idx.search_exact_device(xq, 129, 10, D, I, R, n, filter=c.idx.filter_ids(five))
        got = (hip.download(D, (129, 10), np.uint32), hip.download(I, (129, 10), np.int64),
               hip.download(R, (129, 10), np.uint64), hip.download(n, (129,), np.uint64))
    finally:
        hip.close()
    for g, e in zip(got, c.expect(129, 10, np.isin(c.ext, five))):
        assert (g == e).all()


def test_options_never_change_a_result(case):
    c = case("gauss", 20)
    base = c.check(129, 10)
    for opts in ({"seed_probe": 1}, {"seed_probe": NLIST}, {"cand_cap": 10, "seed_probe": 1}):
        D, I = c.check(129, 10, opts=opts)
        assert (D.view(np.uint32) == base[0].view(np.uint32)).all() and (I == base[1]).all()
    st = c.idx.exact_stats()   # (of the last call: a candidate array of k entries under a one-list seed overflows)
    assert st["cand_cap"] == 10 and st["seed_probe"] == 1 and st["overflow_rows"] > 0 and st["nq"] == 129


def test_equals_the_probed_search_at_every_list(case):
    c = case("gauss", 20)
    D, I = c.idx.search_exact_sync(c.Q[40:104], 10)             # (no stored rows among them: no equal distances)
    Ds, Is = c.idx.search_sync(c.Q[40:104], 10, c.idx.num_centroids)
    assert (D.view(np.uint32) == Ds.view(np.uint32)).all() and (I == Is).all()


@pytest.mark.parametrize("what", ["copies_of_one_vector", "every_vector_twice"])
def test_ties_go_to_the_lower_ordinal(tmp_path, what):
    c = Case.__new__(Case)
    X = make_rows("gauss", 700, 20, 3)
    if what == "copies_of_one_vector":     # 600 equal keys but for the ordinal: more than the candidates hold
        X = np.concatenate([X, np.repeat(X[:1], 600, axis=0)])
    else:
        X = np.concatenate([X, X])
    c.idx = vip.build(X, str(tmp_path), nlist=NLIST, now_secs=1_700_000_000)
    c.ext, c.X, _, _ = c.idx.export()
    c.Q, c._dist = np.concatenate([X[:3], make_rows("gauss", 30, 20, 4)]), {}
    c.check(33, 128, opts={"cand_cap": 128})
    if what == "copies_of_one_vector":
        assert c.idx.exact_stats()["overflow_rows"] >= 1   # (the query that is the copied vector)
    c.check(33, 10)
