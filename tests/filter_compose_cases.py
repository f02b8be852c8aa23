"""Helpers of test_filter_compose_gpu.py: the fixtures' sizes and the expected results of a search through ANY filter.

The contract is test_id_filter_gpu.py's, with the predicate left open: admit[row] says, per record of the data set, whether
the filter admits it (computed in numpy from the ids and timestamps the fixture wrote); the oracle's full stable-sorted
candidate sequence (Fixture.full) masked by it, cut at k, is the answer — ids, distance bits, counts and padding."""
import numpy as np

from test_id_filter_gpu import (EVERYTHING, HALF, NOW, U64_MAX, Fixture, bits, ext_ids_for, queries,  # noqa: F401
                                timestamps_for, u64)

SHAPES = [(1, 1, 1), (33, 10, 8), (300, 100, 10_000)]
MID = SHAPES[1]


def make_base(root):      # D = 32: the MFMA engine; 24 lists of about 250 = 3 x 64 + 58: ragged last blocks
    rng = np.random.default_rng(1)
    X = rng.standard_normal((6000, 32)).astype(np.float32)
    return Fixture(root, X, 24, queries(rng, X, 300), seed=1)


def make_valu(root):      # D % 4 != 0: the exact-order VALU engine
    rng = np.random.default_rng(3)
    X = rng.standard_normal((6000, 10)).astype(np.float32)
    return Fixture(root, X, 24, queries(rng, X, 300), seed=3)


def make_bytes8(root):    # 8-bit descriptors with integer queries: the int8 rank kernel
    rng = np.random.default_rng(5)
    centers = rng.integers(40, 216, size=(24, 128))
    X = np.clip(centers[rng.integers(0, 24, 6000)] + rng.integers(-40, 41, size=(6000, 128)), 0, 255).astype(np.float32)
    return Fixture(root, X, 24, queries(rng, X, 300, integer=True), seed=5)


def in_set(fx, name):
    return np.isin(fx.ext, fx.ids(name))


def in_window(fx, window):
    return (fx.ts >= np.uint64(window[0])) & (fx.ts <= np.uint64(window[1]))


def in_range(fx, lo, hi):
    return (fx.ext >= np.uint64(lo)) & (fx.ext <= np.uint64(hi))


def list_rows(fx, index=None):
    """(row of the data set, `where`) of every resident record of `index`, in its list order (what a mask is indexed by)"""
    ext, _, _, where = (index or fx.gpu).export()
    return fx.rows_of(ext.astype(np.int64)), where


def mask_for(fx, admit, index=None):
    """admit (per row of the data set) as the mask of `index`: one uint8 per resident record in list order"""
    return admit[list_rows(fx, index)[0]].astype(np.uint8)


def expected(fx, admit, nq, k, n_probe):
    D, I = fx.full(n_probe)
    D, I = D[:nq], I[:nq]
    keep = (I >= 0) & admit[fx.rows_of(I)]
    rank = np.cumsum(keep, axis=1) - 1
    take = keep & (rank < k)
    De, Ie = np.full((nq, k), np.inf, dtype=np.float32), np.full((nq, k), -1, dtype=np.int64)
    r, c = np.nonzero(take)
    De[r, rank[r, c]], Ie[r, rank[r, c]] = D[r, c], I[r, c]
    return De, Ie, np.minimum(keep.sum(axis=1), k)


def check(fx, flt, admit, nq, k, n_probe, index=None, what=""):
    De, Ie, cnt = expected(fx, admit, nq, k, n_probe)
    Dg, Ig = (index or fx.gpu).search_sync(fx.Q[:nq], k, n_probe, filter=flt)
    bad = np.nonzero((Ig != Ie).any(axis=1) | (bits(Dg) != bits(De)).any(axis=1))[0]
    assert bad.size == 0, (f"{what} nq {nq} k {k} n_probe {n_probe}: {bad.size} queries differ, first {bad[0]}: gpu "
                           f"{Ig[bad[0]][:12]} {Dg[bad[0]][:12]} expected {Ie[bad[0]][:12]} {De[bad[0]][:12]}")
    assert ((Ig >= 0).sum(axis=1) == cnt).all()
    return cnt


def check_all(fx, flt, admit, shapes=SHAPES, index=None, what=""):
    """the count, and the search at every shape"""
    assert flt.num_allowed == int(admit.sum()), (what, flt.num_allowed, int(admit.sum()))
    return [check(fx, flt, admit, nq, k, p, index=index, what=what) for nq, k, p in shapes]


def same_results(fx, fa, fb, shapes=SHAPES, index=None):
    """two filters (or None: the unfiltered entry) give bit-identical searches"""
    for nq, k, p in shapes:
        Da, Ia = (index or fx.gpu).search_sync(fx.Q[:nq], k, p, filter=fa)
        Db, Ib = (index or fx.gpu).search_sync(fx.Q[:nq], k, p, filter=fb)
        assert np.array_equal(Ia, Ib) and np.array_equal(bits(Da), bits(Db)), (nq, k, p)


def nothing_found(fx, flt, shapes=SHAPES):
    assert flt.num_allowed == 0
    for nq, k, p in shapes:
        D, I = fx.gpu.search_sync(fx.Q[:nq], k, p, filter=flt)   # VI_OK
        assert (I == -1).all() and np.isinf(D).all()


class AndCase:
    """the expression the engine tests share: AND(window HALF, ids "half", NOT ids "tenth", mask of a random 70 %)"""

    def __init__(self, fx):
        self.fx = fx
        self.mask_rows = np.random.default_rng(77).random(fx.n) < 0.7
        self.parts = [in_window(fx, HALF), in_set(fx, "half"), ~in_set(fx, "tenth"), self.mask_rows]
        self.admit_and = np.logical_and.reduce(self.parts)
        self.admit_or = np.logical_or.reduce(self.parts)

    def terms(self, vip, index=None):
        fx = self.fx
        return [vip.Term.timestamps(*HALF), vip.Term.ids(fx.sets["half"]), ~vip.Term.ids(fx.sets["tenth"]),
                vip.Term.mask(mask_for(fx, self.mask_rows, index))]

    def chain(self, index=None):
        """the same four predicates as single filters of the existing entries"""
        ix = index or self.fx.gpu
        return [ix.filter_timestamps(*HALF), ix.filter_ids(self.fx.sets["half"]),
                ix.filter_ids(self.fx.sets["tenth"], exclude=True), ix.filter_mask(mask_for(self.fx, self.mask_rows, index))]
