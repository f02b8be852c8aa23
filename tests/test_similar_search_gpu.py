"""GPU: search by stored record — vi_indexer_search_by_ids (queries named by external id) and vi_indexer_knn_graph (rows =
records of the list order), host and device forms, with and without the record itself.

The contract: the row of a stored record r is the reference's candidate sequence for r's stored f32 bits with the
candidates a filter does not admit deleted, then — exclude_self — the ONE candidate that is r itself, then the reference's
stable sort and take(k).  The expected rows come from the untouched oracle: OracleIndex.search_batch(X[rows], N, p) is the
whole candidate sequence of each stored vector already stably sorted.  r's own entry in it is the first entry that carries
r's external id at distance bits 0 (its own distance is a sum of squares of zeros; among several such entries — records
sharing id AND vector — deleting any one leaves the same (D, I) row).  Ids, distance bits, counts and padding must match
exactly."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from test_id_filter_gpu import HALF, NOW, U64_MAX, bits, ext_ids_for, timestamps_for, u64
from vector_indexer_py import _native as N

pytestmark = pytest.mark.gpu

KS = [1, 10, 63, 64, 100, 128, 200]
PS = [1, 8, 24, 10_000]
SHAPES = [(k, 8) for k in KS] + [(10, p) for p in PS if p != 8]   # every k at n_probe 8, every n_probe at k 10
NROWS = 300
ORACLE_CHUNK = 500


def own_entries(D, I, own_ids):
    """mask of the first entry of every row that carries the row's own id at distance bits 0"""
    own = (I >= 0) & (I == own_ids.astype(np.int64)[:, None]) & (bits(D) == 0)   # (every stored id is below 2^63)
    return own & (np.cumsum(own, axis=1) == 1)


def take_k(D, I, keep, k):
    n = D.shape[0]
    rank = np.cumsum(keep, axis=1) - 1
    take = keep & (rank < k)
    De, Ie = np.full((n, k), np.inf, dtype=np.float32), np.full((n, k), -1, dtype=np.int64)
    r, c = np.nonzero(take)
    De[r, rank[r, c]], Ie[r, rank[r, c]] = D[r, c], I[r, c]
    return De, Ie, np.minimum(keep.sum(axis=1), k).astype(np.uint64)


class Fixture:
    """one index written once by the oracle and opened by both sides; the oracle's full sorted candidate sequences of the
    chosen rows per n_probe are made once and shared by the tests"""

    def __init__(self, root, X, nlist, ext=None):
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.n, self.dim = self.X.shape
        self.ext = ext_ids_for(self.n) if ext is None else u64(ext)
        self.ts = timestamps_for(self.n)
        self._sorted, self._order = np.sort(self.ext), np.argsort(self.ext)
        self.idx, self.sh = str(root / "index"), str(root / "shards")
        self.orc = O.OracleIndex.build(self.X, self.idx, self.sh, ext_ids=self.ext, timestamps=self.ts, nlist=nlist, now=NOW)
        self.gpu = self.open()
        assert self.gpu.num_vectors == self.n
        self.nlists = self.gpu.num_centroids
        self._full = {}
        self.rows = self.choose_rows()

    def open(self, **kw):
        return vip.load(self.idx, self.sh, self.dim, **kw)

    def rows_of(self, I):   # (unique ids only)
        return self._order[np.searchsorted(self._sorted, np.where(I >= 0, I, 0).astype(np.uint64))]

    def sequences(self, X, n_probe):
        rc, D, I = self.orc.search_batch(X, self.n, min(n_probe, self.nlists))
        assert rc == O.ORC_OK
        return D, I

    def choose_rows(self):
        """300 records: the one carrying id 0, up to five whose own list is NOT the first the coarse step probes (the
        oracle's nearest neighbour at n_probe 1 is then another record), the rest at random"""
        rc, _, I1 = self.orc.search_batch(self.X, 1, 1)
        assert rc == O.ORC_OK
        self.unprobed = np.nonzero(I1[:, 0] != self.ext.astype(np.int64))[0]
        rng = np.random.default_rng(17)
        first = np.unique(np.concatenate([[self.n // 3], self.unprobed[:5]]))
        rest = rng.permutation(np.setdiff1d(np.arange(self.n), first))[: NROWS - first.size]
        return rng.permutation(np.concatenate([first, rest]))

    def full(self, n_probe):
        p = min(n_probe, self.nlists)
        if p not in self._full:
            D, I = self.sequences(self.X[self.rows], p)
            D.setflags(write=False), I.setflags(write=False)
            self._full[p] = (D, I)
        return self._full[p]

    def expected(self, k, n_probe, exclude, admit=None):
        """of self.rows; admit(I) -> mask of the candidates a filter admits"""
        D, I = self.full(n_probe)
        keep = I >= 0
        if admit is not None:
            keep = keep & admit(I)
        if exclude:
            keep = keep & ~own_entries(D, I, self.ext[self.rows])
        return take_k(D, I, keep, k)


def raw_by_ids(index, ids, k, n_probe, exclude, flt=None, want_v=False):
    """the host entry itself -> (D, I, counts, found, k_out[, V])"""
    ids = u64(ids)
    n = ids.size
    D, I = np.full((n, k), 7.0, dtype=np.float32), np.full((n, k), 7, dtype=np.int64)
    counts, found, kout = np.full(n, 7, dtype=np.uint64), np.full(n, 7, dtype=np.uint32), C.c_uint64(0)
    V = np.full((n, k, index.dimension), 7.0, dtype=np.float32) if want_v else None
    N.check(N.lib().vi_indexer_search_by_ids(index._h, flt._h if flt is not None else None, N.ptr(ids), n, k, n_probe,
                                             1 if exclude else 0, N.ptr(D), N.ptr(I), N.ptr(V), N.ptr(counts), N.ptr(found),
                                             C.byref(kout)))
    kk = int(kout.value)
    D, I = D.reshape(-1)[: n * kk].reshape(n, kk), I.reshape(-1)[: n * kk].reshape(n, kk)
    if want_v:
        return D, I, counts, found, kk, V.reshape(-1)[: n * kk * index.dimension].reshape(n, kk, index.dimension)
    return D, I, counts, found, kk


def assert_rows(got, want, what):
    (Dg, Ig, cg), (De, Ie, ce) = got, want
    bad = np.nonzero((Ig != Ie).any(axis=1) | (bits(Dg) != bits(De)).any(axis=1) | (cg != ce))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rows differ, first {bad[0]}: gpu {Ig[bad[0]][:12]} {Dg[bad[0]][:12]} count "
                           f"{cg[bad[0]]} expected {Ie[bad[0]][:12]} {De[bad[0]][:12]} count {ce[bad[0]]}")
    pad = np.arange(Ig.shape[1])[None, :] >= cg[:, None].astype(np.int64)
    assert (Ig[pad] == -1).all() and np.isposinf(Dg[pad]).all(), what


@pytest.fixture(scope="module")
def base(tmp_path_factory):         # D = 32: the MFMA engine; 250-vector lists end in a ragged block
    rng = np.random.default_rng(1)
    return Fixture(tmp_path_factory.mktemp("base"), rng.standard_normal((6000, 32)).astype(np.float32), 24)


@pytest.fixture(scope="module")
def valu(tmp_path_factory):         # D % 4 != 0: the exact-order VALU engine
    rng = np.random.default_rng(3)
    return Fixture(tmp_path_factory.mktemp("valu"), rng.standard_normal((6000, 10)).astype(np.float32), 24)


@pytest.fixture(scope="module")
def bytes8(tmp_path_factory):       # 8-bit descriptors: the int8 rank kernel
    rng = np.random.default_rng(5)
    centers = rng.integers(40, 216, size=(24, 128))
    X = np.clip(centers[rng.integers(0, 24, 6000)] + rng.integers(-40, 41, size=(6000, 128)), 0, 254).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("bytes"), X, 24)


@pytest.fixture(scope="module")
def hip():
    from hiprt import Hip
    h = Hip()
    yield h
    h.close()


def device_by_ids(hip, index, ids, k, n_probe, exclude, flt=None):
    ids = u64(ids)
    n = ids.size
    D, I, T, F = hip.alloc(n * k * 4), hip.alloc(n * k * 8), hip.alloc(n * k * 8), hip.alloc(n * 4)
    index.search_by_ids_device(hip.upload(ids), n, k, n_probe, D, I, T, F, exclude_self=exclude, filter=flt)
    return (hip.download(D, (n, k), np.float32), hip.download(I, (n, k), np.int64), hip.download(T, (n, k), np.uint64),
            hip.download(F, (n,), np.uint32))


def device_search(hip, index, X, k, n_probe, flt=None):
    n = X.shape[0]
    D, I, T = hip.alloc(n * k * 4), hip.alloc(n * k * 8), hip.alloc(n * k * 8)
    index.search_device(hip.upload(X), n, k, n_probe, D, I, T, filter=flt)
    return hip.download(D, (n, k), np.float32), hip.download(I, (n, k), np.int64), hip.download(T, (n, k), np.uint64)


# ---- by id, all three engines ----
@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("name", ["base", "valu", "bytes8"])
def test_by_id_against_the_oracle(name, exclude, request, hip):
    fx = request.getfixturevalue(name)
    ids = fx.ext[fx.rows]
    assert (ids == 0).sum() == 1            # the record carrying id 0 is asked about
    for k, p in SHAPES:
        D, I, counts, found, kk = raw_by_ids(fx.gpu, ids, k, p, exclude)
        assert kk == k and (found == 1).all()
        assert_rows((D, I, counts), fx.expected(k, p, exclude), f"{name} k {k} n_probe {p} exclude {exclude}")
        st = fx.gpu.last_stats()
        assert st["k"] == k and st["nq"] == NROWS, st    # the caller's k, not k + 1
        if name == "bytes8" and (k, p) == (10, 8):
            assert st["rank_mode"] == 3 and st["rank_int8"] == 1, st
        if not exclude:
            # bit for bit the plain search of the stored bits, tie keys (device entries) included
            Ds, Is = fx.gpu.search_sync(fx.X[fx.rows], k, p)
            assert np.array_equal(I, Is) and np.array_equal(bits(D), bits(Ds)), (name, k, p)
    for k, p in [(10, 8), (64, 8), (128, 8), (200, 24)]:
        Dd, Id, Td, Fd = device_by_ids(hip, fx.gpu, ids, k, p, exclude)
        De, Ie, ce = fx.expected(k, p, exclude)
        assert np.array_equal(Id, Ie) and np.array_equal(bits(Dd), bits(De)) and (Fd == 1).all(), (name, k, p)
        # the tie keys: those of the plain device search one entry wider, less the row's own entry
        Ds, Is, Ts = device_search(hip, fx.gpu, fx.X[fx.rows], k + 1 if exclude else k, p)
        keep = Is >= 0
        if exclude:
            keep &= ~own_entries(Ds, Is, ids)
        rank = np.cumsum(keep, axis=1) - 1
        Te = np.full((NROWS, k), U64_MAX, dtype=np.uint64)
        r, c = np.nonzero(keep & (rank < k))
        Te[r, rank[r, c]] = Ts[r, c]
        assert np.array_equal(Td, Te), (name, k, p)


def test_the_engine_crossings_are_exercised(base, valu):
    """k + 1 picks the engine: the non-excluding call at k = 128 (MFMA) / k = 64 (VALU) runs the fast engine, the
    excluding one the engine that sorts every candidate — with the same bits (test_by_id_against_the_oracle)"""
    ids = base.ext[base.rows]
    raw_by_ids(base.gpu, ids, 128, 8, False)
    assert base.gpu.last_stats()["rank_mode"] >= 1
    raw_by_ids(base.gpu, ids, 128, 8, True)
    assert base.gpu.last_stats()["rank_mode"] == 0
    # the VALU engine and the generic one both report rank_mode 0; only the fast engines take phase times
    ids = valu.ext[valu.rows]
    valu.gpu.enable_timing(True)
    try:
        raw_by_ids(valu.gpu, ids, 64, 8, False)
        st = valu.gpu.last_stats()
        assert st["rank_mode"] == 0 and st["ms_total"] > 0.0, st
        raw_by_ids(valu.gpu, ids, 64, 8, True)
        st = valu.gpu.last_stats()
        assert st["rank_mode"] == 0 and st["ms_total"] == 0.0 and st["k"] == 64, st
    finally:
        valu.gpu.enable_timing(False)


@pytest.fixture(scope="module")
def hier(tmp_path_factory):
    """more than 100 lists: the reference's build assigns through its two-level hierarchy, which does not guarantee that a
    record's list is the one its nearest centroid names (the 24-list fixtures have no such record)"""
    rng = np.random.default_rng(1)
    return Fixture(tmp_path_factory.mktemp("hier"), rng.standard_normal((3000, 32)).astype(np.float32), 104)


def test_a_record_whose_own_list_is_not_probed_gets_the_plain_top_k(hier):
    base = hier
    assert base.unprobed.size >= 5 and np.isin(base.unprobed[:5], base.rows).all()
    D, I = base.full(1)
    probed = own_entries(D, I, base.ext[base.rows]).any(axis=1)
    assert (~probed).any() and probed.any(), "no chosen record has its own list unprobed at n_probe 1"
    rows = np.nonzero(~probed)[0]
    for k in (1, 10):
        De, Ie, ce = base.expected(k, 1, True)
        Dp, Ip, cp = base.expected(k, 1, False)
        assert np.array_equal(Ie[rows], Ip[rows])        # nothing is there to delete
        Dg, Ig, cg, _, _ = raw_by_ids(base.gpu, base.ext[base.rows], k, 1, True)
        assert_rows((Dg, Ig, cg), (De, Ie, ce), f"n_probe 1 k {k}")
        Ds, Is = base.gpu.search_sync(base.X[base.rows[rows]], k, 1)
        assert np.array_equal(Ig[rows], Is) and np.array_equal(bits(Dg[rows]), bits(Ds))


# ---- duplicates ----
@pytest.fixture(scope="module")
def dups(tmp_path_factory):
    rng = np.random.default_rng(23)
    n = 1500
    X = rng.standard_normal((n, 32)).astype(np.float32)
    ext = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    ext[900] = ext[100]                   # one id, two vectors
    X[1000] = X[200]                      # one vector, two ids
    ext[1100], X[1100] = ext[300], X[300]   # both shared
    return Fixture(tmp_path_factory.mktemp("dups"), X, 8, ext=ext)


def test_duplicate_ids_and_copied_vectors(dups):
    fx, n = dups, dups.n
    shared, a, b = fx.ext[100], fx.ext[200], fx.ext[1000]
    cnt, Xg, _, where = fx.gpu.get([shared])
    assert cnt[0] == 2
    # the row of the shared id is the row of the record get() reports: its vector, less exactly that record
    D, I, counts, found, _ = raw_by_ids(fx.gpu, [shared], n, 10_000, True)
    assert found[0] == 2 and counts[0] == n - 1
    Do, Io = fx.sequences(Xg, 10_000)
    assert (Io >= 0).sum() == n
    want = take_k(Do, Io, (Io >= 0) & ~own_entries(Do, Io, u64([shared])), n)
    assert_rows((D, I, counts), want, "shared id")
    assert (I[0] == int(shared)).sum() == 1 and bits(D[0][I[0] == int(shared)])[0] != 0   # the other carrier stays
    # a copied vector: the twin stays, at distance bits 0, first
    for me, twin in ((a, b), (b, a)):
        D, I, counts, found, _ = raw_by_ids(fx.gpu, [me], 10, 10_000, True)
        assert found[0] == 1 and I[0, 0] == int(twin) and bits(D[0, :2])[0] == 0 and bits(D[0, :2])[1] != 0
        assert int(me) not in I[0].tolist()
    # id and vector shared: one of the pair goes, the other stays at distance bits 0
    D, I, counts, found, _ = raw_by_ids(fx.gpu, [fx.ext[300]], 10, 10_000, True)
    assert found[0] == 2 and I[0, 0] == int(fx.ext[300]) and bits(D[0])[0] == 0
    assert (I[0] == int(fx.ext[300])).sum() == 1
    D, I, counts, found, _ = raw_by_ids(fx.gpu, [fx.ext[300]], 10, 10_000, False)
    assert (I[0, :2] == int(fx.ext[300])).all() and (bits(D[0, :2]) == 0).all()


# ---- absent and repeated ids ----
def test_absent_and_repeated_ids(base, hip, monkeypatch):
    present = base.ext[base.rows[:20]]
    absent = u64([U64_MAX, U64_MAX - 1, (1 << 50) + 12345, 5])
    assert not np.isin(absent, base.ext).any()
    # absent at the first row, in the middle, as a whole chunk of 4 (rows 12..15 at VI_GRAPH_CHUNK 4) and at the last row
    ids = np.concatenate([absent[:1], present[:6], absent[1:2], np.full(4, present[3], dtype=np.uint64), np.tile(absent[2:3], 4),
                          present[6:], absent[3:4]])
    assert np.isin(ids[12:16], absent).all()
    is_absent = np.isin(ids, absent)
    pos = {int(e): i for i, e in enumerate(base.ext[base.rows])}
    sel = np.array([pos[int(e)] for e in ids[~is_absent]])
    for chunk in ("4", None):
        if chunk is None:
            monkeypatch.delenv("VI_GRAPH_CHUNK", raising=False)
        else:
            monkeypatch.setenv("VI_GRAPH_CHUNK", chunk)
        for exclude in (True, False):
            # (k = 64: k + 1 crosses the engine boundary of the excluding call)
            for k, p in [(10, 8), (64, 8)] + ([(200, 8)] if chunk is None else []):
                D, I, counts, found, _, V = raw_by_ids(base.gpu, ids, k, p, exclude, want_v=True)      # VI_OK
                assert base.gpu.similar_times()["chunk_rows"] == int(chunk or 65536)     # the knob reached the call
                assert (found == np.where(is_absent, 0, 1)).all() and (counts[is_absent] == 0).all()
                assert np.isposinf(D[is_absent]).all() and (I[is_absent] == -1).all() and (V[is_absent] == 0).all()
                De, Ie, ce = base.expected(k, p, exclude)
                assert_rows((D[~is_absent], I[~is_absent], counts[~is_absent]), (De[sel], Ie[sel], ce[sel]),
                            f"mixed chunk {chunk} k {k} exclude {exclude}")
                rep = np.nonzero(ids == present[3])[0]
                assert rep.size == 5 and all(np.array_equal(I[rep[0]], I[r]) and np.array_equal(bits(D[rep[0]]), bits(D[r]))
                                             and np.array_equal(V[rep[0]], V[r]) for r in rep)
                # the vectors are the stored vectors of the hits
                hit = I[~is_absent] >= 0
                assert np.array_equal(V[~is_absent][hit], base.X[base.rows_of(I[~is_absent][hit])])
                Dd, Id, Td, Fd = device_by_ids(hip, base.gpu, ids, k, p, exclude)
                assert np.array_equal(Id, I) and np.array_equal(bits(Dd), bits(D)) and np.array_equal(Fd, found)
                assert (Td[is_absent] == U64_MAX).all() and (Td[Id == -1] == U64_MAX).all() and (Td[Id >= 0] != U64_MAX).all()
            D, I, counts, found, _ = raw_by_ids(base.gpu, absent, 10, 8, exclude)   # only absent ids: VI_OK
            assert np.isposinf(D).all() and (I == -1).all() and (counts == 0).all() and (found == 0).all()
    D, I, found = base.gpu.search_by_ids(np.zeros(0, dtype=np.uint64), 10, 8)
    assert D.shape == (0, 10) and found.size == 0


# ---- the timing report ----
def test_timing_report_counts_the_drop_kernels_bytes(base, monkeypatch):
    """VI_SIMILAR_TIMING: drop_bytes is what self_drop_kernel reads and writes per row — D, I and slots of k + 1 entries
    (20 bytes each), D and I of the k output entries (12 bytes each, 20 with the slots a gather of V needs) and the row's
    count, slot and found words (16 bytes, the count read and written); the three spans are measured.  Without the
    variable the spans are 0; the bytes are counted all the same."""
    n, k = 30, 10
    ids = base.ext[base.rows[:n]]
    monkeypatch.setenv("VI_GRAPH_CHUNK", "4")
    monkeypatch.setenv("VI_SIMILAR_TIMING", "1")
    for want_v, out_entry in ((False, 12), (True, 20)):
        raw_by_ids(base.gpu, ids, k, 8, True, want_v=want_v)
        tm = base.gpu.similar_times()
        print("similar_times", want_v, tm)
        assert tm["chunk_rows"] == 4 and tm["drop_bytes"] == n * ((k + 1) * 20 + k * out_entry + 16), tm
        assert tm["ms_resolve"] > 0 and tm["ms_search"] > 0 and tm["ms_drop"] > 0, tm
    monkeypatch.delenv("VI_SIMILAR_TIMING")
    raw_by_ids(base.gpu, ids, k, 8, True)
    assert base.gpu.similar_times() == {"ms_resolve": 0.0, "ms_search": 0.0, "ms_drop": 0.0,
                                        "drop_bytes": n * ((k + 1) * 20 + k * 12 + 16), "chunk_rows": 4}


# ---- with a filter ----
def test_with_a_filter(base, tmp_path):
    ids = base.ext[base.rows]
    deny = np.concatenate([ids[:40], base.ext[np.setdiff1d(np.arange(base.n), base.rows)[:500]]])
    flt = base.gpu.filter_timestamps(*HALF) & base.gpu.filter_ids(deny, exclude=True)

    def admit(I):
        rows = base.rows_of(I)
        s = base.ts[rows]
        return (s >= np.uint64(HALF[0])) & (s <= np.uint64(HALF[1])) & ~np.isin(base.ext[rows], deny)

    for exclude in (True, False):
        for k, p in [(10, 8), (64, 8), (128, 24), (200, 8)]:
            D, I, counts, found, _ = raw_by_ids(base.gpu, ids, k, p, exclude, flt=flt)
            assert (found == 1).all()          # a row exists whether or not the filter admits its record
            assert_rows((D, I, counts), base.expected(k, p, exclude, admit), f"filtered k {k} n_probe {p} exclude {exclude}")
    # the rows of denied records: their own hit is already gone, exclusion removes nothing more
    De, Ie, _ = base.expected(10, 8, True, admit)
    Dp, Ip, _ = base.expected(10, 8, False, admit)
    assert np.array_equal(Ie[:40], Ip[:40]) and not np.array_equal(Ie[40:], Ip[40:])
    # a filter made before an add is rejected afterwards
    rng = np.random.default_rng(31)
    X = rng.standard_normal((500, 8)).astype(np.float32)
    ix = vip.build(X, str(tmp_path), now_secs=NOW)
    old = ix.filter_ids([1, 2, 3], exclude=True)
    ix.search_by_ids([5, 6], 5, 4, filter=old)
    ix.add(rng.standard_normal((10, 8)).astype(np.float32))
    for call in (lambda: ix.search_by_ids([5, 6], 5, 4, filter=old), lambda: ix.knn_graph(5, 4, filter=old)):
        with pytest.raises(vip.ViError) as e:
            call()
        assert e.value.kind == "InvalidInput"
    D, I, found = ix.search_by_ids([5, 509], 5, 4, filter=ix.filter_ids([1, 2, 3], exclude=True))
    assert (found == 1).all()


# ---- max_k ----
def test_max_k_clamps_the_callers_k_not_the_extra_candidate(base):
    cfg, keep = vip._config(base.dim, base.idx, base.sh, max_k=10)
    h = C.c_void_p()
    N.check(N.lib().vi_indexer_load(C.byref(cfg), C.byref(h)))
    ix = vip.VectorIndex(h, base.dim, keep)
    D, I, counts, found, kk = raw_by_ids(ix, base.ext[base.rows], 50, 8, True)
    assert kk == 10 and D.shape == (NROWS, 10)
    assert_rows((D, I, counts), base.expected(10, 8, True), "max_k 10, k 50")
    assert (counts == 10).all() and ix.last_stats()["k"] == 10


# ---- the k-NN graph ----
@pytest.fixture(scope="module")
def graph_expected(base):
    """rows of the whole list order of `base` at k 10, n_probe 8, from the oracle, by the ids export() reports"""
    ext_e, X_e, _, _ = base.gpu.export()
    assert np.array_equal(np.sort(ext_e), np.sort(base.ext))
    out = {True: [], False: []}
    for at in range(0, base.n, ORACLE_CHUNK):
        D, I = base.sequences(X_e[at:at + ORACLE_CHUNK], 8)
        own = own_entries(D, I, ext_e[at:at + ORACLE_CHUNK])
        for exclude in (True, False):
            out[exclude].append(take_k(D, I, (I >= 0) & ~(own & exclude), 10))
    return {e: tuple(np.concatenate([c[j] for c in out[e]]) for j in range(3)) for e in out}, ext_e


def raw_graph(index, first, count, k, n_probe, exclude, flt=None):
    D, I = np.full((count, k), 7.0, dtype=np.float32), np.full((count, k), 7, dtype=np.int64)
    counts, kout = np.full(count, 7, dtype=np.uint64), C.c_uint64(0)
    st = N.lib().vi_indexer_knn_graph(index._h, flt._h if flt is not None else None, first, count, k, n_probe,
                                      1 if exclude else 0, N.ptr(D), N.ptr(I), N.ptr(counts), C.byref(kout))
    return st, D, I, counts, int(kout.value)


@pytest.mark.parametrize("chunk", ["64", "1000", None])
def test_knn_graph_of_the_whole_index_and_a_sub_range(base, graph_expected, chunk, monkeypatch, hip):
    want, ext_e = graph_expected
    if chunk is None:
        monkeypatch.delenv("VI_GRAPH_CHUNK", raising=False)
    else:
        monkeypatch.setenv("VI_GRAPH_CHUNK", chunk)
    for exclude in (True, False):
        st, D, I, counts, kk = raw_graph(base.gpu, 0, base.n, 10, 8, exclude)
        assert st == N.VI_OK and kk == 10
        assert base.gpu.similar_times()["chunk_rows"] == int(chunk or 65536)     # the knob reached the call
        assert_rows((D, I, counts), want[exclude], f"graph chunk {chunk} exclude {exclude}")
        if exclude:
            assert (I != ext_e.astype(np.int64)[:, None]).all()     # (unique ids: no row holds its own record)
        # a chunk border inside a list, `first` inside a block
        st, Ds, Is, cs, _ = raw_graph(base.gpu, 70, 1000, 10, 8, exclude)
        assert st == N.VI_OK
        assert_rows((Ds, Is, cs), tuple(w[70:1070] for w in want[exclude]), f"sub-range chunk {chunk} exclude {exclude}")
        # host and device entries agree; the tie keys are those of the by-id device entry for the same records
        Dp, Ip, Tp = hip.alloc(1000 * 10 * 4), hip.alloc(1000 * 10 * 8), hip.alloc(1000 * 10 * 8)
        base.gpu.knn_graph_device(70, 1000, 10, 8, Dp, Ip, Tp, exclude_self=exclude)
        Dd, Id, Td = hip.download(Dp, (1000, 10), np.float32), hip.download(Ip, (1000, 10), np.int64), hip.download(Tp, (1000, 10), np.uint64)
        assert np.array_equal(Id, Is) and np.array_equal(bits(Dd), bits(Ds))
        _, Ib, Tb, _ = device_by_ids(hip, base.gpu, ext_e[70:1070], 10, 8, exclude)
        assert np.array_equal(Ib, Is) and np.array_equal(Tb, Td)
    Dw, Iw = base.gpu.knn_graph(10, 8, first=5990)
    assert Dw.shape == (10, 10) and np.array_equal(Iw, want[True][1][5990:])


def test_knn_graph_by_ordinal_on_duplicates(dups, monkeypatch):
    monkeypatch.setenv("VI_GRAPH_CHUNK", "64")
    ext_e, X_e, _, _ = dups.gpu.export()
    D, I = dups.sequences(X_e, 8)
    for exclude in (True, False):
        want = take_k(D, I, (I >= 0) & ~(own_entries(D, I, ext_e) & exclude), 10)
        st, Dg, Ig, cg, _ = raw_graph(dups.gpu, 0, dups.n, 10, 8, exclude)
        assert st == N.VI_OK
        assert_rows((Dg, Ig, cg), want, f"duplicates exclude {exclude}")
    # both carriers of the shared id have a row of their own, with their own vectors
    j = np.nonzero(ext_e == dups.ext[100])[0]
    assert j.size == 2 and not np.array_equal(Ig[j[0]], Ig[j[1]])


def test_knn_graph_range_past_the_end_is_an_error_and_writes_nothing(base, hip):
    for first, count in ((0, base.n + 1), (base.n, 1), (5000, 1001), (U64_MAX, 2)):
        D, I = np.full((8, 10), 7.0, dtype=np.float32), np.full((8, 10), 7, dtype=np.int64)
        counts, kout = np.full(8, 7, dtype=np.uint64), C.c_uint64(7)
        st = N.lib().vi_indexer_knn_graph(base.gpu._h, None, first, count, 10, 8, 1, N.ptr(D), N.ptr(I), N.ptr(counts), C.byref(kout))
        assert st == N.VI_ERR_INVALID_INPUT and N.lib().vi_last_error(), (first, count)
        assert (D == 7.0).all() and (I == 7).all() and (counts == 7).all() and kout.value == 7
        assert N.lib().vi_indexer_knn_graph_device(base.gpu._h, None, first, count, 10, 8, 1, hip.alloc(64), hip.alloc(64),
                                                   None) == N.VI_ERR_INVALID_INPUT
    st, D, I, counts, _ = raw_graph(base.gpu, base.n, 0, 10, 8, True)     # an empty range at the end: VI_OK, nothing touched
    assert st == N.VI_OK


# ---- partitioned handles ----
def test_partitioned_handles_are_rejected_with_advice(base, hip):
    part = base.open(rank=0, world_size=2)
    ids = base.ext[:4]
    D, I = np.full((4, 5), 7.0, dtype=np.float32), np.full((4, 5), 7, dtype=np.int64)
    L, h = N.lib(), part._h
    dD, dI, dids = hip.alloc(4 * 5 * 4), hip.alloc(4 * 5 * 8), hip.upload(ids)
    for call in (lambda: L.vi_indexer_search_by_ids(h, None, N.ptr(ids), 4, 5, 8, 1, N.ptr(D), N.ptr(I), None, None, None, None),
                 lambda: L.vi_indexer_search_by_ids_device(h, None, dids, 4, 5, 8, 1, dD, dI, None, None),
                 lambda: L.vi_indexer_knn_graph(h, None, 0, 4, 5, 8, 1, N.ptr(D), N.ptr(I), None, None),
                 lambda: L.vi_indexer_knn_graph_device(h, None, 0, 4, 5, 8, 1, dD, dI, None)):
        assert call() == N.VI_ERR_INVALID_INPUT
        msg = L.vi_last_error()
        assert b"get_records_device" in msg and b"where" in msg and b"probe" in msg, msg
    assert (D == 7.0).all() and (I == 7).all()


# ---- threads ----
def test_eight_threads_search_by_ids_and_get_on_one_handle(base):
    ids = base.ext[base.rows]
    parts = [ids[i::8][:30] for i in range(8)]
    want = [base.gpu.search_by_ids(p, 10, 8) for p in parts]
    want_get = [base.gpu.get(p) for p in parts]
    errors = []

    def worker(t):
        try:
            for _ in range(4):
                D, I, found = base.gpu.search_by_ids(parts[t], 10, 8)
                assert np.array_equal(I, want[t][1]) and np.array_equal(bits(D), bits(want[t][0])) and (found == 1).all()
                cnt, X, ts, where = base.gpu.get(parts[t])
                assert np.array_equal(X, want_get[t][1]) and np.array_equal(where, want_get[t][3])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,), daemon=True) for t in range(8)]
    [t.start() for t in threads]
    [t.join(timeout=60) for t in threads]
    assert not any(t.is_alive() for t in threads), "deadlock: a thread is still waiting for a context"
    assert not errors, errors
    De, Ie, _ = base.expected(10, 8, True)
    pos = {int(e): i for i, e in enumerate(ids)}
    sel = np.array([pos[int(e)] for e in parts[0]])
    assert np.array_equal(want[0][1], Ie[sel]) and np.array_equal(bits(want[0][0]), bits(De[sel]))


# ---- the Python surface ----
def test_python_surface(base):
    from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig
    ix = VectorIndexer.load(VectorIndexerConfig.new(base.dim).with_index_dir(base.idx).with_shards_dir(base.sh))
    De, Ie, ce = base.expected(10, 8, True)
    for i in (0, 1, 77):
        me = int(base.ext[base.rows[i]])
        res = ix.search_similar(me, k=10, n_probe=8, include_vectors=True)
        assert len(res) == 10 and me not in [r.external_id for r in res]
        assert [r.external_id for r in res] == Ie[i].tolist()
        assert np.array_equal(bits([r.distance for r in res]), bits(De[i]))
        assert np.array_equal(np.array([r.vector for r in res], dtype=np.float32), base.X[base.rows_of(Ie[i])])
        with_self = ix.search_similar(me, k=10, n_probe=8, exclude_self=False)
        assert with_self[0].external_id == me and with_self[0].distance == 0.0
        near = ix.search_similar(me, k=10, n_probe=8, excluded_ids=[Ie[i][0]], timestamp_range=(0, U64_MAX))
        assert near[0].external_id == Ie[i][1]
    assert ix.search_similar(U64_MAX, k=10, n_probe=8) is None
    assert len(ix.search_similar(int(base.ext[0]))) == ix.config().default_k
    with pytest.raises(ValueError):
        ix.search_similar(1, allowed_ids=[1], excluded_ids=[2])
    D, I, V, found = base.gpu.search_by_ids(base.ext[base.rows], 10, 8, include_vectors=True)
    assert np.array_equal(I, Ie) and np.array_equal(bits(D), bits(De)) and (found == 1).all() and V.shape == (NROWS, 10, base.dim)
