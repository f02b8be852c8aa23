"""GPU: searches filtered by external id — vi_indexer_filter_ids (allow / deny sets), vi_indexer_filter_ids_device and
vi_filter_intersect — on all three engines, the radius search and the per-rank merge.

The contract: the filtered result of a query is the reference's candidate sequence with the candidates whose external id
is not in the set (ALLOW) / is in the set (DENY) deleted, then the reference's stable sort and take(k).  The expected
results come from the untouched oracle: OracleIndex.search_batch with k = N returns the whole candidate sequence already
stable-sorted; keeping the entries with np.isin(I, ids) != exclude and the first k of them is the filtered answer.  Ids,
distance bits, counts and padding must match exactly."""
import ctypes as C
import threading

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from vector_indexer_py import _native as N

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000
U64_MAX = (1 << 64) - 1
EVERYTHING, HALF = (0, U64_MAX), (1000, 1499)
ALLOW, DENY = False, True
SOME_SHAPES = [(1, 1, 1), (33, 10, 8), (300, 100, 10_000), (300, 10, 8), (33, 100, 1)]
SWEEP_SHAPES = SOME_SHAPES[:3]
SET_NAMES = ["empty", "one", "all", "n63", "n64", "n65", "tenth", "half", "mostly_absent", "repeated", "odd"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def ext_ids_for(n):
    """ids that break weak hashing: many differ only above bit 32; all below 2^63; one record carries 0"""
    i = np.arange(n, dtype=np.uint64)
    ext = ((i % np.uint64(5)) << np.uint64(40)) | (np.uint64(7) * i + np.uint64(3))
    ext[n // 3] = 0
    assert np.unique(ext).size == n and int(ext.max()) < 1 << 63
    return ext


def timestamps_for(n):
    i = np.arange(n, dtype=np.uint64)
    return np.uint64(1000) + (i * np.uint64(7919)) % np.uint64(1000)


class Fixture:
    """one index written once by the oracle and opened by both sides; the oracle's full sorted candidate sequences per
    n_probe and the id sets are made once and shared by the tests"""

    def __init__(self, root, X, nlist, Q, seed=0):
        self.X, self.Q = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)
        n = X.shape[0]
        self.n, self.dim = n, X.shape[1]
        self.ext, self.ts = ext_ids_for(n), timestamps_for(n)
        self._sorted, self._order = np.sort(self.ext), np.argsort(self.ext)
        self.idx, self.sh = str(root / "index"), str(root / "shards")
        self.orc = O.OracleIndex.build(self.X, self.idx, self.sh, ext_ids=self.ext, timestamps=self.ts, nlist=nlist, now=NOW)
        self.gpu = self.open()
        assert self.gpu.num_vectors == n
        self.nlists = self.gpu.num_centroids
        self._full, self._filters = {}, {}
        self.sets = self.make_sets(np.random.default_rng(100 + seed))

    def open(self, **kw):
        return vip.load(self.idx, self.sh, self.dim, **kw)

    def rows_of(self, I):
        return self._order[np.searchsorted(self._sorted, np.where(I >= 0, I, 0).astype(np.uint64))]

    def full(self, n_probe):
        p = min(n_probe, self.nlists)
        if p not in self._full:
            rc, D, I = self.orc.search_batch(self.Q, self.n, p)
            assert rc == O.ORC_OK
            D.setflags(write=False), I.setflags(write=False)
            self._full[p] = (D, I)
        return self._full[p]

    def make_sets(self, rng):
        ext, n = self.ext, self.n
        pick = lambda m: ext[rng.choice(n, m, replace=False)]  # noqa: E731
        # "tenth": 10 % of the records, drawn so that query 0 keeps exactly 5 of the candidates its 8 nearest lists hold
        # (found = 5 < k = 10 at the shape (33, 10, 8)): 5 of its candidates and 595 records it does not reach
        _, I8 = self.full(8)
        reach = np.unique(self.rows_of(I8[0][I8[0] >= 0]))
        beyond = np.setdiff1d(np.arange(n), reach)
        if beyond.size >= n // 10 - 5:
            tenth = np.concatenate([ext[rng.choice(reach, 5, replace=False)], ext[rng.choice(beyond, n // 10 - 5, replace=False)]])
        else:   # (a single list: every query reaches everything)
            tenth = pick(n // 10)
        absent = (np.uint64(1) << np.uint64(50)) + np.arange(19_400, dtype=np.uint64) * np.uint64(0x10000001)
        flipped = ext[rng.choice(n, 500, replace=False)] ^ (np.uint64(1) << np.uint64(40))
        flipped = flipped[~np.isin(flipped, ext)]   # (such an id must not be another record's id)
        assert flipped.size >= 400 and not np.isin(absent, ext).any()
        sets = {"empty": np.zeros(0, dtype=np.uint64), "one": ext[17:18].copy(), "all": rng.permutation(ext),
                "n63": pick(63), "n64": pick(64), "n65": pick(65), "tenth": rng.permutation(tenth), "half": pick(n // 2),
                "mostly_absent": rng.permutation(np.concatenate([pick(600), absent])),
                "repeated": np.full(20_000, ext[4321], dtype=np.uint64),
                "odd": np.concatenate([u64([0, U64_MAX]), flipped])}
        assert sets["mostly_absent"].size == 20_000 and int(np.isin(ext, sets["odd"]).sum()) == 1
        for s in sets.values():
            s.setflags(write=False)
        return sets

    def ids(self, name):
        return self.sets[name] if isinstance(name, str) else name

    def filter(self, name, exclude, index=None):
        if index is not None:
            return index.filter_ids(self.ids(name), exclude=exclude)
        if (name, exclude) not in self._filters:
            self._filters[(name, exclude)] = self.gpu.filter_ids(self.sets[name], exclude=exclude)
        return self._filters[(name, exclude)]

    def matched(self, name):
        return int(np.isin(self.ext, self.ids(name)).sum())

    def keep(self, name, exclude, nq, n_probe, window=None):
        """(D, I, mask) of the oracle's sorted candidates of the first nq queries: mask = survives the filter(s)"""
        D, I = self.full(n_probe)
        D, I = D[:nq], I[:nq]
        keep = (I >= 0) & (np.isin(np.where(I >= 0, I, 0).astype(np.uint64), self.ids(name)) != exclude)
        if window is not None:
            s = self.ts[self.rows_of(I)]
            keep &= (s >= np.uint64(window[0])) & (s <= np.uint64(window[1]))
        return D, I, keep

    def expected(self, name, exclude, nq, k, n_probe, window=None):
        D, I, keep = self.keep(name, exclude, nq, n_probe, window)
        rank = np.cumsum(keep, axis=1) - 1
        take = keep & (rank < k)
        De, Ie = np.full((nq, k), np.inf, dtype=np.float32), np.full((nq, k), -1, dtype=np.int64)
        r, c = np.nonzero(take)
        De[r, rank[r, c]], Ie[r, rank[r, c]] = D[r, c], I[r, c]
        return De, Ie, np.minimum(keep.sum(axis=1), k)

    def check(self, name, exclude, nq, k, n_probe, index=None, flt=None, window=None):
        De, Ie, cnt = self.expected(name, exclude, nq, k, n_probe, window)
        gpu = index or self.gpu
        Dg, Ig = gpu.search_sync(self.Q[:nq], k, n_probe, filter=flt or self.filter(name, exclude))
        bad = np.nonzero((Ig != Ie).any(axis=1) | (bits(Dg) != bits(De)).any(axis=1))[0]
        what = name if isinstance(name, str) else "ids"
        assert bad.size == 0, (f"set {what} exclude {exclude} nq {nq} k {k} n_probe {n_probe}: {bad.size} queries differ, first "
                               f"{bad[0]}: gpu {Ig[bad[0]][:12]} {Dg[bad[0]][:12]} expected {Ie[bad[0]][:12]} {De[bad[0]][:12]}")
        assert ((Ig >= 0).sum(axis=1) == cnt).all()
        return cnt


def queries(rng, X, nq, integer=False):
    near = X[rng.integers(0, X.shape[0], nq - 40)]
    near = near + (rng.integers(-3, 4, size=near.shape) if integer else 0.3 * rng.standard_normal(near.shape))
    Q = np.concatenate([X[:40], near]).astype(np.float32)   # stored vectors first: distance 0.0 unless filtered out
    return np.clip(Q, 0, 254) if integer else Q


@pytest.fixture(scope="module")
def base(tmp_path_factory):         # D = 32: the MFMA engine; 250-vector lists end in a ragged block
    rng = np.random.default_rng(1)
    X = rng.standard_normal((6000, 32)).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("base"), X, 24, queries(rng, X, 300), seed=1)


@pytest.fixture(scope="module")
def valu(tmp_path_factory):         # D % 4 != 0: the exact-order VALU engine
    rng = np.random.default_rng(3)
    X = rng.standard_normal((6000, 10)).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("valu"), X, 24, queries(rng, X, 300), seed=3)


@pytest.fixture(scope="module")
def bytes8(tmp_path_factory):       # 8-bit descriptors with integer queries: the int8 rank kernel
    rng = np.random.default_rng(5)
    centers = rng.integers(40, 216, size=(24, 128))
    X = np.clip(centers[rng.integers(0, 24, 6000)] + rng.integers(-40, 41, size=(6000, 128)), 0, 255).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("bytes"), X, 24, queries(rng, X, 300, integer=True), seed=5)


def test_the_tenth_set_leaves_a_query_short_by_construction(base):
    _, _, cnt = base.expected("tenth", ALLOW, 33, 10, 8)
    assert cnt[0] == 5 and base.sets["tenth"].size == 600 == base.matched("tenth")


@pytest.mark.parametrize("name", SET_NAMES)
def test_every_set_in_both_modes(base, name):
    matched = base.matched(name)
    assert matched == {"empty": 0, "one": 1, "all": 6000, "n63": 63, "n64": 64, "n65": 65, "tenth": 600, "half": 3000,
                       "mostly_absent": 600, "repeated": 1, "odd": 1}[name]
    short = False
    for exclude in (ALLOW, DENY):
        # DENY: N - matched proves that no pad slot is admitted, whatever the set holds (0 is in "odd")
        assert base.filter(name, exclude).num_allowed == (base.n - matched if exclude else matched), (name, exclude)
        for nq, k, p in SWEEP_SHAPES:
            cnt = base.check(name, exclude, nq, k, p)
            short = short or bool(((cnt > 0) & (cnt < k)).any())
            if matched == (base.n if exclude else 0):
                assert (cnt == 0).all()
    if name in ("one", "n63", "n64", "n65", "tenth", "repeated", "odd"):
        assert short, "no query was left with fewer than k (and more than 0) allowed candidates"
    assert base.gpu.last_stats()["rank_mode"] >= 1


def device_search(hip, index, xq, nq, k, n_probe, flt):
    D, I, T = hip.alloc(nq * k * 4), hip.alloc(nq * k * 8), hip.alloc(nq * k * 8)
    index.search_device(xq, nq, k, n_probe, D, I, T, filter=flt)
    return hip.download(D, (nq, k), np.float32), hip.download(I, (nq, k), np.int64), hip.download(T, (nq, k), np.uint64)


def test_admitting_everything_equals_the_unfiltered_entry_and_admitting_nothing_is_ok(base):
    from hiprt import Hip
    hip = Hip()
    try:
        nq = 300
        xq = hip.upload(base.Q)
        for k, p in [(10, 8), (100, 24), (200, 8)]:
            Du, Iu, Tu = device_search(hip, base.gpu, xq, nq, k, p, None)
            for name, exclude in (("empty", DENY), ("all", ALLOW)):
                Df, If, Tf = device_search(hip, base.gpu, xq, nq, k, p, base.filter(name, exclude))
                assert np.array_equal(bits(Du), bits(Df)) and np.array_equal(Iu, If) and np.array_equal(Tu, Tf), (name, k, p)
            Dn, In, Tn = device_search(hip, base.gpu, xq, nq, k, p, base.filter("empty", ALLOW))   # VI_OK
            assert (In == -1).all() and np.isinf(Dn).all() and (Tn == U64_MAX).all()
        # n == 0 with a NULL set through the raw entry
        for mode, want in ((N.VI_IDS_ALLOW, 0), (N.VI_IDS_DENY, base.n)):
            h = C.c_void_p()
            N.check(N.lib().vi_indexer_filter_ids(base.gpu._h, None, 0, mode, C.byref(h)))
            assert N.lib().vi_filter_num_allowed(h) == want
            N.lib().vi_filter_free(h)
    finally:
        hip.close()


def engine_pass(fx):
    for name in ("tenth", "half"):
        for exclude in (ALLOW, DENY):
            for nq, k, p in SOME_SHAPES:
                fx.check(name, exclude, nq, k, p)


def test_valu_engine(valu):
    engine_pass(valu)
    assert valu.gpu.last_stats()["rank_mode"] == 0


@pytest.mark.parametrize("rank_i8", ["1", "0"])
def test_byte_lists(bytes8, rank_i8, monkeypatch):
    monkeypatch.setenv("VI_RANK_I8", rank_i8)
    engine_pass(bytes8)
    st = bytes8.gpu.last_stats()
    assert st["rank_mode"] == 3 and st["rank_int8"] == int(rank_i8), st


def test_forced_generic_engine(base, monkeypatch):
    monkeypatch.setenv("VI_FORCE_GENERIC", "1")
    engine_pass(base)
    assert base.gpu.last_stats()["rank_mode"] == 0


def test_generic_engine_beyond_the_select_limits(base):
    """k = 200 > 128 takes the sort-everything engine"""
    for name in ("tenth", "half"):
        for exclude in (ALLOW, DENY):
            for nq in (1, 33):
                base.check(name, exclude, nq, 200, 8)


def test_holes_in_one_list(tmp_path_factory):
    """nlist = 1: list order is record order; the denied records are whole 16-vector sub-blocks (four that start their
    block, one that does not) and one whole block — a denied slot in the middle of a list must rank like a pad slot"""
    rng = np.random.default_rng(9)
    X = rng.standard_normal((6000, 32)).astype(np.float32)
    holes = [5, 40, 41, 93]
    rows = np.concatenate([np.arange(64 * j, 64 * j + 16) for j in holes]
                          + [np.arange(64 * 70 + 16, 64 * 70 + 32), np.arange(64 * 80, 64 * 81)])
    Q = np.concatenate([X[64 * j + 3: 64 * j + 5] for j in holes] + [X[64 * 70 + 20: 64 * 70 + 22], X[64 * 80 + 1: 64 * 80 + 3],
                                                                    X[64 * 5 + 16: 64 * 5 + 20], queries(rng, X, 60)])
    fx = Fixture(tmp_path_factory.mktemp("holes"), X, 1, Q, seed=9)
    assert fx.nlists == 1
    ids = rng.permutation(fx.ext[rows])
    deny, allow = fx.gpu.filter_ids(ids, exclude=True), fx.gpu.filter_ids(ids)
    assert allow.num_allowed == 16 * len(holes) + 16 + 64 and deny.num_allowed == fx.n - allow.num_allowed
    for k in (1, 10, 100, 200):
        fx.check(ids, DENY, Q.shape[0], k, 1, flt=deny)
        fx.check(ids, ALLOW, Q.shape[0], k, 1, flt=allow)
    De, _, _ = fx.expected(ids, DENY, 2, 1, 1)
    assert (De[:, 0] > 0.0).all()   # the fixture does what it is for: the queries' own records are denied


def test_intersection_with_a_timestamp_window(base):
    ids_f, ts_f = base.filter("tenth", ALLOW), base.gpu.filter_timestamps(*HALF)
    both = ids_f & ts_f
    in_window = (base.ts >= HALF[0]) & (base.ts <= HALF[1])
    assert both.num_allowed == int((np.isin(base.ext, base.sets["tenth"]) & in_window).sum()) > 0
    for nq, k, p in SOME_SHAPES:
        base.check("tenth", ALLOW, nq, k, p, flt=both, window=HALF)
    deny_both = base.filter("half", DENY) & ts_f
    for nq, k, p in SOME_SHAPES[:3]:
        base.check("half", DENY, nq, k, p, flt=deny_both, window=HALF)
    # f & everything is f; a & b is b & a
    same, swapped = ids_f & base.gpu.filter_timestamps(*EVERYTHING), ts_f & ids_f
    assert same.num_allowed == ids_f.num_allowed and swapped.num_allowed == both.num_allowed
    for k, p in [(10, 8), (100, 10_000), (200, 8)]:
        Da, Ia = base.gpu.search_sync(base.Q, k, p, filter=ids_f)
        Db, Ib = base.gpu.search_sync(base.Q, k, p, filter=same)
        assert np.array_equal(Ia, Ib) and np.array_equal(bits(Da), bits(Db))
        Da, Ia = base.gpu.search_sync(base.Q, k, p, filter=both)
        Db, Ib = base.gpu.search_sync(base.Q, k, p, filter=swapped)
        assert np.array_equal(Ia, Ib) and np.array_equal(bits(Da), bits(Db))
    other = base.open()
    with pytest.raises(vip.ViError) as e:
        other.filter_ids(base.sets["tenth"]) & ids_f
    assert e.value.kind == "InvalidInput"
    with pytest.raises(vip.ViError) as e:
        ids_f & other.filter_timestamps(*HALF)
    assert e.value.kind == "InvalidInput"


def test_radius_search(base):
    nq, p = 300, 8
    D, I, keep = base.keep("tenth", ALLOW, nq, p)
    tenth_nearest = np.sort(np.where(keep, D, np.inf), axis=1)[:, 9]
    radius2 = float(np.median(tenth_nearest))
    hit = keep & (D <= np.float32(radius2))
    per = hit.sum(axis=1)
    assert (per == 0).any() and (per >= 10).any()   # some queries find nothing, some many
    lims_e = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    lims, Dg, Ig = base.gpu.range_search_sync(base.Q[:nq], radius2, p, filter=base.filter("tenth", ALLOW))
    assert np.array_equal(lims, lims_e) and np.array_equal(Ig, I[hit]) and np.array_equal(bits(Dg), bits(D[hit]))


def test_ids_in_device_memory(base):
    from hiprt import Hip
    hip = Hip()
    try:
        rng = np.random.default_rng(7)
        ids = rng.permutation(np.concatenate([base.sets["tenth"], base.sets["tenth"][:250], base.sets["n65"]]))
        assert np.unique(ids).size < ids.size and (np.diff(ids.astype(np.int64)) < 0).any()
        dev = hip.upload(ids)
        for exclude in (ALLOW, DENY):
            fd, fh = base.gpu.filter_ids_device(dev, ids.size, exclude=exclude), base.gpu.filter_ids(ids, exclude=exclude)
            matched = int(np.isin(base.ext, ids).sum())
            assert fd.num_allowed == fh.num_allowed == (base.n - matched if exclude else matched)
            for nq, k, p in SWEEP_SHAPES:
                base.check(ids, exclude, nq, k, p, flt=fd)
                Dd, Id = base.gpu.search_sync(base.Q[:nq], k, p, filter=fd)
                Dh, Ih = base.gpu.search_sync(base.Q[:nq], k, p, filter=fh)
                assert np.array_equal(Id, Ih) and np.array_equal(bits(Dd), bits(Dh))
    finally:
        hip.close()


@pytest.mark.parametrize("placement", [0, 1])
def test_two_ranks_each_with_its_own_filter_merge_to_the_single_gpu_result(base, placement):
    from hiprt import Hip
    world, nq = 2, 300
    parts = [base.open(rank=r, world_size=world, placement=placement) for r in range(world)]
    assert sum(p.num_vectors for p in parts) == base.n
    hip = Hip()
    try:
        xq = hip.upload(base.Q)
        for name, exclude in (("tenth", ALLOW), ("half", DENY), ("odd", DENY)):
            filters = [base.filter(name, exclude, index=p) for p in parts]
            assert sum(f.num_allowed for f in filters) == base.filter(name, exclude).num_allowed
            for k, n_probe in [(10, 8), (200, 8)]:
                De, Ie, _ = base.expected(name, exclude, nq, k, n_probe)
                S = int(N.lib().vi_packed_result_bytes(nq, k))
                off_i = (nq * k * 4 + 7) // 8 * 8
                packed, Dm, Im = hip.alloc(world * S), hip.alloc(nq * k * 4), hip.alloc(nq * k * 8)
                for r, p in enumerate(parts):
                    b = packed + r * S
                    p.search_device(xq, nq, k, n_probe, b, b + off_i, b + off_i + nq * k * 8, filter=filters[r])
                N.check(N.lib().vi_merge_partials_packed_device(0, nq, k, world, packed, Dm, Im))
                assert np.array_equal(hip.download(Im, (nq, k), np.int64), Ie), (name, k, n_probe)
                assert np.array_equal(bits(hip.download(Dm, (nq, k), np.float32)), bits(De)), (name, k, n_probe)
    finally:
        hip.close()


def test_uint64_max_as_a_stored_id(tmp_path):
    rng = np.random.default_rng(11)
    X = rng.standard_normal((200, 8)).astype(np.float32)
    ext = np.arange(200, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    ext[77] = U64_MAX
    ix = vip.build(X, str(tmp_path), ext_ids=ext, now_secs=NOW)
    assert ix.num_vectors == 200
    one = u64([U64_MAX])
    for ids, n_in in ((one, 1), (u64([U64_MAX, U64_MAX, 5]), 1), (u64([U64_MAX - 1, 4]), 1), (u64([U64_MAX - 1]), 0)):
        for mode in (N.VI_IDS_ALLOW, N.VI_IDS_DENY):
            h = C.c_void_p()
            N.check(N.lib().vi_indexer_filter_ids(ix._h, N.ptr(ids), ids.size, mode, C.byref(h)))
            assert N.lib().vi_filter_num_allowed(h) == (200 - n_in if mode == N.VI_IDS_DENY else n_in), (ids, mode)
            N.lib().vi_filter_free(h)
    D, I = ix.search_sync(X[77:78], 5, 10_000, filter=ix.filter_ids(one))
    assert D[0, 0] == 0.0 and np.isinf(D[0, 1:]).all() and I[0, 0] == -1   # (the id as an i64; the distance shows the hit)
    D, I = ix.search_sync(X[77:78], 5, 10_000, filter=ix.filter_ids(one, exclude=True))
    assert D[0, 0] > 0.0 and (I[0] >= 0).all()


def test_errors(base):
    ids = u64([1, 2, 3])
    h = C.c_void_p()
    for entry in (N.lib().vi_indexer_filter_ids, N.lib().vi_indexer_filter_ids_device):
        assert entry(base.gpu._h, N.ptr(ids), 3, 2, C.byref(h)) == N.VI_ERR_INVALID_INPUT and N.lib().vi_last_error()
        assert entry(base.gpu._h, N.ptr(ids), 3, -1, C.byref(h)) == N.VI_ERR_INVALID_INPUT
        assert entry(base.gpu._h, None, 3, N.VI_IDS_ALLOW, C.byref(h)) == N.VI_ERR_INVALID_INPUT
        assert entry(base.gpu._h, N.ptr(ids), 3, N.VI_IDS_ALLOW, None) == N.VI_ERR_INVALID_INPUT
    assert not h.value
    with pytest.raises(vip.ViError) as e:
        N.check(N.lib().vi_indexer_filter_ids(base.gpu._h, None, 3, N.VI_IDS_DENY, C.byref(h)))
    assert e.value.kind == "InvalidInput"
    f = base.filter("tenth", ALLOW)
    assert N.lib().vi_filter_intersect(base.gpu._h, f._h, None, C.byref(h)) == N.VI_ERR_INVALID_INPUT
    other = base.open()
    with pytest.raises(vip.ViError) as e:
        other.search_sync(base.Q[:3], 5, 4, filter=f)
    assert e.value.kind == "InvalidInput"


def test_four_threads_share_one_handle_and_one_filter(base):
    flt = base.filter("tenth", DENY)
    want = {i: base.gpu.search_sync(base.Q[i:i + 9], 10, 8, filter=flt) for i in range(16)}
    errors = []

    def worker(t):
        try:
            for rep in range(10):
                for i in range(t, 16, 4):
                    D, I = base.gpu.search_sync(base.Q[i:i + 9], 10, 8, filter=flt)
                    assert np.array_equal(I, want[i][1]) and np.array_equal(bits(D), bits(want[i][0]))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors
    De, Ie, _ = base.expected("tenth", DENY, 9, 10, 8)
    assert np.array_equal(want[0][1], Ie) and np.array_equal(bits(want[0][0]), bits(De))


def test_python_surface(base):
    from vector_indexer_py.api import SearchRequest, VectorIndexer, VectorIndexerConfig
    from vector_indexer_py.harness import FaissStyleAdapter
    ix = VectorIndexer.load(VectorIndexerConfig.new(base.dim).with_index_dir(base.idx).with_shards_dir(base.sh))
    ids = base.sets["tenth"]
    for q in (0, 1, 77):
        for k, p in [(10, 8), (100, 24)]:
            fx = Fixture.__new__(Fixture)
            fx.__dict__.update(base.__dict__)
            fx.Q, fx._full = base.Q[q:q + 1], {}
            req = SearchRequest(base.Q[q].tolist(), False, k, p).with_allowed_ids(ids.tolist()).with_timestamp_range(*HALF)
            res = ix.search(req)
            De, Ie, cnt = fx.expected("tenth", ALLOW, 1, k, p, window=HALF)
            assert len(res) == cnt[0]
            assert [r.external_id for r in res] == Ie[0, :cnt[0]].tolist()
            assert np.array_equal(bits([r.distance for r in res]), bits(De[0, :cnt[0]]))
            res = ix.search(SearchRequest(base.Q[q].tolist(), False, k, p).with_excluded_ids(ids))
            De, Ie, cnt = fx.expected("tenth", DENY, 1, k, p)
            assert [r.external_id for r in res] == Ie[0, :cnt[0]].tolist()
    assert len(ix._filters) == 4   # the window, the allow set, their intersection, the deny set: each made once
    D, I, keep = base.keep("tenth", ALLOW, 1, 8)
    radius2 = float(D[0][keep[0]][2])   # the third of query 0's five allowed candidates
    hit = keep[0] & (D[0] <= np.float32(radius2))
    res = ix.range_search(base.Q[0], radius2, 8, allowed_ids=ids)
    assert [r.external_id for r in res] == I[0][hit].tolist() and len(res) >= 3

    adapter = FaissStyleAdapter(base.gpu)
    adapter.nprobe = 8
    Da, Ia = adapter.search(base.Q[:33], 10, excluded_ids=ids)
    Ds, Is = base.gpu.search_sync(base.Q[:33], 10, 8, filter=base.filter("tenth", DENY))
    assert np.array_equal(Ia, Is) and np.array_equal(bits(Da), bits(Ds))
    Da, Ia = adapter.search(base.Q[:33], 10, allowed_ids=ids)
    base_De, base_Ie, _ = base.expected("tenth", ALLOW, 33, 10, 8)
    assert np.array_equal(Ia, base_Ie) and np.array_equal(bits(Da), bits(base_De))
    lims, Dr, Ir = adapter.range_search(base.Q[:1], radius2, allowed_ids=ids)
    assert Ir.tolist() == I[0][hit].tolist()
    Du, Iu = adapter.search(base.Q[:33], 10)
    assert np.array_equal(Iu, base.gpu.search_sync(base.Q[:33], 10, 8)[1])
    with pytest.raises(ValueError):
        adapter.search(base.Q[:3], 10, allowed_ids=ids, excluded_ids=ids)
    with pytest.raises(ValueError):
        adapter.range_search(base.Q[:3], 1.0, allowed_ids=ids, excluded_ids=ids)
