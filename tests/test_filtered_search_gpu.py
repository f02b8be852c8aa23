"""GPU: timestamp-window filtered search (vi_indexer_filter_timestamps, vi_indexer_search_filtered*) on all three engines.

The contract: the filtered result of a query is the reference's candidate sequence (probed lists in shard visiting order,
probe rank, list position — ivf_index.rs:223-262) with the candidates whose STORED timestamp lies outside the window
deleted, then the reference's stable sort and take(k).  The expected results therefore come from the untouched oracle:
OracleIndex.search with k = N returns the whole candidate sequence already stable-sorted; dropping the ids outside the
window and keeping the first k is the filtered answer.  Ids, distance bits, counts and padding must match exactly."""
import threading

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from vector_indexer_py import _native as N

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000
U64_MAX = (1 << 64) - 1
EVERYTHING, NOTHING, ONE_VALUE, TENTH, HALF, ONLY_NOW, FEW = \
    (0, U64_MAX), (5, 10), (1500, 1500), (1000, 1099), (1000, 1499), (NOW, NOW), (1500, 1502)
WINDOWS = [EVERYTHING, NOTHING, ONE_VALUE, TENTH, HALF, ONLY_NOW, FEW]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def timestamps_for(n):
    """spread over 1000 values; about 1 % of the records carry 0 and are stored with the build's `now`"""
    i = np.arange(n, dtype=np.uint64)
    ts = np.uint64(1000) + (i * np.uint64(7919)) % np.uint64(1000)
    ts[::97] = 0
    return ts


class Fixture:
    """one index written once by the oracle (now fixed) and opened by both sides; the oracle's full sorted candidate
    sequences per n_probe are computed once and shared by the tests"""

    def __init__(self, root, X, nlist, Q, ts=None):
        self.X, self.Q = np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)
        n = X.shape[0]
        self.n, self.dim = n, X.shape[1]
        self.ext = np.uint64(1_000_003) + np.uint64(7) * np.arange(n, dtype=np.uint64)  # unique, ascending in the row
        self.ts = timestamps_for(n) if ts is None else np.ascontiguousarray(ts, dtype=np.uint64)
        self.stored = np.where(self.ts == 0, np.uint64(NOW), self.ts)
        self.idx, self.sh = str(root / "index"), str(root / "shards")
        self.orc = O.OracleIndex.build(self.X, self.idx, self.sh, ext_ids=self.ext, timestamps=self.ts, nlist=nlist, now=NOW)
        self.gpu = vip.load(self.idx, self.sh, self.dim)
        assert self.gpu.num_vectors == n
        self.nlists = self.gpu.num_centroids
        self._full, self._filters = {}, {}

    def full(self, n_probe):
        p = min(n_probe, self.nlists)
        if p not in self._full:
            rc, D, I = self.orc.search_batch(self.Q, self.n, p)
            assert rc == O.ORC_OK
            row = np.where(I >= 0, (I - 1_000_003) // 7, 0)
            D.setflags(write=False), I.setflags(write=False), row.setflags(write=False)
            self._full[p] = (D, I, row)
        return self._full[p]

    def filter(self, window, index=None):
        if index is not None:
            return index.filter_timestamps(*window)
        if window not in self._filters:
            self._filters[window] = self.gpu.filter_timestamps(*window)
        return self._filters[window]

    def expected(self, window, nq, k, n_probe):
        """(D, I, counts) of the first nq queries: the oracle's sorted candidates inside the window, first k"""
        D, I, row = self.full(n_probe)
        D, I, row = D[:nq], I[:nq], row[:nq]
        s = self.stored[row]
        keep = (I >= 0) & (s >= np.uint64(window[0])) & (s <= np.uint64(window[1]))
        rank = np.cumsum(keep, axis=1) - 1
        take = keep & (rank < k)
        De, Ie = np.full((nq, k), np.inf, dtype=np.float32), np.full((nq, k), -1, dtype=np.int64)
        r, c = np.nonzero(take)
        De[r, rank[r, c]], Ie[r, rank[r, c]] = D[r, c], I[r, c]
        return De, Ie, np.minimum(keep.sum(axis=1), k)

    def check(self, window, nq, k, n_probe, index=None, flt=None):
        De, Ie, cnt = self.expected(window, nq, k, n_probe)
        gpu = index or self.gpu
        Dg, Ig = gpu.search_sync(self.Q[:nq], k, n_probe, filter=flt or self.filter(window))
        bad = np.nonzero((Ig != Ie).any(axis=1) | (bits(Dg) != bits(De)).any(axis=1))[0]
        assert bad.size == 0, (f"window {window} nq {nq} k {k} n_probe {n_probe}: {bad.size} queries differ, first {bad[0]}: "
                               f"gpu {Ig[bad[0]][:12]} {Dg[bad[0]][:12]} expected {Ie[bad[0]][:12]} {De[bad[0]][:12]}")
        assert ((Ig >= 0).sum(axis=1) == cnt).all()
        return cnt


def queries(rng, X, nq, integer=False):
    near = X[rng.integers(0, X.shape[0], nq - 40)]
    near = near + (rng.integers(-3, 4, size=near.shape) if integer else 0.3 * rng.standard_normal(near.shape))
    Q = np.concatenate([X[:40], near]).astype(np.float32)   # stored vectors first: distance 0.0 unless filtered out
    return np.clip(Q, 0, 254) if integer else Q


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((6000, 32)).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("base"), X, 24, queries(rng, X, 300))


@pytest.fixture(scope="module")
def long_lists(tmp_path_factory):   # ~47 blocks per list: a list crosses a 32-block segment of the MFMA engine
    rng = np.random.default_rng(2)
    X = rng.standard_normal((6000, 32)).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("long"), X, 2, queries(rng, X, 300))


@pytest.fixture(scope="module")
def valu(tmp_path_factory):         # D % 4 != 0: the exact-order VALU engine
    rng = np.random.default_rng(3)
    X = rng.standard_normal((6000, 10)).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("valu"), X, 24, queries(rng, X, 300))


@pytest.fixture(scope="module")
def wide(tmp_path_factory):         # D > 128: the wide rank kernel
    rng = np.random.default_rng(4)
    X = rng.standard_normal((6000, 200)).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("wide"), X, 24, queries(rng, X, 300))


@pytest.fixture(scope="module")
def bytes8(tmp_path_factory):       # 8-bit descriptors with integer queries: the int8 rank kernel
    rng = np.random.default_rng(5)
    centers = rng.integers(40, 216, size=(24, 128))
    X = np.clip(centers[rng.integers(0, 24, 6000)] + rng.integers(-40, 41, size=(6000, 128)), 0, 255).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("bytes"), X, 24, queries(rng, X, 300, integer=True))


SHAPES = [(nq, k, p) for nq in (1, 33, 300) for k in (1, 10, 100) for p in (1, 8, 10_000)]
SOME_SHAPES = [(1, 1, 1), (33, 10, 8), (300, 100, 10_000), (300, 10, 8), (33, 100, 1)]


def sweep(fx, shapes, windows=WINDOWS):
    """every window x shape against the oracle; the windows must reach a query with 0 < allowed candidates < k"""
    short = False
    for w in windows:
        for nq, k, p in shapes:
            cnt = fx.check(w, nq, k, p)
            short = short or bool(((cnt > 0) & (cnt < k)).any())
            if w == NOTHING:
                assert (cnt == 0).all()
    assert short, "no query was left with fewer than k (and more than 0) allowed candidates"


@pytest.mark.parametrize("nq", [1, 33, 300])
def test_every_window_and_batch_shape(base, nq):
    sweep(base, [s for s in SHAPES if s[0] == nq])
    assert base.gpu.last_stats()["rank_mode"] >= 1


def test_lists_longer_than_a_segment(long_lists):
    sweep(long_lists, SOME_SHAPES)
    assert long_lists.gpu.last_stats()["rank_mode"] >= 1


def test_valu_engine(valu):
    sweep(valu, SOME_SHAPES)
    assert valu.gpu.last_stats()["rank_mode"] == 0


def test_wide_vectors(wide):
    sweep(wide, SOME_SHAPES)
    assert wide.gpu.last_stats()["rank_mode"] == 2


@pytest.mark.parametrize("rank_i8", ["1", "0"])
def test_byte_lists(bytes8, rank_i8, monkeypatch):
    monkeypatch.setenv("VI_RANK_I8", rank_i8)
    sweep(bytes8, SOME_SHAPES)
    st = bytes8.gpu.last_stats()
    assert st["rank_mode"] == 3 and st["rank_int8"] == int(rank_i8), st


@pytest.mark.parametrize("env,modes", [({"VI_FILTER": "0"}, (0,)), ({"VI_FORCE_GENERIC": "1"}, (0,)), ({"VI_FILTER_BF16": "0"}, (1,)),
                                       ({"VI_RANK_APPROX": "0"}, (2, 5)), ({"VI_RANK_APPROX": "1"}, (4, 6)),
                                       ({"VI_RANK_APPROX": "2"}, (4, 6)),
                                       ({"VI_RANK_APPROX": "1", "VI_RANK_STREAM": "0"}, (4, 6)),
                                       ({"VI_RANK_APPROX": "1", "VI_RANK_STREAM": "1"}, (4, 6))],
                         ids=lambda v: "-".join(f"{a}={b}" for a, b in v.items()) if isinstance(v, dict) else None)
def test_engine_settings(base, env, modes, monkeypatch):
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    sweep(base, SOME_SHAPES)
    assert base.gpu.last_stats()["rank_mode"] in modes, base.gpu.last_stats()["rank_mode"]


def test_generic_engine_beyond_the_select_limits(base, long_lists):
    """k = 200 > 128 takes the sort-everything engine"""
    for w in WINDOWS:
        for nq in (1, 33):
            base.check(w, nq, 200, 8)
            long_lists.check(w, nq, 200, 2)


def test_generic_engine_more_probes_than_the_select_holds(tmp_path_factory):
    """n_probe = 80 > 64 on an index of 100 lists: the sort-everything engine, with k below and above 128"""
    rng = np.random.default_rng(6)
    X = rng.standard_normal((6000, 32)).astype(np.float32)
    fx = Fixture(tmp_path_factory.mktemp("many"), X, 100, queries(rng, X, 64))
    assert fx.nlists >= 80
    for w in WINDOWS:
        fx.check(w, 33, 10, 80)
        fx.check(w, 33, 200, 80)


def test_a_query_the_rank_arithmetic_cannot_be_trusted_for(base):
    """|q|^2 >= 1e30: the select trusts no rank value and re-evaluates everything the query probes — through the allow bits"""
    Q = np.concatenate([np.full((1, 32), 1.0e16, np.float32), base.X[:3]]).astype(np.float32)
    fx = Fixture.__new__(Fixture)
    fx.__dict__.update(base.__dict__)
    fx.Q, fx._full = Q, {}
    for w in (EVERYTHING, TENTH, ONE_VALUE, NOTHING):
        for k, p in [(10, 8), (100, 10_000)]:
            fx.check(w, 4, k, p)


def test_surviving_duplicates_keep_candidate_order(tmp_path_factory):
    rng = np.random.default_rng(8)
    X = rng.standard_normal((3000, 32)).astype(np.float32)
    dup = 50 + 71 * np.arange(40)
    X[dup] = X[dup[0]]
    Q = np.concatenate([X[dup[:1]], X[:31]])
    fx = Fixture(tmp_path_factory.mktemp("dups"), X, 12, Q)
    for w in WINDOWS + [(1000, 1799)]:
        for k, p in [(10, 12), (100, 12), (64, 3), (200, 12)]:
            fx.check(w, 32, k, p)
    De, Ie, cnt = fx.expected(HALF, 1, 100, 12)
    inside = int(((fx.stored[dup] >= 1000) & (fx.stored[dup] <= 1499)).sum())
    assert 0 < inside < 40 and (De[0, :inside] == 0.0).all() and De[0, inside] > 0.0   # the fixture does what it is for


def test_a_whole_sub_block_excluded_between_allowed_neighbours(tmp_path_factory):
    """nlist = 1: list order is id order; records 64 j .. 64 j + 15 (one 16-vector sub-block) are outside the window, their
    neighbours inside it — an excluded slot in the middle of a list must rank like a pad slot at its tail"""
    rng = np.random.default_rng(9)
    X = rng.standard_normal((6000, 32)).astype(np.float32)
    ts = np.full(6000, 1200, dtype=np.uint64)
    holes = [5, 40, 41, 93]
    for j in holes:
        ts[64 * j: 64 * j + 16] = 5000
    ts[64 * 70 + 16: 64 * 70 + 32] = 5000      # a sub-block that does not start its block
    ts[64 * 80: 64 * 81] = 5000                # a whole block
    Q = np.concatenate([X[64 * j + 3: 64 * j + 5] for j in holes] + [X[64 * 70 + 20: 64 * 70 + 22], X[64 * 80 + 1: 64 * 80 + 3],
                                                                    X[64 * 5 + 16: 64 * 5 + 20], queries(rng, X, 60)])
    fx = Fixture(tmp_path_factory.mktemp("holes"), X, 1, Q, ts=ts)
    assert fx.nlists == 1
    for w in [(1000, 1999), (5000, 5000), EVERYTHING]:
        for k in (1, 10, 100, 200):
            fx.check(w, Q.shape[0], k, 1)
    for env in ({"VI_FILTER": "0"}, {"VI_FILTER_BF16": "0"}, {"VI_RANK_APPROX": "1", "VI_RANK_STREAM": "1"}):
        mp = pytest.MonkeyPatch()
        try:
            for a, b in env.items():
                mp.setenv(a, b)
            fx.check((1000, 1999), Q.shape[0], 10, 1)
        finally:
            mp.undo()
    assert fx.filter((5000, 5000)).num_allowed == 16 * len(holes) + 16 + 64


def device_search(hip, index, xq, nq, k, n_probe, flt):
    D, I, T = hip.alloc(nq * k * 4), hip.alloc(nq * k * 8), hip.alloc(nq * k * 8)
    index.search_device(xq, nq, k, n_probe, D, I, T, filter=flt)
    return hip.download(D, (nq, k), np.float32), hip.download(I, (nq, k), np.int64), hip.download(T, (nq, k), np.uint64)


def test_all_admitting_filter_equals_the_unfiltered_entry_and_device_equals_host(base):
    from hiprt import Hip
    hip = Hip()
    try:
        nq = 300
        xq = hip.upload(base.Q)
        for k, p in [(10, 8), (100, 24), (200, 8)]:
            Du, Iu, Tu = device_search(hip, base.gpu, xq, nq, k, p, None)
            Df, If, Tf = device_search(hip, base.gpu, xq, nq, k, p, base.filter(EVERYTHING))
            assert np.array_equal(bits(Du), bits(Df)) and np.array_equal(Iu, If) and np.array_equal(Tu, Tf)
            Dh, Ih, Vh = base.gpu.search_sync(base.Q, k, p, include_vectors=True)
            Dg, Ig, Vg = base.gpu.search_sync(base.Q, k, p, include_vectors=True, filter=base.filter(EVERYTHING))
            assert np.array_equal(bits(Dh), bits(Dg)) and np.array_equal(Ih, Ig) and np.array_equal(Vh, Vg)
            for w in (TENTH, FEW):   # device entry against the host entry (which the other tests pin to the oracle)
                Dd, Id, Td = device_search(hip, base.gpu, xq, nq, k, p, base.filter(w))
                Dh, Ih = base.gpu.search_sync(base.Q, k, p, filter=base.filter(w))
                assert np.array_equal(bits(Dd), bits(Dh)) and np.array_equal(Id, Ih)
                assert ((Td == U64_MAX) == (Id == -1)).all()
    finally:
        hip.close()


def test_num_allowed_is_the_count_of_stored_timestamps_in_the_window(base):
    for w in WINDOWS:
        want = int(((base.stored >= np.uint64(w[0])) & (base.stored <= np.uint64(w[1]))).sum())
        assert base.filter(w).num_allowed == want, w
    assert base.filter(EVERYTHING).num_allowed == base.n and base.filter(NOTHING).num_allowed == 0
    assert base.filter(ONLY_NOW).num_allowed == int((base.ts == 0).sum()) > 0


def test_include_vectors_returns_the_stored_rows_of_the_survivors(base):
    for w in (TENTH, FEW, NOTHING):
        for k, p in [(10, 8), (100, 1)]:
            D, I, V = base.gpu.search_sync(base.Q[:33], k, p, include_vectors=True, filter=base.filter(w))
            De, Ie, _ = base.expected(w, 33, k, p)
            assert np.array_equal(I, Ie) and np.array_equal(bits(D), bits(De))
            rows = np.where(I >= 0, (I - 1_000_003) // 7, 0)
            want = np.where((I >= 0)[:, :, None], base.X[rows], np.float32(0.0))
            assert np.array_equal(V, want)


@pytest.mark.parametrize("placement", [0, 1])
def test_two_ranks_each_with_its_own_filter_merge_to_the_single_gpu_result(base, placement):
    from hiprt import Hip
    world, nq = 2, 300
    parts = [vip.load(base.idx, base.sh, base.dim, rank=r, world_size=world, placement=placement) for r in range(world)]
    assert sum(p.num_vectors for p in parts) == base.n
    hip = Hip()
    try:
        xq = hip.upload(base.Q)
        for w in (TENTH, FEW, EVERYTHING, NOTHING):
            filters = [p.filter_timestamps(*w) for p in parts]
            assert sum(f.num_allowed for f in filters) == base.filter(w).num_allowed
            for k, n_probe in [(10, 8), (100, 24), (200, 8)]:
                De, Ie, _ = base.expected(w, nq, k, n_probe)
                S = int(N.lib().vi_packed_result_bytes(nq, k))
                off_i = (nq * k * 4 + 7) // 8 * 8
                packed, Dm, Im = hip.alloc(world * S), hip.alloc(nq * k * 4), hip.alloc(nq * k * 8)
                for r, p in enumerate(parts):
                    b = packed + r * S
                    p.search_device(xq, nq, k, n_probe, b, b + off_i, b + off_i + nq * k * 8, filter=filters[r])
                N.check(N.lib().vi_merge_partials_packed_device(0, nq, k, world, packed, Dm, Im))
                assert np.array_equal(hip.download(Im, (nq, k), np.int64), Ie), (w, k, n_probe)
                assert np.array_equal(bits(hip.download(Dm, (nq, k), np.float32)), bits(De)), (w, k, n_probe)
                # the coarse step split over the ranks by query, then the filtered list phase on every rank
                p_eff = min(n_probe, base.nlists)
                probes, order = hip.alloc(nq * p_eff * 4), hip.alloc(nq * p_eff * 4)
                per = nq // world
                for r, p in enumerate(parts):
                    assert p.probe_device(xq + r * per * base.dim * 4, per, n_probe, probes + r * per * p_eff * 4,
                                          order + r * per * p_eff * 4) == p_eff
                for r, p in enumerate(parts):
                    b = packed + r * S
                    p.search_probed_device(xq, nq, k, p_eff, probes, order, b, b + off_i, b + off_i + nq * k * 8, filter=filters[r])
                N.check(N.lib().vi_merge_partials_packed_device(0, nq, k, world, packed, Dm, Im))
                assert np.array_equal(hip.download(Im, (nq, k), np.int64), Ie), ("probed", w, k, n_probe)
                assert np.array_equal(bits(hip.download(Dm, (nq, k), np.float32)), bits(De)), ("probed", w, k, n_probe)
    finally:
        hip.close()


def test_errors(base, valu):
    with pytest.raises(vip.ViError) as e:
        base.gpu.filter_timestamps(11, 10)
    assert e.value.kind == "InvalidInput"
    other = vip.load(base.idx, base.sh, base.dim)
    with pytest.raises(vip.ViError) as e:
        other.search_sync(base.Q[:3], 5, 4, filter=base.filter(TENTH))
    assert e.value.kind == "InvalidInput"
    with pytest.raises(vip.ViError) as e:
        valu.gpu.search_sync(valu.Q[:3], 5, 4, filter=base.filter(TENTH))
    assert e.value.kind == "InvalidInput"
    D, I = other.search_sync(base.Q[:3], 5, 4, filter=None)   # NULL: the unfiltered entry
    assert np.array_equal(I, base.gpu.search_sync(base.Q[:3], 5, 4)[1])


def test_four_threads_share_one_handle_and_one_filter(base):
    flt = base.filter(TENTH)
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
    De, Ie, _ = base.expected(TENTH, 9, 10, 8)
    assert np.array_equal(want[0][1], Ie) and np.array_equal(bits(want[0][0]), bits(De))
