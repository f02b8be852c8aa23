"""GPU: radius (range) search — vi_indexer_range_search* — on the MFMA engine in every rank mode and on the generic engine.

The contract: the radius result of a query is the reference's candidate sequence (probed lists in shard visiting order,
probe rank, list position — ivf_index.rs:223-262) under the reference's stable sort by distance, cut at the first candidate
whose f32 distance exceeds radius2: take_while(d <= radius2) where a search has take(k).  The expected results come from
the untouched oracle, as in test_filtered_search_gpu.py: OracleIndex.search_batch with k = N is the whole stable-sorted
candidate sequence; with a window the ids outside it are dropped; the prefix with distance <= np.float32(radius2) is the
answer.  lims, ids and distance bits must match exactly."""
import threading

import numpy as np
import pytest

import vector_indexer_py as vip
from test_filtered_search_gpu import (EVERYTHING, NOTHING, ONLY_NOW, TENTH, Fixture, base, bits, bytes8, long_lists,  # noqa: F401
                                      queries, valu, wide)

pytestmark = pytest.mark.gpu

INF = float("inf")


def expected(fx, radius2, nq, n_probe, window=EVERYTHING):
    """(lims, D, I, candidates) of the first nq queries: the oracle's sorted candidates inside the window, while d <= radius2"""
    D, I, row = fx.full(n_probe)
    D, I, row = D[:nq], I[:nq], row[:nq]
    s = fx.stored[row]
    keep = (I >= 0) & (s >= np.uint64(window[0])) & (s <= np.uint64(window[1]))
    hit = keep & (D <= np.float32(radius2))
    lims = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.uint64)
    return lims, D[hit], I[hit], int(keep.sum())


def check(fx, radius2, nq, n_probe, window=EVERYTHING, index=None, flt=None, want=None):
    lims_e, De, Ie, ncand = want or expected(fx, radius2, nq, n_probe, window)
    gpu = index or fx.gpu
    if flt is None and window != EVERYTHING:
        flt = fx.filter(window)
    lims, D, I = gpu.range_search_sync(fx.Q[:nq], radius2, n_probe, filter=flt)
    assert lims.dtype == np.uint64 and lims.shape == (nq + 1,) and D.dtype == np.float32 and I.dtype == np.int64
    bad = np.nonzero(lims != lims_e)[0]
    assert bad.size == 0, f"radius2 {radius2!r} nq {nq} n_probe {n_probe}: lims differ from query {bad[0] - 1}: {lims[bad[0]]} expected {lims_e[bad[0]]}"
    assert np.array_equal(I, Ie), f"radius2 {radius2!r} nq {nq} n_probe {n_probe}: ids differ"
    assert np.array_equal(bits(D), bits(De)), f"radius2 {radius2!r} nq {nq} n_probe {n_probe}: distance bits differ"
    return int(lims_e[-1]), ncand


def kth_distances(fx, n_probe, kth):
    """distance of every query's kth candidate (1-based) in the oracle's sorted sequence; queries with fewer are left out"""
    D, I, _ = fx.full(n_probe)
    have = I[:, kth - 1] >= 0
    return D[have, kth - 1]


def median_radius(fx, n_probe, kth):
    d = np.sort(kth_distances(fx, n_probe, kth))
    assert d.size > 0
    return float(d[d.size // 2])   # (an actual distance: the boundary is hit exactly by that query)


def retarget(fx, Q):
    """the same index with other queries"""
    other = Fixture.__new__(Fixture)
    other.__dict__.update(fx.__dict__)
    other.Q, other._full = np.ascontiguousarray(Q, dtype=np.float32), {}
    return other


@pytest.fixture(scope="module")
def offset(tmp_path_factory):       # far from the origin: catastrophic cancellation in ||v||^2 - 2 q.v, margins admit nearly everything
    rng = np.random.default_rng(21)
    X = (rng.standard_normal((6000, 32)) + 100.0).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("offset"), X, 24, queries(rng, X, 300))


RADII = ["negative", "zero", "boundary", "below_boundary", "median10", "median100", "inf"]


@pytest.mark.parametrize("nq", [1, 33, 300])
@pytest.mark.parametrize("n_probe", [1, 8, 10_000])
@pytest.mark.parametrize("which", RADII)
def test_radii_and_batch_shapes(base, which, n_probe, nq):
    """n_probe 10 000 is clamped to the 24 lists and runs on the MFMA engine.  The boundary pair uses query 50 (the last
    query of the batch when it has fewer than 51)"""
    D, I, _ = base.full(n_probe)
    qb = min(50, nq - 1)
    edge = D[qb, 9]
    assert I[qb, 9] >= 0 and edge > 0
    r = {"negative": -1.0, "zero": 0.0, "boundary": float(edge), "below_boundary": float(np.nextafter(edge, np.float32(-1.0))),
         "median10": median_radius(base, n_probe, 10), "median100": median_radius(base, n_probe, 100), "inf": INF}[which]
    lims, De, Ie, ncand = want = expected(base, r, nq, n_probe)
    hits = int(lims[-1])
    own = int(lims[qb + 1] - lims[qb])
    if which == "negative":
        assert hits == 0
    elif which == "zero":
        assert hits > 0 and (De == 0.0).all()    # the stored-vector queries find themselves
    elif which == "boundary":
        assert own >= 10 and De[int(lims[qb]) + own - 1] == edge      # d == radius2 is inside
    elif which == "below_boundary":
        assert own == int((D[qb][I[qb] >= 0] < edge).sum()) < 10
    elif which in ("median10", "median100"):
        assert 0 < hits < ncand
    else:
        assert hits == ncand > 0
    check(base, r, nq, n_probe, want=want)
    st = base.gpu.last_stats()
    assert st["k"] == 0 and st["nq"] == nq and (st["rank_mode"] >= 1 or which == "negative")   # (a negative radius runs no engine)


def test_lists_longer_than_a_segment_and_more_hits_than_one_sort_chunk(long_lists):
    hits, ncand = check(long_lists, INF, 33, 2)
    assert hits == ncand == 33 * 6000      # a query owns 6000 hits: past one 2048-key chunk and past the pick queue
    for p in (1, 2):
        for kth in (10, 100):
            r = median_radius(long_lists, p, kth)
            hits, ncand = check(long_lists, r, 300, p)
            assert 0 < hits < ncand
    assert long_lists.gpu.last_stats()["rank_mode"] >= 1


@pytest.mark.parametrize("rank_i8", ["1", "0"])
def test_byte_lists(bytes8, rank_i8, monkeypatch):
    """integer distances with masses of exact ties: the order inside a query is decided by candidate order"""
    monkeypatch.setenv("VI_RANK_I8", rank_i8)
    D, _, _ = bytes8.full(8)
    assert (np.diff(D[:, :200], axis=1) == 0).any()      # the fixture does have ties
    for nq, p in [(300, 8), (33, 10_000), (1, 1)]:
        for r in (median_radius(bytes8, p, 10), median_radius(bytes8, p, 100), median_radius(bytes8, p, 100) + 0.5, 0.0, INF):
            hits, ncand = check(bytes8, r, nq, p)
            assert hits > 0 and (hits < ncand or r == INF)
        st = bytes8.gpu.last_stats()
        assert st["rank_mode"] == 3 and st["rank_int8"] == int(rank_i8), st


def test_byte_lists_one_fractional_query_value(bytes8):
    """one fractional value in the batch: the batch is ranked with bf16, its other queries keep their byte form"""
    Q = bytes8.Q.copy()
    Q[5, 3] += 0.5
    fx = retarget(bytes8, Q)
    for r in (median_radius(fx, 8, 10), median_radius(fx, 8, 100), INF):
        hits, ncand = check(fx, r, 300, 8)
        assert 0 < hits <= ncand
    st = fx.gpu.last_stats()
    assert st["rank_mode"] == 3 and st["rank_int8"] == 0, st


def test_wide_vectors(wide):
    for nq, p in [(300, 8), (33, 10_000), (1, 1)]:
        for r in (median_radius(wide, p, 10), median_radius(wide, p, 100), INF):
            hits, ncand = check(wide, r, nq, p)
            assert 0 < hits and (hits < ncand or r == INF)
    assert wide.gpu.last_stats()["rank_mode"] == 2


def test_generic_engine_for_a_dimension_the_mfma_engine_does_not_take(valu):
    for nq, p in [(300, 8), (33, 10_000), (1, 1)]:
        for r in (-1.0, 0.0, median_radius(valu, p, 10), median_radius(valu, p, 100), INF):
            hits, ncand = check(valu, r, nq, p)
            assert (hits == 0) == (r < 0) and (hits < ncand or r == INF)
    assert valu.gpu.last_stats()["rank_mode"] == 0


def test_far_from_the_origin(offset):
    for nq, p in [(300, 8), (33, 10_000), (1, 1)]:
        for r in (0.0, median_radius(offset, p, 10), median_radius(offset, p, 100), INF):
            hits, ncand = check(offset, r, nq, p)
            assert 0 < hits and (hits < ncand or r == INF)
    assert offset.gpu.last_stats()["rank_mode"] >= 1


def test_more_probes_than_the_mfma_select_holds(tmp_path_factory):
    """n_probe = 65 > 64 on an index of 130 lists: the generic engine"""
    rng = np.random.default_rng(22)
    X = rng.standard_normal((6000, 32)).astype(np.float32)
    fx = Fixture(tmp_path_factory.mktemp("many"), X, 130, queries(rng, X, 64))
    assert fx.nlists >= 65
    for r in (0.0, median_radius(fx, 65, 10), median_radius(fx, 65, 100), INF):
        hits, ncand = check(fx, r, 64, 65)
        assert 0 < hits and (hits < ncand or r == INF)
    assert fx.gpu.last_stats()["rank_mode"] == 0 and fx.gpu.last_stats()["n_probe_eff"] == 65
    for w in (TENTH, NOTHING):
        check(fx, median_radius(fx, 65, 100), 64, 65, window=w)


def test_engines_agree(base, monkeypatch):
    r = median_radius(base, 8, 100)
    mfma = base.gpu.range_search_sync(base.Q, r, 8)
    st = base.gpu.last_stats()
    assert st["rank_mode"] != 0 and st["filter_tile_blocks"] > 0
    monkeypatch.setenv("VI_FORCE_GENERIC", "1")      # (the knobs are read per search)
    generic = base.gpu.range_search_sync(base.Q, r, 8)
    assert base.gpu.last_stats()["rank_mode"] == 0
    assert mfma[0][-1] > 0
    assert np.array_equal(mfma[0], generic[0]) and np.array_equal(mfma[2], generic[2]) and np.array_equal(bits(mfma[1]), bits(generic[1]))


SWEEP = [{"VI_RANK_APPROX": "0"}, {"VI_RANK_APPROX": "1"}, {"VI_RANK_APPROX": "2"}, {"VI_FILTER_BF16": "0"}, {"VI_RANK_STREAM": "0"},
         {"VI_RANK_STREAM": "1"}, {"VI_FILTER_GQ": "32"}]


@pytest.mark.parametrize("centre", ["0", "1"])
@pytest.mark.parametrize("which", ["base", "offset"])
def test_rank_modes(which, centre, request, monkeypatch):
    """centring is a load-time choice: the index is loaded a second time under VI_CENTER"""
    fx = request.getfixturevalue(which)
    monkeypatch.setenv("VI_CENTER", centre)
    index = vip.load(fx.idx, fx.sh, fx.dim)
    r = median_radius(fx, 8, 10)
    want = expected(fx, r, 300, 8)
    assert 0 < int(want[0][-1]) < want[3]
    modes = set()
    for env in SWEEP:
        with pytest.MonkeyPatch.context() as mp:
            for a, b in env.items():
                mp.setenv(a, b)
            check(fx, r, 300, 8, index=index, want=want)
            st = index.last_stats()
            assert st["rank_mode"] >= 1, (env, st)
            modes.add((st["rank_mode"], st["group_queries"]))
    assert len(modes) >= 3, modes     # the sweep did reach different rank kernels and arithmetic


def test_pruning_happens(base, monkeypatch):
    monkeypatch.setenv("VI_FILTER_STATS", "1")
    base.gpu.enable_timing(True)
    try:
        check(base, median_radius(base, 8, 10), 300, 8)
        st = base.gpu.last_stats()
    finally:
        base.gpu.enable_timing(False)
    print("re-evaluated", st["filter_rechecked"], "of", st["scanned_vectors"], "probed vectors")
    assert 0 < st["filter_rechecked"] < st["scanned_vectors"], st


@pytest.mark.parametrize("which", ["base", "valu"])
def test_with_a_timestamp_window(which, request):
    fx = request.getfixturevalue(which)
    r = median_radius(fx, 8, 100)
    for nq, p in [(300, 8), (33, 10_000), (1, 1)]:
        plain = fx.gpu.range_search_sync(fx.Q[:nq], r, p)
        everything = fx.gpu.range_search_sync(fx.Q[:nq], r, p, filter=fx.filter(EVERYTHING))
        assert np.array_equal(plain[0], everything[0]) and np.array_equal(plain[2], everything[2])
        assert np.array_equal(bits(plain[1]), bits(everything[1]))
        for w in (EVERYTHING, NOTHING, TENTH, ONLY_NOW):
            hits, ncand = check(fx, r, nq, p, window=w)
            assert hits <= ncand and (w != NOTHING or ncand == 0)
    hits_tenth, _ = check(fx, r, 300, 8, window=TENTH)
    assert 0 < hits_tenth < int(expected(fx, r, 300, 8)[0][-1])      # the window does thin the result
    other = vip.load(fx.idx, fx.sh, fx.dim)
    with pytest.raises(vip.ViError) as e:
        other.range_search_sync(fx.Q[:3], r, 4, filter=fx.filter(TENTH))
    assert e.value.kind == "InvalidInput"


@pytest.mark.parametrize("k", [10, 100])
def test_the_first_k_of_everything_are_the_search_results(base, k):
    for p in (1, 8):
        lims, D, I = base.gpu.range_search_sync(base.Q, INF, p)
        Ds, Is = base.gpu.search_sync(base.Q, k, p)
        for q in range(300):
            n = min(k, int(lims[q + 1] - lims[q]))
            assert n > 0
            a = int(lims[q])
            assert np.array_equal(I[a:a + n], Is[q, :n]) and np.array_equal(bits(D[a:a + n]), bits(Ds[q, :n]))
            assert (Is[q, n:] == -1).all()


@pytest.mark.parametrize("placement", [0, 1])
def test_two_ranks_merge_by_distance_and_tie(base, placement):
    """each rank's radius result covers its resident part and carries the tie keys of vi_indexer_search_device (stripe
    correction included): the union merged on the host by (distance bits, tie) is the oracle's result"""
    from hiprt import Hip
    world, nq, p = 2, 300, 8
    parts = [vip.load(base.idx, base.sh, base.dim, rank=r, world_size=world, placement=placement) for r in range(world)]
    assert sum(x.num_vectors for x in parts) == base.n
    hip = Hip()
    try:
        xq = hip.upload(base.Q)
        for r in (median_radius(base, p, 10), median_radius(base, p, 100), INF):
            lims_e, De, Ie, _ = expected(base, r, nq, p)
            got = []
            for part in parts:
                res = part.range_search_device(xq, nq, r, p)
                lims = hip.download(res.lims_ptr, (nq + 1,), np.uint64)
                assert int(lims[-1]) == res.total
                got.append((lims, hip.download(res.D_ptr, (res.total,), np.float32), hip.download(res.I_ptr, (res.total,), np.int64),
                            hip.download(res.tie_ptr, (res.total,), np.uint64)))
                res.free()
            assert sum(int(g[0][-1]) for g in got) == int(lims_e[-1]) > 0
            assert all(int(g[0][-1]) > 0 for g in got)      # both ranks hold part of the answer
            for q in range(nq):
                Dq = np.concatenate([g[1][int(g[0][q]):int(g[0][q + 1])] for g in got])
                Iq = np.concatenate([g[2][int(g[0][q]):int(g[0][q + 1])] for g in got])
                Tq = np.concatenate([g[3][int(g[0][q]):int(g[0][q + 1])] for g in got])
                order = np.lexsort((Tq, bits(Dq)))      # distances are >= 0: their bit patterns order as they do
                a, b = int(lims_e[q]), int(lims_e[q + 1])
                assert np.array_equal(Iq[order], Ie[a:b]) and np.array_equal(bits(Dq[order]), bits(De[a:b])), (r, q)
    finally:
        hip.close()


def test_four_threads_share_one_handle(base):
    """every thread checks its own radius; a result object of one thread outlives the other threads' searches"""
    from hiprt import Hip
    radii = [median_radius(base, 8, 10), median_radius(base, 8, 100), 0.0, median_radius(base, 1, 100)]
    want = [expected(base, r, 64, 8) for r in radii]
    hip = Hip()
    errors = []
    try:
        xq = hip.upload(base.Q[:64])
        held = base.gpu.range_search_device(xq, 64, radii[1], 8)

        def worker(t):
            try:
                for rep in range(6):
                    check(base, radii[t], 64, 8, want=want[t])
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=worker, args=(t,)) for t in range(4)]
        [t.start() for t in threads]
        [t.join() for t in threads]
        assert not errors, errors
        lims_e, De, Ie, _ = want[1]
        assert held.total == int(lims_e[-1]) > 0
        assert np.array_equal(hip.download(held.lims_ptr, (65,), np.uint64), lims_e)
        assert np.array_equal(hip.download(held.I_ptr, (held.total,), np.int64), Ie)
        assert np.array_equal(bits(hip.download(held.D_ptr, (held.total,), np.float32)), bits(De))
        held.free()
    finally:
        hip.close()
