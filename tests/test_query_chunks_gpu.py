"""GPU: batches whose key rows do not fit the key scratch at once, so that the engines go through them in chunks.

Two constants make a batch of 65 873 queries a two-chunk batch whatever the index: a query's row of sort keys holds at
least 2 048 keys (kChunk, generic_search.hip; kMinRowLog, range_select.hip) and a chunk of queries at most 2^27 keys
(kMaxKeys / kMaxRangeKeys): 65 536 rows.  The second chunk starts at a query q0 > 0, and every per-query array is read
at an offset: probes, candidate offsets, allowed totals, counts, the outputs, the query rows themselves — in the
sort-everything engine's top-k and radius forms, its coarse step (2 048-key rows over the centroid table: 65 536 queries
at a time), and the MFMA engine's radius select, whose results of the first chunk must survive the growth of the result
buffers for the second.

The oracle runs 300 queries; the batch repeats them (Q[i] = fx.Q[i % 300]) and the expected result is the
300-query result repeated.  65 873 is no multiple of 300: a chunk offset that is off by anything shows.  Ids, distance
bits and lims are compared exactly."""
import numpy as np
import pytest

from test_filtered_search_gpu import EVERYTHING, TENTH, Fixture, base, bits, queries, valu, wide  # noqa: F401
from test_range_search_gpu import INF, check, expected, median_radius, retarget

pytestmark = pytest.mark.gpu

NQ = 65_873
ROWS, BUDGET = 2048, 1 << 27
assert NQ * ROWS > BUDGET and NQ % 300 != 0


def repeated(fx, nq=NQ):
    """the same index, its 300 queries repeated to nq"""
    return retarget(fx, np.tile(fx.Q[:300], (-(-nq // 300), 1))[:nq])


def repeat_rows(a, nq=NQ):
    return np.tile(a, (-(-nq // 300),) + (1,) * (a.ndim - 1))[:nq]


def repeat_ranges(want, nq=NQ):
    """(lims, D, I, candidates) of 300 queries -> of the nq queries that repeat them"""
    lims, D, I, ncand = want
    counts = repeat_rows(np.diff(lims.astype(np.int64)), nq)
    lims_t = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    total = int(lims_t[-1])      # whole rounds of the 300, then a prefix of them
    return lims_t, np.tile(D, -(-nq // 300))[:total], np.tile(I, -(-nq // 300))[:total], ncand


def joined(a, b):
    """the expected radius result of batch a followed by batch b"""
    return (np.concatenate([a[0], a[0][-1] + b[0][1:]]), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]]), a[3] + b[3])


@pytest.mark.parametrize("window", [EVERYTHING, TENTH], ids=["plain", "tenth"])
def test_generic_top_k_in_two_chunks(valu, window, monkeypatch):
    """k = 100, n_probe 8 on the sort-everything engine; the window adds the allowed totals read at q0"""
    monkeypatch.setenv("VI_FORCE_GENERIC", "1")
    De, Ie, cnt = valu.expected(window, 300, 100, 8)
    assert (cnt > 0).all()
    De, Ie = repeat_rows(De), repeat_rows(Ie)
    big = repeated(valu)
    Dg, Ig = valu.gpu.search_sync(big.Q, 100, 8, filter=None if window == EVERYTHING else valu.filter(window))
    st = valu.gpu.last_stats()
    assert st["rank_mode"] == 0 and st["nq"] == NQ
    bad = np.nonzero((Ig != Ie).any(axis=1) | (bits(Dg) != bits(De)).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} queries differ, first {bad[0]}: gpu {Ig[bad[0]][:8]} expected {Ie[bad[0]][:8]}"


@pytest.mark.parametrize("window", [EVERYTHING, TENTH], ids=["plain", "tenth"])
def test_generic_radius_in_two_chunks(valu, window):
    """D = 10: the radius search of this index runs on the sort-everything engine"""
    r = median_radius(valu, 8, 10)
    want = expected(valu, r, 300, 8, window)
    assert 0 < int(want[0][-1]) < want[3]
    check(repeated(valu), r, NQ, 8, window=window, want=repeat_ranges(want))
    assert valu.gpu.last_stats()["rank_mode"] == 0


@pytest.mark.parametrize("window", [EVERYTHING, TENTH], ids=["plain", "tenth"])
def test_mfma_radius_in_two_chunks(base, window):
    """the result stays on the device: its total is the last of lims, and what the first chunk placed is still there
    after the buffers grew for the second — the first entries of the arrays compared"""
    from hiprt import Hip
    r = median_radius(base, 8, 10)
    want = expected(base, r, 300, 8, window)
    assert 0 < int(want[0][-1]) < want[3]
    lims_e, De, Ie, _ = repeat_ranges(want)
    big = repeated(base)
    hip = Hip()
    try:
        xq = hip.upload(big.Q)
        res = base.gpu.range_search_device(xq, NQ, r, 8, filter=None if window == EVERYTHING else base.filter(window))
        st = base.gpu.last_stats()
        assert st["rank_mode"] >= 1 and st["nq"] == NQ
        lims = hip.download(res.lims_ptr, (NQ + 1,), np.uint64)
        assert int(lims[-1]) == res.total == int(lims_e[-1])
        bad = np.nonzero(lims != lims_e)[0]
        assert bad.size == 0, f"lims differ from query {bad[0] - 1}: {lims[bad[0]]} expected {lims_e[bad[0]]}"
        I, D = hip.download(res.I_ptr, (res.total,), np.int64), hip.download(res.D_ptr, (res.total,), np.float32)
        first = int(lims_e[1024])
        assert first > 0 and np.array_equal(I[:first], Ie[:first]) and np.array_equal(bits(D[:first]), bits(De[:first]))
        assert np.array_equal(I, Ie) and np.array_equal(bits(D), bits(De))
        res.free()
    finally:
        hip.close()


@pytest.fixture(scope="module")
def two_lists_far_from_the_origin(tmp_path_factory):
    """two lists of 3 000 vectors (47 blocks) around +300 and -300 in every dimension.  Far from the origin the rank
    margins (they scale with |q|^2 + 2 max |v|^2) are wider than a cluster, so a query near the data re-evaluates its
    whole cluster and needs a row longer than 2 048 keys; the mean of the stored vectors is the origin, so images taken
    about the mean would be the same images.  (test_range_search_gpu.py's `offset` data — one cloud around +100 — in two
    lists is ranked about its mean and re-evaluates 390 vectors per query: measured, 117 140 for the 300 queries)"""
    rng = np.random.default_rng(21)
    side = rng.permutation(np.repeat([300.0, -300.0], 3000))
    X = (rng.standard_normal((6000, 32)) + side[:, None]).astype(np.float32)
    fx = Fixture(tmp_path_factory.mktemp("offset2"), X, 2, queries(rng, X, 300))
    assert sorted(int(fx.orc.list_len(c)) for c in range(2)) == [3000, 3000]
    return fx


def rechecked(fx, Q, r, monkeypatch):
    """vectors the radius select evaluated exactly for this batch: the sum of the rows' fill before the radius cut"""
    with monkeypatch.context() as mp:
        mp.setenv("VI_FILTER_STATS", "1")
        fx.gpu.enable_timing(True)
        try:
            fx.gpu.range_search_sync(Q, r, 2)
            st = fx.gpu.last_stats()
        finally:
            fx.gpu.enable_timing(False)
    assert st["rank_mode"] >= 1
    return st["filter_rechecked"]


def test_two_row_lengths_in_one_batch(two_lists_far_from_the_origin, monkeypatch):
    """40 000 queries that no record comes near (a bound of 0: rows of 2 048 keys) and 300 near ones (rows of more than
    2 048 keys), in both orders.  Far then near: 40 000 x 2 048 keys fit the budget, the first long row (40 001 x 4 096
    or more) does not — the chunk breaks where the row length would grow.  Near then far: every row of the first chunk is
    long, the far queries behind the break get short ones"""
    fx = two_lists_far_from_the_origin
    near, far300 = fx.Q[:300], fx.Q[:300] + np.float32(1000.0)
    far = repeat_rows(far300, 40_000)
    r = median_radius(fx, 2, 10)
    n_far, n_near = rechecked(fx, far, r, monkeypatch), rechecked(fx, near, r, monkeypatch)
    print("exact evaluations: far", n_far, "near", n_near, "of", 300 * fx.n)
    assert n_far == 0
    assert n_near > ROWS * 300
    assert 40_001 * 2 * ROWS > BUDGET >= 40_000 * ROWS
    want_near = expected(fx, r, 300, 2)
    want_far = repeat_ranges(expected(retarget(fx, far300), r, 300, 2), 40_000)
    assert 0 < int(want_near[0][-1]) < want_near[3] and int(want_far[0][-1]) == 0      # (the oracle: nothing within the radius of a far query)
    check(retarget(fx, np.concatenate([far, near])), r, 40_300, 2, want=joined(want_far, want_near))
    check(retarget(fx, np.concatenate([near, far])), r, 40_300, 2, want=joined(want_near, want_far))
    assert fx.gpu.last_stats()["rank_mode"] >= 1


def test_stored_vectors_of_more_hits_than_one_gather_step(wide):
    """range_result_copy gathers the stored vectors of (1 << 28) / D hits at a time: 1 342 177 at D = 200"""
    nq = 240
    lims_e, De, Ie, _ = expected(wide, INF, nq, 10_000)
    assert int(lims_e[-1]) == nq * wide.n > (1 << 28) // wide.dim
    lims, D, I, V = wide.gpu.range_search_sync(wide.Q[:nq], INF, 10_000, include_vectors=True)
    assert np.array_equal(lims, lims_e) and np.array_equal(I, Ie) and np.array_equal(bits(D), bits(De))
    assert V.shape == (I.size, wide.dim)
    rows = (I - 1_000_003) // 7
    for a in range(0, I.size, 1 << 17):      # (in pieces: X[rows] whole is another gigabyte)
        assert np.array_equal(V[a:a + (1 << 17)], wide.X[rows[a:a + (1 << 17)]]), a
