"""GPU: radius search by stored record — vi_indexer_range_search_by_ids (host and device form) and vi_indexer_radius_graph.

The contract: the row of a stored record r is the reference's candidate sequence for r's stored f32 bits with the
candidates a filter does not admit deleted, then — exclude_self — the ONE candidate that is r itself (its slot), then the
reference's stable sort and take_while(d <= radius2).  The expected rows come from the untouched oracle: Fixture.full(p)
is the whole stably sorted candidate sequence of each chosen stored vector; the expected row is its entries with I >= 0
that the filter admits, less own_entries when excluding, with D <= np.float32(radius2); the expected result is those rows
concatenated.  lims, I, the bits of D and found must match exactly.  The radii are taken from the oracle's sequences."""
import ctypes as C
import threading

import numpy as np
import pytest

import vector_indexer_py as vip
from test_id_filter_gpu import HALF, U64_MAX, bits, u64
from test_similar_search_gpu import NROWS, ORACLE_CHUNK, Fixture, own_entries
from vector_indexer_py import _native as N

pytestmark = pytest.mark.gpu

PS = [1, 8, 24, 10_000]
INF = float("inf")


# ---- fixtures of this module (the classes and rules are shared, the indexes are its own) ----
@pytest.fixture(scope="module")
def base(tmp_path_factory):         # D = 32: the MFMA engine; 250-vector lists end in a ragged block
    rng = np.random.default_rng(1)
    return Fixture(tmp_path_factory.mktemp("rbase"), rng.standard_normal((6000, 32)).astype(np.float32), 24)


@pytest.fixture(scope="module")
def valu(tmp_path_factory):         # D % 4 != 0: the generic engine's radius form
    rng = np.random.default_rng(3)
    return Fixture(tmp_path_factory.mktemp("rvalu"), rng.standard_normal((6000, 10)).astype(np.float32), 24)


@pytest.fixture(scope="module")
def bytes8(tmp_path_factory):       # 8-bit descriptors: the int8 rank kernel
    rng = np.random.default_rng(5)
    centers = rng.integers(40, 216, size=(24, 128))
    X = np.clip(centers[rng.integers(0, 24, 6000)] + rng.integers(-40, 41, size=(6000, 128)), 0, 254).astype(np.float32)
    return Fixture(tmp_path_factory.mktemp("rbytes"), X, 24)


@pytest.fixture(scope="module")
def hier(tmp_path_factory):         # more than 100 lists: records whose own list is not the first probed; n_probe 100 > 64
    rng = np.random.default_rng(1)
    return Fixture(tmp_path_factory.mktemp("rhier"), rng.standard_normal((3000, 32)).astype(np.float32), 104)


NCOPIES = 70


@pytest.fixture(scope="module")
def copies(tmp_path_factory):       # one vector stored 70 times under distinct ids, among 3000 random ones
    rng = np.random.default_rng(41)
    X = rng.standard_normal((3000 + NCOPIES, 32)).astype(np.float32)
    fx_rows = rng.permutation(3000 + NCOPIES)[:NCOPIES]
    X[fx_rows] = X[fx_rows[0]]
    fx = Fixture(tmp_path_factory.mktemp("rcopies"), X, 8)
    fx.copies = np.sort(fx_rows)
    return fx


@pytest.fixture(scope="module")
def dups(tmp_path_factory):
    rng = np.random.default_rng(23)
    n = 1500
    X = rng.standard_normal((n, 32)).astype(np.float32)
    ext = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    ext[900] = ext[100]                   # one id, two vectors
    X[1000] = X[200]                      # one vector, two ids
    ext[1100], X[1100] = ext[300], X[300]   # both shared
    return Fixture(tmp_path_factory.mktemp("rdups"), X, 8, ext=ext)


@pytest.fixture(scope="module")
def hip():
    from hiprt import Hip
    h = Hip()
    yield h
    h.close()


# ---- expected rows ----
def keep_mask(D, I, own_ids, radius2, exclude, admit=None):
    keep = I >= 0
    if admit is not None:
        keep = keep & admit(I)
    if exclude:
        keep = keep & ~own_entries(D, I, own_ids)
    return keep & (D <= np.float32(radius2))


def csr(D, I, keep):
    """rows of (D, I) restricted to keep, concatenated -> (lims, D, I)"""
    lims = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint64)
    return lims, D[keep], I[keep]


_SHARED = {}    # made once from the oracle's sequences, shared by the tests, never changed


def masks(fx, n_probe):
    """of fx.full(n_probe): the entries that hold a candidate, and each row's own entry"""
    key = (id(fx), "masks", min(n_probe, fx.nlists))
    if key not in _SHARED:
        D, I = fx.full(n_probe)
        valid, own = I >= 0, own_entries(D, I, fx.ext[fx.rows])
        valid.setflags(write=False), own.setflags(write=False)
        _SHARED[key] = (valid, own)
    return _SHARED[key]


def expected(fx, n_probe, radius2, exclude, admit=None):
    D, I = fx.full(n_probe)
    valid, own = masks(fx, n_probe)
    keep = valid & (D <= np.float32(radius2))
    if admit is not None:
        keep &= admit(I)
    if exclude:
        keep &= ~own
    return csr(D, I, keep)


def radii_of(fx, n_probe=8):
    """from the oracle's sequences at n_probe: the median over rows of the 1st, 10th and 100th non-own distance, and for
    one row the exact bits of its 5th non-own distance and the f32 just below"""
    key = (id(fx), "radii", n_probe)
    if key in _SHARED:
        return _SHARED[key]
    D, I = fx.full(n_probe)
    valid, own = masks(fx, n_probe)
    keep = valid & ~own
    rank = np.cumsum(keep, axis=1) - 1

    def nth(j):     # per row its (j + 1)-th non-own distance, inf where the row has fewer
        hit = keep & (rank == j)
        return np.where(hit.any(axis=1), np.where(hit, D, np.float32(0)).max(axis=1), np.float32(np.inf)).astype(np.float32)

    out = {"r1": np.float32(np.median(nth(0))), "r10": np.float32(np.median(nth(9))), "r100": np.float32(np.median(nth(99)))}
    fourth, fifth, sixth = nth(3), nth(4), nth(5)
    row = int(np.argmax(np.isfinite(sixth) & (fourth < fifth) & (fifth < sixth)))     # a row whose 5th stands alone
    assert fourth[row] < fifth[row] < sixth[row]
    out["fifth"], out["below_fifth"] = fifth[row], np.nextafter(fifth[row], np.float32(-np.inf))
    _SHARED[key] = (out, row)
    return out, row


def assert_csr(got, want, what):
    (lg, Dg, Ig), (le, De, Ie) = got, want
    assert lg.dtype == np.uint64 and np.array_equal(lg, le), (what, "lims", lg[:8], le[:8], int(lg[-1]), int(le[-1]))
    assert np.array_equal(Ig, Ie), (what, "ids")
    assert np.array_equal(bits(Dg), bits(De)), (what, "distance bits")


def raw_by_ids(index, ids, radius2, n_probe, exclude, flt=None):
    """the host entry itself -> (status, handle, found)"""
    ids = u64(ids)
    found, h = np.full(max(ids.size, 1), 7, dtype=np.uint32), C.c_void_p()
    st = N.lib().vi_indexer_range_search_by_ids(index._h, flt._h if flt is not None else None, N.ptr(ids) if ids.size else None,
                                                ids.size, float(radius2), n_probe, 1 if exclude else 0, N.ptr(found), C.byref(h))
    return st, h, found[: ids.size] if ids.size else found


def device_arrays(hip, res):
    """a RangeResult's four device arrays on the host: (lims, D, I, tie)"""
    n = max(res.total, 1)
    pl, pd, pi, pt = hip.alloc((res.nq + 1) * 8), hip.alloc(n * 4), hip.alloc(n * 8), hip.alloc(n * 8)
    res.copy_device(pl, pd, pi, pt)
    return (hip.download(pl, (res.nq + 1,), np.uint64), hip.download(pd, (res.total,), np.float32),
            hip.download(pi, (res.total,), np.int64), hip.download(pt, (res.total,), np.uint64))


def device_by_ids(hip, index, ids, radius2, n_probe, exclude, flt=None):
    ids = u64(ids)
    F = hip.upload(np.full(max(ids.size, 1), 7, dtype=np.uint32))
    res = index.range_search_by_ids_device(hip.upload(ids), ids.size, radius2, n_probe, exclude_self=exclude, found_ptr=F, filter=flt)
    try:
        return device_arrays(hip, res) + (hip.download(F, (ids.size,), np.uint32),)
    finally:
        res.free()


# ---- 1. by id against the oracle, the three engines ----
@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("name", ["base", "valu", "bytes8"])
def test_by_id_against_the_oracle(name, exclude, request, hip):
    fx = request.getfixturevalue(name)
    ids = fx.ext[fx.rows]
    radii, row5 = radii_of(fx)
    seen = {"empty": False, "single": False, "long": False}
    for p in PS:
        for rname, r in [("zero", 0.0), ("negative", -1.0), ("inf", INF)] + list(radii.items()):
            what = f"{name} n_probe {p} radius {rname} exclude {exclude}"
            want = expected(fx, p, r, exclude)
            with_v = rname == "r10"      # (the vectors of every probed record at +inf would be gigabytes on bytes8)
            got = fx.gpu.range_search_by_ids(ids, r, p, exclude_self=exclude, include_vectors=with_v)
            assert_csr(got[:3], want, what)
            assert (got[-1] == 1).all(), what
            if with_v:
                assert np.array_equal(got[3], fx.X[fx.rows_of(got[2])]), what
            st = fx.gpu.last_stats()
            assert st["k"] == 0 and (st["nq"] == NROWS or r < 0), (what, st)      # as after a radius search
            ld, Dd, Id, Td, Fd = device_by_ids(hip, fx.gpu, ids, r, p, exclude)
            assert_csr((ld, Dd, Id), want, what + " (device)")
            assert (Fd == 1).all() and Td.size == Id.size, what
            # what each case relies on
            lens = np.diff(want[0].astype(np.int64))
            plain = np.diff(expected(fx, p, r, False)[0].astype(np.int64)) if exclude else lens
            seen["empty"] |= bool((lens == 0).any()) and r >= 0
            seen["single"] |= bool((plain == 1).any())
            seen["long"] |= bool((lens > 64).any())
            if rname == "negative":
                assert want[0][-1] == 0
            if rname == "r10" and p == 8 and exclude:
                assert 1 <= lens.mean() <= 100, lens.mean()
            if rname in ("fifth", "below_fifth") and p == 8 and exclude:
                assert lens[row5] == (5 if rname == "fifth" else 4), (what, lens[row5])    # d == radius2 is inside
    # (without exclusion every row holds at least its own record: an empty row needs the exclusion)
    assert seen["single"] and seen["long"] and (seen["empty"] or not exclude), seen


# ---- 2. composition: get + range search of the stored bits ----
def test_device_entry_is_get_plus_range_search_bit_for_bit(base, hip):
    fx, ids = base, base.ext[base.rows]
    radii, _ = radii_of(fx)
    dids, dX = hip.upload(ids), hip.alloc(NROWS * fx.dim * 4)
    fx.gpu.get_device(dids, NROWS, values_ptr=dX)
    for p in (8, 10_000):
        for r in (0.0, float(radii["r10"]), float(radii["r100"]), INF):
            plain = fx.gpu.range_search_device(dX, NROWS, r, p)
            lp, Dp, Ip, Tp = device_arrays(hip, plain)
            plain.free()
            ld, Dd, Id, Td, _ = device_by_ids(hip, fx.gpu, ids, r, p, False)
            assert np.array_equal(ld, lp) and np.array_equal(bits(Dd), bits(Dp)) and np.array_equal(Id, Ip) and np.array_equal(Td, Tp)
            # with exclusion: that less the one entry per row carrying the row's id (ids and vectors are unique here)
            rowof = np.repeat(np.arange(NROWS), np.diff(lp.astype(np.int64)))
            keep = Ip != ids.astype(np.int64)[rowof]
            assert (~keep).sum() == NROWS
            le = np.concatenate([[0], np.cumsum(np.bincount(rowof[keep], minlength=NROWS))]).astype(np.uint64)
            lx, Dx, Ix, Tx, _ = device_by_ids(hip, fx.gpu, ids, r, p, True)
            assert np.array_equal(lx, le) and np.array_equal(bits(Dx), bits(Dp[keep])) and np.array_equal(Ix, Ip[keep])
            assert np.array_equal(Tx, Tp[keep])


# ---- 3. the hierarchy: own list not probed; n_probe 100 on the generic engine ----
def test_a_record_whose_own_list_is_not_probed_keeps_its_plain_row(hier):
    fx, ids = hier, hier.ext[hier.rows]
    assert fx.unprobed.size >= 5 and np.isin(fx.unprobed[:5], fx.rows).all()
    D, I = fx.full(1)
    probed = own_entries(D, I, ids).any(axis=1)
    assert (~probed).any() and probed.any(), "no chosen record has its own list unprobed at n_probe 1"
    radii, _ = radii_of(fx, 1)
    for r in (float(radii["r10"]), INF):
        want_x, want_p = expected(fx, 1, r, True), expected(fx, 1, r, False)
        lx, lp = np.diff(want_x[0].astype(np.int64)), np.diff(want_p[0].astype(np.int64))
        assert (lx[~probed] == lp[~probed]).all() and (lx[probed] == lp[probed] - 1).all()    # nothing is there to delete
        got = fx.gpu.range_search_by_ids(ids, r, 1)
        assert_csr(got[:3], want_x, f"hier n_probe 1 radius {r}")
        rows = np.nonzero(~probed)[0]
        ls, Ds, Is = fx.gpu.range_search_sync(fx.X[fx.rows[rows]], r, 1)
        for j, q in enumerate(rows):
            a, b, c, d = int(got[0][q]), int(got[0][q + 1]), int(ls[j]), int(ls[j + 1])
            assert np.array_equal(got[2][a:b], Is[c:d]) and np.array_equal(bits(got[1][a:b]), bits(Ds[c:d]))


def test_n_probe_100_runs_the_generic_engine_with_the_oracles_bits(hier, hip):
    fx, ids = hier, hier.ext[hier.rows]
    radii, _ = radii_of(fx, 100)
    for exclude in (True, False):
        for r in (0.0, float(radii["r10"]), float(radii["r100"]), INF):
            want = expected(fx, 100, r, exclude)
            got = fx.gpu.range_search_by_ids(ids, r, 100, exclude_self=exclude)
            assert_csr(got[:3], want, f"hier n_probe 100 radius {r} exclude {exclude}")
            st = fx.gpu.last_stats()
            assert st["n_probe_eff"] == 100 and st["rank_mode"] == 0, st
            assert_csr(device_by_ids(hip, fx.gpu, ids, r, 100, exclude)[:3], want, "device")


# ---- 4. copies and duplicates: slot, not id; slot, not bits ----
def test_seventy_copies_at_radius_zero(copies, hip):
    fx = copies
    ids = fx.ext[fx.copies]
    assert ids.size == NCOPIES
    D, I = fx.sequences(fx.X[fx.copies], 1)
    zero = (I >= 0) & (bits(D) == 0)
    assert (zero.sum(axis=1) == NCOPIES).all(), "the oracle does not hold all 70 copies in one list"
    assert (zero[:, :NCOPIES]).all() and np.array_equal(np.sort(I[0, :NCOPIES]), np.sort(ids.astype(np.int64)))
    own_pos = np.array([int(np.nonzero(I[q, :NCOPIES] == int(ids[q]))[0][0]) for q in range(NCOPIES)])
    assert np.array_equal(np.sort(own_pos), np.arange(NCOPIES)) and (own_pos >= 64).any()     # across the 64-entry ballot step
    order = I[0, :NCOPIES]
    for p in (1, 8):
        lims, Dg, Ig, found = fx.gpu.range_search_by_ids(ids, 0.0, p)
        assert (found == 1).all() and np.array_equal(lims, np.arange(NCOPIES + 1, dtype=np.uint64) * np.uint64(NCOPIES - 1))
        assert (bits(Dg) == 0).all()
        for q in range(NCOPIES):
            assert np.array_equal(Ig[q * 69:(q + 1) * 69], order[order != int(ids[q])]), q     # the 69 others, in list order
        lims, Dg, Ig, found = fx.gpu.range_search_by_ids(ids, 0.0, p, exclude_self=False)
        assert np.array_equal(Ig, np.tile(order, NCOPIES)) and (bits(Dg) == 0).all()
        ld, Dd, Id, Td, Fd = device_by_ids(hip, fx.gpu, ids, 0.0, p, True)
        assert np.array_equal(Id, np.concatenate([order[order != int(e)] for e in ids])) and (Fd == 1).all()
    # a record that is no copy has an empty row at radius 0 with exclusion, itself alone without
    other = fx.ext[np.setdiff1d(np.arange(fx.n), fx.copies)[:5]]
    lims, _, Ig, _ = fx.gpu.range_search_by_ids(other, 0.0, 8)
    assert lims[-1] == 0
    lims, _, Ig, _ = fx.gpu.range_search_by_ids(other, 0.0, 8, exclude_self=False)
    assert np.array_equal(Ig, other.astype(np.int64))


def test_duplicate_ids_and_copied_vectors_at_a_small_radius(dups):
    fx = dups
    shared, a, b, both = fx.ext[100], fx.ext[200], fx.ext[1000], fx.ext[300]
    cnt, Xg, _, where = fx.gpu.get([shared])
    assert cnt[0] == 2
    Do, Io = fx.sequences(Xg, 10_000)
    nonzero = Do[0][(Io[0] >= 0) & (bits(Do[0]) != 0)]
    r = float(nonzero[9])                       # small and positive: the tenth other record of the shared id's row
    # a duplicated id names the first record in list order — the one get() reports — and found is the count
    want = csr(Do, Io, keep_mask(Do, Io, u64([shared]), r, True))
    lims, D, I, found = fx.gpu.range_search_by_ids([shared], r, 10_000)
    assert found[0] == 2
    assert_csr((lims, D, I), want, "shared id")
    assert int(shared) not in I.tolist() or bits(D[I == int(shared)])[0] != 0     # the other carrier is another vector
    lims, D, I, found = fx.gpu.range_search_by_ids([shared], INF, 10_000)
    assert lims[-1] == fx.n - 1 and (I == int(shared)).sum() == 1                 # slot, not id: the other carrier stays
    # a copied vector: the twin stays, at distance bits 0, first (slot, not bits)
    for me, twin in ((a, b), (b, a)):
        lims, D, I, found = fx.gpu.range_search_by_ids([me], 0.0, 10_000)
        assert found[0] == 1 and I.tolist() == [int(twin)] and bits(D)[0] == 0
    # id and vector shared: one of the pair goes, the other stays at distance bits 0
    lims, D, I, found = fx.gpu.range_search_by_ids([both], 0.0, 10_000)
    assert found[0] == 2 and I.tolist() == [int(both)] and bits(D)[0] == 0
    lims, D, I, found = fx.gpu.range_search_by_ids([both], 0.0, 10_000, exclude_self=False)
    assert I.tolist() == [int(both)] * 2 and (bits(D) == 0).all()


# ---- 5. absent and repeated ids ----
def test_absent_and_repeated_ids(base, hip, monkeypatch):
    fx = base
    radii, _ = radii_of(fx)
    r = float(radii["r10"])
    present = fx.ext[fx.rows[:20]]
    absent = u64([U64_MAX, U64_MAX - 1, (1 << 50) + 12345, 5, 6])
    assert not np.isin(absent, fx.ext).any()
    # absent at the first row, in the middle, as a whole chunk of 4 (rows 12..15 at VI_GRAPH_CHUNK 4) and at the last row
    ids = np.concatenate([absent[:1], present[:6], absent[1:2], np.full(4, present[3], dtype=np.uint64), np.tile(absent[2:3], 4),
                          present[6:], absent[3:4]])
    assert np.isin(ids[12:16], absent).all()
    is_absent = np.isin(ids, absent)
    pos = {int(e): i for i, e in enumerate(fx.ext[fx.rows])}
    for chunk in ("4", None):
        if chunk is None:
            monkeypatch.delenv("VI_GRAPH_CHUNK", raising=False)
        else:
            monkeypatch.setenv("VI_GRAPH_CHUNK", chunk)
        for exclude in (True, False):
            le, De, Ie = expected(fx, 8, r, exclude)
            lims, D, I, V, found = fx.gpu.range_search_by_ids(ids, r, 8, exclude_self=exclude, include_vectors=True)
            assert (found == np.where(is_absent, 0, 1)).all()
            lens = np.diff(lims.astype(np.int64))
            assert (lens[is_absent] == 0).all()
            for i, e in enumerate(ids):
                if not is_absent[i]:
                    q = pos[int(e)]
                    a, b, c, d = int(lims[i]), int(lims[i + 1]), int(le[q]), int(le[q + 1])
                    assert np.array_equal(I[a:b], Ie[c:d]) and np.array_equal(bits(D[a:b]), bits(De[c:d])), (chunk, exclude, i)
            assert np.array_equal(V, fx.X[fx.rows_of(I)])
            ld, Dd, Id, Td, Fd = device_by_ids(hip, fx.gpu, ids, r, 8, exclude)
            assert np.array_equal(ld, lims) and np.array_equal(Id, I) and np.array_equal(bits(Dd), bits(D)) and np.array_equal(Fd, found)
            lims, D, I, found = fx.gpu.range_search_by_ids(absent, INF, 8, exclude_self=exclude)     # only absent ids: VI_OK
            assert np.array_equal(lims, np.zeros(absent.size + 1, dtype=np.uint64)) and (found == 0).all() and I.size == 0
    lims, D, I, found = fx.gpu.range_search_by_ids(np.zeros(0, dtype=np.uint64), r, 8)
    assert np.array_equal(lims, np.zeros(1, dtype=np.uint64)) and D.size == 0 and found.size == 0
    le, De, Ie = fx.gpu.range_search_sync(np.zeros((0, fx.dim), dtype=np.float32), r, 8)
    assert np.array_equal(lims, le)


def test_timing_report_counts_the_drop_kernels_bytes(base, monkeypatch):
    """VI_SIMILAR_TIMING: drop_bytes is what range_find_kernel and range_move_kernel read and write — 68 bytes per row
    (its bounds in both results, its slot, count, position and length), the 8-byte slot of every searched entry where the
    row's own is looked for, and 28 bytes in and 28 out per entry moved; the three spans are measured.  The searched
    entries are the result of the non-excluding call (every id is present).  Without the variable the spans are 0; the
    bytes are counted all the same."""
    fx, n = base, 30
    ids = fx.ext[fx.rows[:n]]
    r = float(radii_of(fx)[0]["r10"])
    monkeypatch.setenv("VI_GRAPH_CHUNK", "4")
    monkeypatch.setenv("VI_SIMILAR_TIMING", "1")
    total, tm = {}, {}
    for exclude in (True, False):
        lims, _, _, found = fx.gpu.range_search_by_ids(ids, r, 8, exclude_self=exclude)
        total[exclude], tm[exclude] = int(lims[-1]), fx.gpu.similar_times()
        print("similar_times", exclude, total[exclude], tm[exclude])
        assert (found == 1).all() and total[exclude] == int(expected(fx, 8, r, exclude)[0][n])
        assert tm[exclude]["chunk_rows"] == 4, tm
        assert tm[exclude]["ms_resolve"] > 0 and tm[exclude]["ms_search"] > 0 and tm[exclude]["ms_drop"] > 0, tm
    assert tm[True]["drop_bytes"] == n * 68 + total[False] * 8 + total[True] * 56, (tm, total)
    assert tm[False]["drop_bytes"] == n * 68 + total[False] * 56, (tm, total)
    monkeypatch.delenv("VI_SIMILAR_TIMING")
    fx.gpu.range_search_by_ids(ids, r, 8)
    assert fx.gpu.similar_times() == {"ms_resolve": 0.0, "ms_search": 0.0, "ms_drop": 0.0, "drop_bytes": tm[True]["drop_bytes"],
                                      "chunk_rows": 4}


# ---- 6. with a filter ----
def test_with_a_filter(base):
    fx, ids = base, base.ext[base.rows]
    radii, _ = radii_of(fx)
    deny = np.concatenate([ids[:40], fx.ext[np.setdiff1d(np.arange(fx.n), fx.rows)[:500]]])
    flt = fx.gpu.filter_timestamps(*HALF) & fx.gpu.filter_ids(deny, exclude=True)

    def admit(I):
        rows = fx.rows_of(I)
        s = fx.ts[rows]
        return (s >= np.uint64(HALF[0])) & (s <= np.uint64(HALF[1])) & ~np.isin(fx.ext[rows], deny)

    for exclude in (True, False):
        for p, r in [(8, float(radii["r10"])), (8, float(radii["r100"])), (24, INF), (10_000, float(radii["r100"]))]:
            got = fx.gpu.range_search_by_ids(ids, r, p, exclude_self=exclude, filter=flt)
            assert (got[-1] == 1).all()          # a row exists whether or not the filter admits its record
            assert_csr(got[:3], expected(fx, p, r, exclude, admit), f"filtered n_probe {p} radius {r} exclude {exclude}")
    # the rows of denied records: their own hit is already gone, exclusion removes nothing more
    lx = np.diff(expected(fx, 8, INF, True, admit)[0].astype(np.int64))
    lp = np.diff(expected(fx, 8, INF, False, admit)[0].astype(np.int64))
    assert (lx[:40] == lp[:40]).all() and (lx[40:] < lp[40:]).any() and (lx[40:] >= lp[40:] - 1).all()


# ---- 7. the radius graph ----
@pytest.fixture(scope="module")
def graph_expected(base):
    """rows of the whole list order of `base` at n_probe 8 and the 10th-neighbour radius, from the oracle, by the ids
    export() reports"""
    radii, _ = radii_of(base)
    r = float(radii["r10"])
    ext_e, X_e, _, _ = base.gpu.export()
    assert np.array_equal(np.sort(ext_e), np.sort(base.ext))
    out = {True: [], False: []}
    for at in range(0, base.n, ORACLE_CHUNK):
        D, I = base.sequences(X_e[at:at + ORACLE_CHUNK], 8)
        for exclude in (True, False):
            keep = keep_mask(D, I, ext_e[at:at + ORACLE_CHUNK], r, exclude)
            out[exclude].append((keep.sum(axis=1), D[keep], I[keep]))
    return {e: tuple(np.concatenate([c[j] for c in out[e]]) for j in range(3)) for e in out}, ext_e, r


def graph_slice(want, first, count):
    lens, D, I = want
    off = np.concatenate([[0], np.cumsum(lens)])
    a, b = int(off[first]), int(off[first + count])
    return (off[first:first + count + 1] - off[first]).astype(np.uint64), D[a:b], I[a:b]


@pytest.mark.parametrize("chunk", ["1", "64", "1000", None])
def test_radius_graph_of_the_whole_index_and_a_sub_range(base, graph_expected, chunk, monkeypatch, hip):
    want, ext_e, r = graph_expected
    if chunk is None:
        monkeypatch.delenv("VI_GRAPH_CHUNK", raising=False)
    else:
        monkeypatch.setenv("VI_GRAPH_CHUNK", chunk)
    for exclude in (True, False):
        # (one row per chunk over all 6000 rows is 6000 searches: the sub-range covers chunk 1)
        if chunk != "1":
            res = base.gpu.radius_graph(r, 8, exclude_self=exclude)
            assert base.gpu.similar_times()["chunk_rows"] == int(chunk or 65536)     # the knob reached the call
            assert res.nq == base.n
            assert_csr(res.copy(), graph_slice(want[exclude], 0, base.n), f"graph chunk {chunk} exclude {exclude}")
            if exclude:
                rowof = np.repeat(np.arange(base.n), want[True][0])
                assert (res.copy()[2] != ext_e.astype(np.int64)[rowof]).all()     # (unique ids: no row holds its own record)
            res.free()
        # a chunk border inside a list, `first` inside a block
        first, count = (70, 1000) if chunk != "1" else (70, 130)
        res = base.gpu.radius_graph(r, 8, first=first, count=count, exclude_self=exclude)
        sub = graph_slice(want[exclude], first, count)
        assert_csr(res.copy(), sub, f"sub-range chunk {chunk} exclude {exclude}")
        # the device arrays, tie keys included, are those of the by-id device entry for the same records
        lg, Dg, Ig, Tg = device_arrays(hip, res)
        res.free()
        lb, Db, Ib, Tb, _ = device_by_ids(hip, base.gpu, ext_e[first:first + count], r, 8, exclude)
        assert np.array_equal(lg, lb) and np.array_equal(Ig, Ib) and np.array_equal(bits(Dg), bits(Db)) and np.array_equal(Tg, Tb)
    tail = base.gpu.radius_graph(r, 8, first=5990)
    assert tail.nq == 10
    assert_csr(tail.copy(), graph_slice(want[True], 5990, 10), "tail")
    tail.free()


def test_radius_graph_range_past_the_end_is_an_error_and_an_empty_range_is_empty(base):
    L = N.lib()
    for first, count in ((0, base.n + 1), (base.n, 1), (5000, 1001), (U64_MAX, 2)):
        h = C.c_void_p()
        assert L.vi_indexer_radius_graph(base.gpu._h, None, first, count, 1.0, 8, 1, C.byref(h)) == N.VI_ERR_INVALID_INPUT
        assert L.vi_last_error() and h.value is None, (first, count)
    for first in (0, base.n):
        res = base.gpu.radius_graph(1.0, 8, first=first, count=0)
        assert res.nq == 0 and res.total == 0
        assert np.array_equal(res.copy()[0], np.zeros(1, dtype=np.uint64))
        res.free()


# ---- 8. radius corner cases, partitioned handles ----
def test_negative_radius_nan_and_partitioned_handles(base, hip):
    ids = np.concatenate([base.ext[base.rows[:9]], u64([U64_MAX])])
    L = N.lib()
    st, h, found = raw_by_ids(base.gpu, ids, -1.0, 8, True)
    assert st == N.VI_OK and h.value
    res = vip.RangeResult(base.gpu, h, ids.size)
    assert res.total == 0 and np.array_equal(res.copy()[0], np.zeros(ids.size + 1, dtype=np.uint64))
    assert found.tolist() == [1] * 9 + [0]          # found is still filled
    res.free()
    ld, _, _, _, Fd = device_by_ids(hip, base.gpu, ids, -0.0, 8, True)      # -0.0 is 0.0: no copy of these records exists
    assert ld[-1] == 0 and Fd.tolist() == [1] * 9 + [0]
    g = base.gpu.radius_graph(-1.0, 8, first=0, count=100)
    assert g.total == 0 and g.nq == 100
    g.free()
    st, h, found = raw_by_ids(base.gpu, ids, float("nan"), 8, True)
    assert st == N.VI_ERR_INVALID_INPUT and b"NaN" in L.vi_last_error() and h.value is None and (found == 7).all()
    st, h, found = raw_by_ids(base.gpu, ids, 1.0, 0, True)
    assert st == N.VI_ERR_INVALID_INPUT and h.value is None and (found == 7).all()
    # a partitioned handle
    part = base.open(rank=0, world_size=2)
    dids = hip.upload(ids)
    for call in (lambda o: L.vi_indexer_range_search_by_ids(part._h, None, N.ptr(ids), ids.size, 1.0, 8, 1, N.ptr(found), o),
                 lambda o: L.vi_indexer_range_search_by_ids_device(part._h, None, dids, ids.size, 1.0, 8, 1, None, o),
                 lambda o: L.vi_indexer_radius_graph(part._h, None, 0, 4, 1.0, 8, 1, o)):
        h = C.c_void_p()
        assert call(C.byref(h)) == N.VI_ERR_INVALID_INPUT and h.value is None
        msg = L.vi_last_error()
        assert b"get_records_device" in msg and b"where" in msg and b"vi_range_merge_device" in msg, msg
    assert (found == 7).all()


# ---- 9. threads ----
def test_eight_threads_range_search_by_ids_and_get_on_one_handle(base):
    ids = base.ext[base.rows]
    radii, _ = radii_of(base)
    r = float(radii["r10"])
    parts = [ids[i::8][:30] for i in range(8)]
    want = [base.gpu.range_search_by_ids(p, r, 8) for p in parts]
    want_get = [base.gpu.get(p) for p in parts]
    errors = []

    def worker(t):
        try:
            for _ in range(4):
                lims, D, I, found = base.gpu.range_search_by_ids(parts[t], r, 8)
                assert np.array_equal(lims, want[t][0]) and np.array_equal(I, want[t][2]) and np.array_equal(bits(D), bits(want[t][1]))
                assert (found == 1).all()
                cnt, X, ts, where = base.gpu.get(parts[t])
                assert np.array_equal(X, want_get[t][1]) and np.array_equal(where, want_get[t][3])
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,), daemon=True) for t in range(8)]
    [t.start() for t in threads]
    [t.join(timeout=60) for t in threads]
    assert not any(t.is_alive() for t in threads), "deadlock: a thread is still waiting for a context"
    assert not errors, errors
    le, De, Ie = expected(base, 8, r, True)
    pos = {int(e): i for i, e in enumerate(ids)}
    q = pos[int(parts[0][0])]
    n0 = int(want[0][0][1])
    assert n0 == int(le[q + 1] - le[q]) and np.array_equal(want[0][2][:n0], Ie[int(le[q]):int(le[q + 1])])


# ---- 10. the Python surface ----
def test_python_surface(base):
    from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig
    ix = VectorIndexer.load(VectorIndexerConfig.new(base.dim).with_index_dir(base.idx).with_shards_dir(base.sh))
    radii, _ = radii_of(base)
    r = float(radii["r100"])
    le, De, Ie = expected(base, 8, r, True)
    nonempty = [i for i in range(NROWS) if le[i + 1] > le[i]][:3]
    assert len(nonempty) == 3
    for i in nonempty:
        me = int(base.ext[base.rows[i]])
        a, b = int(le[i]), int(le[i + 1])
        res = ix.range_search_similar(me, r, n_probe=8, include_vectors=True)
        assert [x.external_id for x in res] == Ie[a:b].tolist() and me not in [x.external_id for x in res]
        assert np.array_equal(bits([x.distance for x in res]), bits(De[a:b]))
        assert np.array_equal(np.array([x.vector for x in res], dtype=np.float32), base.X[base.rows_of(Ie[a:b])])
        with_self = ix.range_search_similar(me, r, n_probe=8, exclude_self=False)
        assert with_self[0].external_id == me and with_self[0].distance == 0.0 and len(with_self) == b - a + 1
        same = ix.range_search(base.X[base.rows[i]], r, n_probe=8)
        assert [x.external_id for x in same] == [x.external_id for x in with_self]
    assert ix.range_search_similar(U64_MAX, r, n_probe=8) is None
    assert ix.range_search_similar(int(base.ext[base.rows[0]]), -1.0) == []
    assert isinstance(ix.range_search_similar(int(base.ext[0]), r), list)         # n_probe None: the config's default
    lims, D, I, V, found = base.gpu.range_search_by_ids(base.ext[base.rows], r, 8, include_vectors=True)
    assert_csr((lims, D, I), (le, De, Ie), "VectorIndex.range_search_by_ids")
    assert (found == 1).all() and V.shape == (int(le[-1]), base.dim)
    with pytest.raises(vip.ViError) as e:
        base.gpu.radius_graph(r, 8, first=base.n, count=1)
    assert e.value.kind == "InvalidInput"
