"""GPU: the radius search through every public layer — the C entries' argument checks, VectorIndex.range_search_sync /
range_search_device, VectorIndexer.range_search and FaissStyleAdapter.range_search."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from vector_indexer_py import _native as N
from vector_indexer_py import api
from vector_indexer_py.harness import FaissStyleAdapter

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    class F:
        pass
    f = F()
    root = tmp_path_factory.mktemp("range_api")
    rng = np.random.default_rng(31)
    f.X = rng.standard_normal((3000, 32)).astype(np.float32)
    f.Q = np.concatenate([f.X[:20], rng.standard_normal((44, 32)).astype(np.float32)])
    f.ext = np.uint64(500) + np.uint64(3) * np.arange(3000, dtype=np.uint64)
    f.idx, f.sh = str(root / "index"), str(root / "shards")
    f.orc = O.OracleIndex.build(f.X, f.idx, f.sh, ext_ids=f.ext, nlist=12, now=NOW)
    f.gpu = vip.load(f.idx, f.sh, 32)
    rc, f.D, f.I = f.orc.search_batch(f.Q, 3000, 6)      # the whole sorted candidate sequence of every query
    assert rc == O.ORC_OK
    f.radius = float(np.median(f.D[:, 49]))
    return f


def expected(f, radius2, nq):
    hit = (f.I[:nq] >= 0) & (f.D[:nq] <= np.float32(radius2))
    return np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.uint64), f.D[:nq][hit], f.I[:nq][hit]


def raw(f, Q, dim, radius2, n_probe):
    out = C.c_void_p()
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    st = N.lib().vi_indexer_range_search(f.gpu._h, None, N.ptr(Q), Q.shape[0], dim, radius2, n_probe, C.byref(out))
    return st, out, N.lib().vi_last_error()


@pytest.mark.parametrize("case,status", [("nan_radius", N.VI_ERR_INVALID_INPUT), ("n_probe_0", N.VI_ERR_INVALID_INPUT),
                                         ("dimension", N.VI_ERR_INVALID_INPUT), ("nan_query", N.VI_ERR_PANIC),
                                         ("inf_query", N.VI_ERR_PANIC)])
def test_errors(fx, case, status):
    Q = fx.Q[:4].copy()
    if case == "nan_query":
        Q[2, 7] = np.nan
    if case == "inf_query":
        Q[0, 0] = np.inf
    st, out, msg = raw(fx, Q[:, :16] if case == "dimension" else Q, 16 if case == "dimension" else 32,
                       float("nan") if case == "nan_radius" else fx.radius, 0 if case == "n_probe_0" else 6)
    assert st == status and msg and not out.value, (st, msg)
    with pytest.raises(vip.ViError) as e:       # ... and as the Python layer reports it
        if case == "dimension":
            fx.gpu.range_search_sync(Q[:, :16], fx.radius, 6)
        else:
            fx.gpu.range_search_sync(Q, float("nan") if case == "nan_radius" else fx.radius, 0 if case == "n_probe_0" else 6)
    assert e.value.status == status and str(e.value)


def test_no_queries(fx):
    lims, D, I = fx.gpu.range_search_sync(np.zeros((0, 32), np.float32), fx.radius, 6)
    assert lims.tolist() == [0] and D.size == 0 and I.size == 0


def test_empty_index(tmp_path):
    """an index without a single list (index.bin: two empty arrays and the dimension): every query has zero results"""
    (tmp_path / "index").mkdir(), (tmp_path / "shards").mkdir()
    (tmp_path / "index" / "index.bin").write_bytes(bytes([1, 0, 0, 1, 0, 0, 8]))
    empty = vip.load(str(tmp_path / "index"), str(tmp_path / "shards"), 8)
    assert empty.num_centroids == 0
    lims, D, I = empty.range_search_sync(np.ones((5, 8), np.float32), float("inf"), 4)
    assert lims.tolist() == [0] * 6 and D.size == 0 and I.size == 0
    assert empty.last_stats()["n_probe_eff"] == 0


def test_a_handle_with_nothing_resident_is_an_error_as_for_a_search(tmp_path):
    cfg = api.VectorIndexerConfig.new(8).with_index_dir(tmp_path / "index").with_shards_dir(tmp_path / "shards")
    ix = api.VectorIndexer.new(cfg)
    out = C.c_void_p()
    q = np.zeros((1, 8), np.float32)
    st = N.lib().vi_indexer_range_search(ix._h, None, N.ptr(q), 1, 8, 1.0, 4, C.byref(out))
    assert st == N.VI_ERR_DEVICE and N.lib().vi_last_error() and not out.value


def test_a_window_that_admits_nothing(fx):
    flt = fx.gpu.filter_timestamps(5, 10)
    lims, D, I = fx.gpu.range_search_sync(fx.Q, float("inf"), 6, filter=flt)
    assert (lims == 0).all() and lims.shape == (65,) and D.size == 0 and I.size == 0


def test_host_entry_against_the_oracle_and_include_vectors(fx):
    for r in (fx.radius, 0.0, float("inf")):
        lims_e, De, Ie = expected(fx, r, 64)
        assert int(lims_e[-1]) > 0
        lims, D, I, V = fx.gpu.range_search_sync(fx.Q, r, 6, include_vectors=True)
        assert np.array_equal(lims, lims_e) and np.array_equal(I, Ie) and np.array_equal(bits(D), bits(De))
        assert V.shape == (I.size, 32) and np.array_equal(V, fx.X[(I - 500) // 3])      # the stored rows of the hits


def test_vector_indexer_range_search(fx):
    cfg = api.VectorIndexerConfig(32, fx.idx, fx.sh, default_n_probe=6)
    ix = api.VectorIndexer.load(cfg)
    lims_e, De, Ie = expected(fx, fx.radius, 64)
    for q in (0, 25, 63):
        a, b = int(lims_e[q]), int(lims_e[q + 1])
        res = ix.range_search(fx.Q[q].tolist(), fx.radius, include_vectors=(q == 25))      # n_probe: the config's default
        assert all(isinstance(x, api.SearchResult) for x in res)
        assert [x.external_id for x in res] == Ie[a:b].tolist()
        assert np.array_equal(bits(np.array([x.distance for x in res], dtype=np.float32)), bits(De[a:b]))
        assert [x.distance for x in res] == sorted(x.distance for x in res)
        if q == 25:
            assert all(np.array_equal(np.float32(x.vector), fx.X[(x.external_id - 500) // 3]) for x in res) and res
        else:
            assert all(x.vector is None for x in res)
    assert ix.range_search(fx.Q[0].tolist(), fx.radius, n_probe=10_000_000)      # clamped to max_n_probe, then to the lists
    with pytest.raises(vip.ViError) as e:
        ix.range_search(fx.Q[0].tolist()[:5], fx.radius)
    assert e.value.kind == "InvalidInput"
    assert ix.range_search(fx.Q[0].tolist(), fx.radius, timestamp_range=(5, 10)) == []


def test_faiss_style_adapter(fx):
    ad = FaissStyleAdapter(fx.gpu)
    ad.nprobe = 6
    lims, D, I = ad.range_search(fx.Q, fx.radius)
    lims_e, De, Ie = expected(fx, fx.radius, 64)
    assert lims.dtype == np.uint64 and lims.shape == (65,) and D.dtype == np.float32 and I.dtype == np.int64
    assert D.shape == I.shape == (int(lims[-1]),) and (np.diff(lims.astype(np.int64)) >= 0).all() and lims[0] == 0
    assert np.array_equal(lims, lims_e) and np.array_equal(I, Ie) and np.array_equal(bits(D), bits(De))
    ad.nprobe = 1
    assert int(ad.range_search(fx.Q, fx.radius)[0][-1]) < int(lims[-1])      # nprobe is the adapter's current setting


def test_device_entry_equals_the_host_entry(fx):
    from hiprt import Hip
    hip = Hip()
    try:
        xq = hip.upload(fx.Q)
        for r in (fx.radius, -3.0, float("inf")):
            lims_h, D_h, I_h = fx.gpu.range_search_sync(fx.Q, r, 6)
            res = fx.gpu.range_search_device(xq, 64, r, 6)
            assert res.total == int(lims_h[-1]) and res.lims_ptr
            assert np.array_equal(hip.download(res.lims_ptr, (65,), np.uint64), lims_h)
            if res.total:
                assert np.array_equal(hip.download(res.I_ptr, (res.total,), np.int64), I_h)
                assert np.array_equal(bits(hip.download(res.D_ptr, (res.total,), np.float32)), bits(D_h))
                tie = hip.download(res.tie_ptr, (res.total,), np.uint64)
                for q in (0, 30, 63):      # inside a query (distance, tie) ascends strictly: the stable order
                    a, b = int(lims_h[q]), int(lims_h[q + 1])
                    key = list(zip(bits(D_h[a:b]).tolist(), tie[a:b].tolist()))
                    assert key == sorted(key) and len(set(key)) == len(key)
            lims_c, D_c, I_c = res.copy()
            assert np.array_equal(lims_c, lims_h) and np.array_equal(I_c, I_h) and np.array_equal(bits(D_c), bits(D_h))
            res.free()
            assert res.D_ptr == 0
    finally:
        hip.close()
