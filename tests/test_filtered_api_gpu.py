"""GPU: the timestamp-window filter through the Python mirrors of the public API — api.SearchRequest.with_timestamp_range,
VectorIndex.search_sync(filter=...) — on indexes built by the product itself (records and vector file), and on the same
files loaded again: both ways of making an index resident must fill the resident timestamps identically."""
import struct

import numpy as np
import pytest

import vector_indexer_py as vip
from vector_indexer_py.api import SearchRequest, VectorIndexer, VectorIndexerConfig, VectorRecord

pytestmark = pytest.mark.gpu

NOW = 1_700_000_123


def cfg_for(tmp_path, dim, **kw):
    c = VectorIndexerConfig.new(dim).with_index_dir(tmp_path / "index").with_shards_dir(tmp_path / "shards")
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def data(n=3000, d=16, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    ts = 1000 + (np.arange(n) * 7919) % 1000
    ts[::97] = 0
    return X, ts.astype(np.uint64)


def brute(X, stored, q, lo, hi, k):
    """exhaustive filtered neighbours of one query, reference arithmetic: sequential f32 sum, stable by row"""
    acc = np.zeros(X.shape[0], dtype=np.float32)
    for j in range(X.shape[1]):
        t = (q[j] - X[:, j]).astype(np.float32)
        acc = (acc + t * t).astype(np.float32)
    ok = np.nonzero((stored >= lo) & (stored <= hi))[0]
    order = ok[np.argsort(acc[ok], kind="stable")][:k]
    return order, acc[order]


def test_search_request_with_timestamp_range(tmp_path):
    X, ts = data()
    stored = np.where(ts == 0, NOW, ts)
    recs = [VectorRecord(i, X[i].tolist(), int(ts[i]) or None) for i in range(len(X))]
    ix = VectorIndexer.new(cfg_for(tmp_path, 16, now_secs=NOW)).build_from_records(recs)
    nlists = 10_000   # n_probe >= #lists: exhaustive, so the brute-force answer is the expected SET and distances
    for lo, hi in [(1000, 1099), (1500, 1500), (NOW, NOW), (0, 2**64 - 1), (5, 10)]:
        for qi in (0, 97, 1234):
            req = SearchRequest(X[qi].tolist(), True, 20, nlists).with_timestamp_range(lo, hi)
            assert req.timestamp_range == (lo, hi)
            res = ix.search(req)
            rows, dist = brute(X, stored, X[qi], lo, hi, 20)
            assert len(res) == len(rows)
            assert np.array_equal(np.array([r.distance for r in res], dtype=np.float32), dist)
            assert sorted(r.external_id for r in res) == sorted(rows.tolist()) or len(set(dist.tolist())) < len(dist)
            assert all(lo <= stored[r.external_id] <= hi for r in res)
            assert all(np.array_equal(np.float32(r.vector), X[r.external_id]) for r in res)
    assert len(ix._filters) == 5   # one native filter per range, made once
    plain = ix.search(SearchRequest(X[0].tolist(), False, 20, nlists))
    assert [r.external_id for r in plain] == [r.external_id for r in
                                              ix.search(SearchRequest(X[0].tolist(), False, 20, nlists).with_timestamp_range(0, 2**64 - 1))]
    with pytest.raises(RuntimeError) as e:
        ix.search(SearchRequest(X[0].tolist(), False, 5, 5).with_timestamp_range(9, 3))
    assert e.value.kind == "InvalidInput"


def test_built_and_loaded_index_agree_under_every_window(tmp_path):
    X, ts = data(seed=1)
    ext = (np.arange(len(X), dtype=np.uint64) * 3 + 11)
    built = vip.build(X, str(tmp_path), now_secs=NOW, ext_ids=ext, timestamps=ts)
    loaded = vip.load(str(tmp_path / "index"), str(tmp_path / "shards"), 16)
    stored = np.where(ts == 0, NOW, ts)
    Q = np.concatenate([X[:20], X[100:140] + np.float32(0.25)])
    for lo, hi in [(1000, 1099), (1500, 1502), (NOW, NOW), (0, 2**64 - 1), (5, 10), (1000, 1499)]:
        fb, fl = built.filter_timestamps(lo, hi), loaded.filter_timestamps(lo, hi)
        want = int(((stored >= lo) & (stored <= hi)).sum())
        assert fb.num_allowed == fl.num_allowed == want
        for k, p in [(10, 8), (100, 10_000), (200, 4)]:
            Db, Ib, Vb = built.search_sync(Q, k, p, include_vectors=True, filter=fb)
            Dl, Il, Vl = loaded.search_sync(Q, k, p, include_vectors=True, filter=fl)
            assert np.array_equal(Ib, Il) and np.array_equal(Db.view(np.uint32), Dl.view(np.uint32)) and np.array_equal(Vb, Vl)
            rows = np.where(Ib >= 0, (Ib - 11) // 3, 0)
            assert ((Ib < 0) | ((stored[rows] >= lo) & (stored[rows] <= hi))).all()
        rows, dist = brute(X, stored, Q[3], lo, hi, 10)
        D, I = built.search_sync(Q[3:4], 10, 10_000, filter=fb)
        assert np.array_equal(D[0, :len(rows)], dist) and (I[0, len(rows):] == -1).all()


def _varint(v):
    if v < 251:
        return bytes([v])
    if v <= 0xFFFF:
        return bytes([251]) + struct.pack("<H", v)
    if v <= 0xFFFFFFFF:
        return bytes([252]) + struct.pack("<I", v)
    return bytes([253]) + struct.pack("<Q", v)


def test_build_from_vector_file_keeps_the_file_s_timestamps(tmp_path):
    dim, n = 8, 400
    rng = np.random.default_rng(2)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    ts = 2000 + (np.arange(n) * 31) % 50
    ts[::41] = 0
    blob = b""
    for lo, hi in [(0, 250), (250, n)]:   # two appended bincode batches of Vec<(u64, Vec<f32>, u64)> (utils.rs:34-107)
        blob += _varint(hi - lo)
        for i in range(lo, hi):
            blob += _varint(i) + _varint(dim) + X[i].astype("<f4").tobytes() + _varint(int(ts[i]))
    vf = tmp_path / "vectors.bin"
    vf.write_bytes(blob)
    cfg = cfg_for(tmp_path, dim, now_secs=NOW)
    ix = VectorIndexer.new(cfg).build_from_vector_file(vf)
    loaded = VectorIndexer.load(cfg)
    stored = np.where(ts == 0, NOW, ts)
    for lo, hi in [(2000, 2009), (2049, 2049), (NOW, NOW), (0, 1999)]:
        req = SearchRequest(X[5].tolist(), False, 400, 10_000).with_timestamp_range(lo, hi)
        a, b = ix.search(req), loaded.search(req)
        want = set(np.nonzero((stored >= lo) & (stored <= hi))[0].tolist())
        assert {r.external_id for r in a} == want == {r.external_id for r in b}
        assert [(r.external_id, r.distance) for r in a] == [(r.external_id, r.distance) for r in b]
