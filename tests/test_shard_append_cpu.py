"""CPU: vi_shard_append_to — the file half of vi_indexer_add_records — writes, byte for byte, the shard file the oracle's
writer makes of the merged lists; and the argument errors of vi_indexer_add_records that need no device."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from vector_indexer_py import _native as N

import add_cases as A

SHARD = 7
CIDS = [3, 11, 4, 20, 9]          # file order; list 4 is empty
LENS = [5, 70, 0, 1, 130]


def _make_shard(tmp, dim, seed=0):
    rng = np.random.default_rng(seed)
    lists, nid = [], 0
    for n in LENS:
        ids = np.arange(nid, nid + n, dtype=np.uint64)
        lists.append((ids, ids * 3 + 1, 1_600_000_000 + ids, rng.standard_normal((n, dim)).astype(np.float32)))
        nid += n
    cent = rng.standard_normal((len(CIDS), dim)).astype(np.float32)
    d = str(tmp / "shards")
    (tmp / "shards").mkdir()
    assert O.shard_save(d, SHARD, dim, CIDS, cent, lists) == O.ORC_OK
    return d, nid


def _records(rng, cids, first_id, dim):
    n = len(cids)
    ids = np.arange(first_id, first_id + n, dtype=np.uint64)
    return (np.array(cids, dtype=np.uint64), ids, ids + 1000, 1_700_000_000 + ids,
            rng.standard_normal((n, dim)).astype(np.float32))


def _append(d, shard_id, rec):
    cids, ids, ext, ts, vecs = rec
    return N.lib().vi_shard_append_to(d.encode(), shard_id, len(cids), N.ptr(cids), N.ptr(ids), N.ptr(ext), N.ptr(ts),
                                      N.ptr(vecs))


@pytest.mark.parametrize("dim", [3, 16])
def test_append_is_byte_identical_to_the_oracle_writer(dim, tmp_path):
    """first, middle and last list of the shard and the empty list, interleaved in the call; then a second append"""
    d, nid = _make_shard(tmp_path, dim)
    rng = np.random.default_rng(1)
    rec = _records(rng, [9, 3, 4, 9, 11, 3, 4, 9, 3], nid, dim)   # 3 = first, 4 = empty middle, 11 = middle, 9 = last
    want = A.expected_append(d, str(tmp_path / "exp1"), SHARD, *rec)
    assert _append(d, SHARD, rec) == 0, N.lib().vi_last_error()
    assert A.shard_bytes(d, SHARD) == want
    assert sorted(p.name for p in (tmp_path / "shards").iterdir()) == [f"shard_{SHARD}.bin"]  # no temporary left
    rec2 = _records(rng, [4, 20, 20, 3], nid + 9, dim)
    want2 = A.expected_append(d, str(tmp_path / "exp2"), SHARD, *rec2)
    assert _append(d, SHARD, rec2) == 0
    assert A.shard_bytes(d, SHARD) == want2
    # the appended records come back behind the old ones, in call order
    rc, got = O.shard_get(d, SHARD, [3])
    assert rc == O.ORC_OK
    assert got[0][2][:, 0].tolist() == list(range(5)) + [nid + 1, nid + 5, nid + 8, nid + 12]


@pytest.mark.parametrize("dim", [3, 16])
def test_append_nothing_and_unknown_centroid_leave_the_file(dim, tmp_path):
    d, nid = _make_shard(tmp_path, dim)
    before = A.shard_bytes(d, SHARD)
    assert N.lib().vi_shard_append_to(d.encode(), SHARD, 0, None, None, None, None, None) == 0
    assert A.shard_bytes(d, SHARD) == before
    rec = _records(np.random.default_rng(2), [3, 12345, 9], nid, dim)
    assert _append(d, SHARD, rec) == N.VI_ERR_NOT_FOUND
    assert b"Centroid 12345 not found" in N.lib().vi_last_error()
    assert A.shard_bytes(d, SHARD) == before
    assert sorted(p.name for p in (tmp_path / "shards").iterdir()) == [f"shard_{SHARD}.bin"]


def test_append_reader_errors(tmp_path):
    """a missing and a truncated file give the error kinds of the reader (ShardFile::open)"""
    d, nid = _make_shard(tmp_path, 16)
    rec = _records(np.random.default_rng(3), [3], nid, 16)
    assert _append(d, 999, rec) == N.VI_ERR_OTHER
    p = tmp_path / "shards" / f"shard_{SHARD}.bin"
    raw = p.read_bytes()
    cids = np.array([3], dtype=np.uint64)

    def reader_kind():
        dim, counts = C.c_uint32(0), np.zeros(1, dtype=np.uint64)
        return N.lib().vi_shard_get_centroid_vectors_from(d.encode(), SHARD, N.ptr(cids), 1, C.byref(dim), N.ptr(counts),
                                                          None, None, None)

    for cut in (20, len(raw) - 40):   # inside the header; inside the last list's records
        p.write_bytes(raw[:cut])
        kind = reader_kind()
        assert kind != 0
        assert _append(d, SHARD, rec) == kind
        assert p.read_bytes() == raw[:cut]
    assert sorted(q.name for q in (tmp_path / "shards").iterdir()) == [f"shard_{SHARD}.bin"]


def test_add_records_argument_errors_without_gpu(tmp_path):
    """detected before any file or device work"""
    L = N.lib()
    x = np.ones((2, 8), dtype=np.float32)
    assert L.vi_indexer_add_records(None, None, N.ptr(x), None, 2) == N.VI_ERR_INVALID_INPUT
    cfg = N.Config()
    L.vi_config_init(C.byref(cfg), 8)
    keep = (str(tmp_path / "i").encode(), str(tmp_path / "s").encode())
    cfg.index_dir, cfg.shards_dir = keep
    h = C.c_void_p()
    assert L.vi_indexer_new(C.byref(cfg), C.byref(h)) == 0
    try:
        assert L.vi_indexer_add_records(h, None, N.ptr(x), None, 2) == N.VI_ERR_INVALID_INPUT   # no index
        assert b"no index" in L.vi_last_error()
        assert L.vi_indexer_add_records(h, None, None, None, 2) == N.VI_ERR_INVALID_INPUT
        assert L.vi_last_error() == b"null values"
        bad = x.copy()
        bad[1, 3] = np.nan
        assert L.vi_indexer_add_records(h, None, N.ptr(bad), None, 2) == N.VI_ERR_INVALID_INPUT
        assert L.vi_last_error() == b"non-finite value at flat index 11"
        bad[1, 3] = np.inf
        assert L.vi_indexer_add_records(h, None, N.ptr(bad), None, 2) == N.VI_ERR_INVALID_INPUT
        assert L.vi_indexer_add_records(h, None, None, None, 0) == 0    # nothing to add: nothing happens
        st = N.AddStats()
        assert L.vi_indexer_last_add_stats(h, C.byref(st)) == 0 and st.n == 0
        assert not (tmp_path / "i").exists() and not (tmp_path / "s").exists()
    finally:
        L.vi_indexer_free(h)
