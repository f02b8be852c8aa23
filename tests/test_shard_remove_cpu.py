"""CPU: vi_shard_remove_from — the file half of vi_indexer_remove_ids — writes, byte for byte, the shard file the oracle's
writer makes of the remaining lists; and the argument errors of the remove entries that need no device."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from vector_indexer_py import _native as N

import remove_cases as R

SHARD = 7
CIDS = [3, 11, 4, 20, 9]          # file order; list 4 is empty, list 20 has one record
LENS = [5, 70, 0, 1, 130]
U64_MAX = (1 << 64) - 1
SHARED = 777                      # an external id two records carry (lists 3 and 9)


def _make_shard(tmp, dim, seed=0):
    """external id of internal id i: 3 i + 1, but 0 for id 2 (list 3), 2^64 - 1 for id 10 (list 11), SHARED for ids 4
    (list 3) and 100 (list 9)"""
    rng = np.random.default_rng(seed)
    lists, nid = [], 0
    for n in LENS:
        ids = np.arange(nid, nid + n, dtype=np.uint64)
        ext = ids * np.uint64(3) + np.uint64(1)
        for i, e in ((2, 0), (10, U64_MAX), (4, SHARED), (100, SHARED)):
            ext[ids == i] = np.uint64(e)
        lists.append((ids, ext, np.uint64(1_600_000_000) + ids, rng.standard_normal((n, dim)).astype(np.float32)))
        nid += n
    cent = rng.standard_normal((len(CIDS), dim)).astype(np.float32)
    d = str(tmp / "shards")
    (tmp / "shards").mkdir()
    assert O.shard_save(d, SHARD, dim, CIDS, cent, lists) == O.ORC_OK
    return d


def _remove(d, shard_id, ids):
    a = np.array(ids, dtype=np.uint64)
    removed = C.c_uint64(12345)
    rc = N.lib().vi_shard_remove_from(d.encode(), shard_id, N.ptr(a) if a.size else None, a.size, C.byref(removed))
    return rc, removed.value


def _only_the_shard(tmp):
    return sorted(p.name for p in (tmp / "shards").iterdir()) == [f"shard_{SHARD}.bin"]


def _ext(i):
    return 3 * i + 1


@pytest.mark.parametrize("dim", [3, 16])      # D = 3: four pad bytes behind every record
def test_remove_is_byte_identical_to_the_oracle_writer(dim, tmp_path):
    d = _make_shard(tmp_path, dim)
    # unsorted, with duplicates: ids 0 and 2^64 - 1, the shared id (two records), the one record of list 20 (id 75), the
    # first, a middle and the last record of list 9 (ids 76, 150, 205), a run inside list 11, and ids nobody carries
    gone = [_ext(205), 0, SHARED, _ext(75), 5, U64_MAX, _ext(76), 999_999, _ext(150), 0, _ext(205), 2, U64_MAX - 1]
    gone += [_ext(i) for i in range(30, 41)] + [SHARED]
    n_want = 1 + 1 + 2 + 1 + 3 + 11
    want, n_exp = R.expected_remove(d, str(tmp_path / "exp1"), SHARD, gone, dim)
    assert n_exp == n_want
    rc, removed = _remove(d, SHARD, gone)
    assert rc == 0, N.lib().vi_last_error()
    assert removed == n_want
    assert R.shard_bytes(d, SHARD) == want
    assert _only_the_shard(tmp_path)                      # no temporary left
    # the emptied list keeps its entry and the oracle reads it back empty; the others close up in their old order
    assert R.shard_centroid_ids(d, SHARD) == CIDS
    rc, got = O.shard_get(d, SHARD, [20, 3, 4])
    assert rc == O.ORC_OK
    assert [len(g[2]) for g in got] == [0, 3, 0]
    assert got[1][2][:, 0].tolist() == [0, 1, 3]          # VectorMeta.id of kept records is unchanged
    # a second removal, from the file the first one wrote: the rest of list 3, and ids that are gone already
    gone2 = [_ext(0), _ext(1), _ext(3), SHARED, 0, _ext(76)]
    want2, n2 = R.expected_remove(d, str(tmp_path / "exp2"), SHARD, gone2, dim)
    rc, removed = _remove(d, SHARD, gone2)
    assert (rc, removed, n2) == (0, 3, 3)
    assert R.shard_bytes(d, SHARD) == want2
    rc, got = O.shard_get(d, SHARD, CIDS)
    assert rc == O.ORC_OK and [len(g[2]) for g in got] == [0, 58, 0, 0, 126]


@pytest.mark.parametrize("dim", [3, 16])
def test_no_match_leaves_the_file(dim, tmp_path):
    d = _make_shard(tmp_path, dim)
    before = R.shard_bytes(d, SHARD)
    for ids in ([], [5, 999_999, U64_MAX - 1, 2]):
        rc, removed = _remove(d, SHARD, ids)
        assert (rc, removed) == (0, 0)
        assert R.shard_bytes(d, SHARD) == before
        assert _only_the_shard(tmp_path)
    assert N.lib().vi_shard_remove_from(d.encode(), SHARD, None, 0, None) == 0    # removed_out is optional


def test_remove_reader_errors(tmp_path):
    """a missing and a truncated file give the error kinds of the reader; the file stays as it is"""
    d = _make_shard(tmp_path, 16)
    assert _remove(d, 999, [_ext(0)]) == (N.VI_ERR_OTHER, 0)
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
        assert _remove(d, SHARD, [_ext(0)]) == (kind, 0)
        assert p.read_bytes() == raw[:cut]
    assert _only_the_shard(tmp_path)
    a = np.array([1], dtype=np.uint64)
    assert N.lib().vi_shard_remove_from(None, SHARD, N.ptr(a), 1, None) == N.VI_ERR_INVALID_INPUT
    assert N.lib().vi_shard_remove_from(d.encode(), SHARD, None, 1, None) == N.VI_ERR_INVALID_INPUT


def test_remove_entries_argument_errors_without_gpu(tmp_path):
    """detected before any file or device work"""
    L = N.lib()
    ids = np.array([1, 2], dtype=np.uint64)
    removed = C.c_uint64(7)
    assert L.vi_indexer_remove_ids(None, N.ptr(ids), 2, C.byref(removed)) == N.VI_ERR_INVALID_INPUT
    assert L.vi_indexer_retain(None, None, C.byref(removed)) == N.VI_ERR_INVALID_INPUT
    assert removed.value == 0
    cfg = N.Config()
    L.vi_config_init(C.byref(cfg), 8)
    keep = (str(tmp_path / "i").encode(), str(tmp_path / "s").encode())
    cfg.index_dir, cfg.shards_dir = keep
    h = C.c_void_p()
    assert L.vi_indexer_new(C.byref(cfg), C.byref(h)) == 0
    try:
        assert L.vi_indexer_remove_ids(h, N.ptr(ids), 2, None) == N.VI_ERR_INVALID_INPUT     # no index
        assert b"no index" in L.vi_last_error()
        assert L.vi_indexer_retain(h, None, None) == N.VI_ERR_INVALID_INPUT
        st = N.RemoveStats()
        assert L.vi_indexer_last_remove_stats(h, C.byref(st)) == 0 and st.n_removed == 0
        assert L.vi_indexer_last_remove_stats(h, None) == N.VI_ERR_INVALID_INPUT
        assert not (tmp_path / "i").exists() and not (tmp_path / "s").exists()
    finally:
        L.vi_indexer_free(h)
