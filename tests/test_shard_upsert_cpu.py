"""CPU: vi_shard_upsert_to — the file half of vi_indexer_upsert_records — writes, byte for byte, the shard file the
oracle's reader and writer make by removing and then appending, and the file vi_shard_remove_from followed by
vi_shard_append_to leaves; shard_update_write itself (emptied, all-new and unchanged-length lists, a rename that fails)
in a stand-alone host program, plain and under the sanitizers; and the argument errors that need no device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from vector_indexer_py import _native as N

import upsert_cases as U
from add_cases import shard_bytes, shard_centroid_ids
from test_shard_remove_cpu import CIDS, LENS, SHARD, SHARED, U64_MAX, _ext, _make_shard, _only_the_shard

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "vector-indexer_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _call(rng, dim):
    """unsorted, with duplicates.  By list of the file (ids 0..4 | 5..74 | none | 75 | 76..205):
    3: loses ids 2 (external id 0) and 4 (SHARED) and receives 2: its length stays; 11: loses a run and id 10
    (2^64 - 1), receives 3; 4: empty, receives 2 (all new); 20: loses its one record, receives nothing (emptied);
    9: loses id 100 (SHARED) and its last, receives every other row of the call, those of the ids nobody carries and
    of the ids named twice among them"""
    ext = [0, SHARED, U64_MAX] + [_ext(i) for i in range(30, 41)] + [_ext(75), _ext(205), 999_999, 5, SHARED, 0]
    cid = [3, 3, 11, 11, 11, 4, 4]
    cid = cid + [9] * (len(ext) - len(cid))
    order = rng.permutation(len(ext))
    ext, cid = np.array(ext, dtype=np.uint64)[order], np.array(cid, dtype=np.uint64)[order]
    n = len(ext)
    return dict(ext=ext, cid=cid, ids=np.arange(500, 500 + n, dtype=np.uint64), ts=np.uint64(9000) + np.arange(n, dtype=np.uint64),
                vecs=rng.standard_normal((n, dim)).astype(np.float32))


def _upsert(d, shard_id, c):
    removed = C.c_uint64(12345)
    n = len(c["ext"])
    rc = N.lib().vi_shard_upsert_to(d.encode(), shard_id, n, N.ptr(c["cid"]), N.ptr(c["ids"]), N.ptr(c["ext"]), N.ptr(c["ts"]),
                                    N.ptr(c["vecs"]), C.byref(removed))
    return rc, removed.value


N_GONE = 2 + 1 + 11 + 1 + 2      # list 3; id 10; the run of list 11; list 20; id 100 and the last of list 9


@pytest.mark.parametrize("dim", [3, 16])      # D = 3: four pad bytes behind every record
def test_upsert_is_byte_identical_to_the_oracle_and_to_remove_then_append(dim, tmp_path):
    d = _make_shard(tmp_path, dim)
    c = _call(np.random.default_rng(dim), dim)
    want, n_exp = U.expected_upsert(d, str(tmp_path / "exp"), SHARD, c["ext"], c["cid"], c["ids"], c["ext"], c["ts"], c["vecs"], dim)
    assert n_exp == N_GONE
    # the two existing calls, on a copy
    pair = tmp_path / "pair"
    shutil.copytree(tmp_path / "shards", pair / "shards")
    removed = C.c_uint64(0)
    assert N.lib().vi_shard_remove_from(str(pair / "shards").encode(), SHARD, N.ptr(c["ext"]), len(c["ext"]), C.byref(removed)) == 0
    assert N.lib().vi_shard_append_to(str(pair / "shards").encode(), SHARD, len(c["ext"]), N.ptr(c["cid"]), N.ptr(c["ids"]),
                                      N.ptr(c["ext"]), N.ptr(c["ts"]), N.ptr(c["vecs"])) == 0
    assert removed.value == N_GONE
    rc, got_removed = _upsert(d, SHARD, c)
    assert rc == 0, N.lib().vi_last_error()
    assert got_removed == N_GONE
    assert shard_bytes(d, SHARD) == want
    assert shard_bytes(d, SHARD) == shard_bytes(str(pair / "shards"), SHARD)
    assert _only_the_shard(tmp_path)                      # no temporary left
    assert shard_centroid_ids(d, SHARD) == CIDS
    rc, got = O.shard_get(d, SHARD, CIDS)
    assert rc == O.ORC_OK
    received = [int((c["cid"] == cid).sum()) for cid in CIDS]
    assert received[:4] == [2, 3, 2, 0]
    assert [len(g[2]) for g in got] == [LENS[0], LENS[1] - 12 + 3, 2, 0, LENS[4] - 2 + received[4]]
    assert got[0][2][:3, 0].tolist() == [0, 1, 3]         # kept records first, VectorMeta.id unchanged ...
    assert got[0][2][3:, 0].tolist() == c["ids"][c["cid"] == 3].tolist()      # ... then the new ones in call order
    assert got[2][2][:, 1].tolist() == c["ext"][c["cid"] == 4].tolist()
    # a second upsert of the file the first wrote: the emptied list receives, an id named twice before loses both records
    c2 = dict(ext=np.array([SHARED, 77, 78], dtype=np.uint64), cid=np.array([20, 20, 3], dtype=np.uint64),
              ids=np.array([900, 901, 902], dtype=np.uint64), ts=np.array([1, 2, 3], dtype=np.uint64),
              vecs=np.ones((3, dim), dtype=np.float32))
    want2, n2 = U.expected_upsert(d, str(tmp_path / "exp2"), SHARD, c2["ext"], c2["cid"], c2["ids"], c2["ext"], c2["ts"], c2["vecs"], dim)
    rc, got_removed = _upsert(d, SHARD, c2)
    assert (rc, got_removed, n2) == (0, 2, 2)
    assert shard_bytes(d, SHARD) == want2


@pytest.mark.parametrize("dim", [3, 16])
def test_unknown_centroid_and_n_zero_leave_the_file(dim, tmp_path):
    d = _make_shard(tmp_path, dim)
    before = shard_bytes(d, SHARD)
    c = _call(np.random.default_rng(1), dim)
    c["cid"][len(c["cid"]) // 2] = 12345
    rc, removed = _upsert(d, SHARD, c)
    assert (rc, removed) == (N.VI_ERR_NOT_FOUND, 0)
    assert b"Centroid 12345 not found" in N.lib().vi_last_error()
    assert shard_bytes(d, SHARD) == before and _only_the_shard(tmp_path)
    removed = C.c_uint64(9)
    assert N.lib().vi_shard_upsert_to(d.encode(), SHARD, 0, None, None, None, None, None, C.byref(removed)) == 0
    assert removed.value == 0
    assert N.lib().vi_shard_upsert_to(d.encode(), SHARD, 0, None, None, None, None, None, None) == 0     # removed_out is optional
    assert shard_bytes(d, SHARD) == before and _only_the_shard(tmp_path)
    # the reader's errors, and null pointers
    assert N.lib().vi_shard_upsert_to(d.encode(), 999, 0, None, None, None, None, None, None) == N.VI_ERR_OTHER
    assert N.lib().vi_shard_upsert_to(None, SHARD, 0, None, None, None, None, None, None) == N.VI_ERR_INVALID_INPUT
    assert N.lib().vi_shard_upsert_to(d.encode(), SHARD, 2, N.ptr(c["cid"]), N.ptr(c["ids"]), None, N.ptr(c["ts"]), N.ptr(c["vecs"]),
                                      None) == N.VI_ERR_INVALID_INPUT
    assert shard_bytes(d, SHARD) == before and _only_the_shard(tmp_path)


def test_upsert_entry_argument_errors_without_gpu(tmp_path):
    """detected before any file or device work"""
    L = N.lib()
    ids = np.array([1, 2], dtype=np.uint64)
    x = np.zeros((2, 8), dtype=np.float32)
    replaced = C.c_uint64(7)
    assert L.vi_indexer_upsert_records(None, N.ptr(ids), N.ptr(x), None, 2, C.byref(replaced)) == N.VI_ERR_INVALID_INPUT
    assert replaced.value == 0
    cfg = N.Config()
    L.vi_config_init(C.byref(cfg), 8)
    keep = (str(tmp_path / "i").encode(), str(tmp_path / "s").encode())
    cfg.index_dir, cfg.shards_dir = keep
    h = C.c_void_p()
    assert L.vi_indexer_new(C.byref(cfg), C.byref(h)) == 0
    try:
        assert L.vi_indexer_upsert_records(h, None, None, None, 0, C.byref(replaced)) == 0                  # n == 0
        assert L.vi_indexer_upsert_records(h, None, N.ptr(x), None, 2, None) == N.VI_ERR_INVALID_INPUT     # null ids
        assert L.vi_indexer_upsert_records(h, N.ptr(ids), None, None, 2, None) == N.VI_ERR_INVALID_INPUT   # null values
        assert L.vi_indexer_upsert_records(h, N.ptr(ids), N.ptr(x), None, 1 << 32, None) == N.VI_ERR_INVALID_INPUT
        assert b"2^32 - 2" in L.vi_last_error()
        bad = x.copy()
        bad[1, 3] = np.inf
        assert L.vi_indexer_upsert_records(h, N.ptr(ids), N.ptr(bad), None, 2, None) == N.VI_ERR_INVALID_INPUT
        assert b"non-finite value at flat index 11" in L.vi_last_error()
        assert L.vi_indexer_upsert_records(h, N.ptr(ids), N.ptr(x), None, 2, C.byref(replaced)) == N.VI_ERR_INVALID_INPUT   # no index
        assert b"no index" in L.vi_last_error() and replaced.value == 0
        st = N.UpsertStats()
        assert L.vi_indexer_last_upsert_stats(h, C.byref(st)) == 0 and (st.n, st.n_replaced) == (0, 0)
        assert L.vi_indexer_last_upsert_stats(h, None) == N.VI_ERR_INVALID_INPUT
        assert not (tmp_path / "i").exists() and not (tmp_path / "s").exists()
    finally:
        L.vi_indexer_free(h)


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    work = tmp_path / (name + "_work")
    work.mkdir()
    cmd = [CXX, "-std=c++17", *flags, "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"), "-I", CSRC,
           os.path.join(HERE, "shard_upsert_check.cpp"), os.path.join(CSRC, "shards.cpp"), "-o", exe]
    cc = subprocess.run(cmd, capture_output=True, text=True)
    return cc, (subprocess.run([exe, str(work)], capture_output=True, text=True) if cc.returncode == 0 else None)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_shard_update_write_lists_and_rename_failure(tmp_path):
    cc, run = _run(tmp_path, "shard_upsert_check", [])
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_shard_update_write_under_sanitizers(tmp_path):
    """the same stand-alone program with AddressSanitizer and UBSan (host code only, nothing preloaded)"""
    cc, run = _run(tmp_path, "shard_upsert_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if cc.returncode != 0 and any(w in cc.stderr for w in ("sanitize", "asan", "ubsan")):
        pytest.skip("the host compiler has no sanitizer runtimes")  # (the source itself compiles: the test above)
    assert cc.returncode == 0, cc.stderr
    assert run.returncode == 0 and run.stdout == "", run.stdout + run.stderr
