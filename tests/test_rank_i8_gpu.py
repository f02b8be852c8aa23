"""GPU parity of the int8 list rank (rank_stream.hip: rank_stream_i8_kernel): 8-bit descriptors against queries of
integers in 0..254 are ranked with exact int8 products in the frame shifted by 127; a batch holding a 255 or a
non-integer falls back to the bf16 kernel.  Every case: the oracle's ids AND distance bits, and `rank_int8` in the
search stats says which kernel ran."""
import os

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from hiprt import Hip as _Hip

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def _stream(monkeypatch):
    if os.environ.get("VI_FILTER") == "0" or os.environ.get("VI_FILTER_BF16") == "0" or os.environ.get("VI_FILTER_HI_ONLY") == "0":
        pytest.skip("the int8 rank belongs to the bf16 MFMA engine's streaming kernel")
    monkeypatch.setenv("VI_RANK_STREAM", "1")   # below D = 97 the streaming kernel runs only when asked for
    monkeypatch.delenv("VI_RANK_I8", raising=False)
    yield


def build(tmp_path, X, nlist=0):
    idx, sh = str(tmp_path / "index"), str(tmp_path / "shards")
    orc = O.OracleIndex.build(X, idx, sh, nlist=nlist, seed=42)
    return orc, vip.load(idx, sh, X.shape[1])


def check(orc, gpu, Q, k, n_probe, int8):
    rc, Do, Io = orc.search_batch(Q, k, n_probe)
    assert rc == O.ORC_OK
    Dg, Ig = gpu.search_sync(Q, k, n_probe)
    bad = np.nonzero((Ig != Io).any(axis=1) | (bits(Dg) != bits(Do)).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} queries differ, first {bad[0]}: gpu {Ig[bad[0]]} {Dg[bad[0]]} oracle {Io[bad[0]]} {Do[bad[0]]}"
    st = gpu.last_stats()
    assert st["rank_int8"] == int8, (k, n_probe, st)
    assert st["rank_mode"] == 3, st
    return Dg, Ig


def descriptors(rng, n, d):
    """SIFT-like bytes with the extremes: 0 and 255 in every dimension, duplicates, an all-zero and an all-255 vector"""
    X = np.minimum(rng.gamma(0.6, 40.0, size=(n, d)), 255.0).astype(np.int64)
    X[rng.integers(0, n, n // 50), rng.integers(0, d, n // 50)] = 255
    X[rng.integers(0, n, n // 50), rng.integers(0, d, n // 50)] = 0
    X[100:140] = X[0:40]        # duplicates
    X[200] = 0
    X[201] = 255
    X[202] = X[200]
    return X.astype(np.float32)


def queries(rng, X, nq):
    """integers in 0..254 with both extremes, stored vectors among them (distance 0, ties across sub-blocks)"""
    n, d = X.shape
    Q = np.clip(X[rng.integers(0, n, nq)] + rng.integers(-6, 7, size=(nq, d)), 0, 254)
    Q[: nq // 8] = np.minimum(X[: nq // 8], 254)     # stored vectors (those without a 255 exactly)
    Q[nq // 8] = 0                                   # equal to the all-zero vector
    Q[nq // 8 + 1] = 254
    Q[nq // 8 + 2, :: 2] = 0
    return np.ascontiguousarray(Q, dtype=np.float32)


@pytest.mark.parametrize("d,n,nlist", [(16, 9000, 0), (48, 12000, 0), (100, 12000, 0), (128, 16000, 0),
                                       (128, 24000, 4)])   # lists of ~6000 vectors: three segments each
def test_int8_rank_parity(d, n, nlist, tmp_path):
    rng = np.random.default_rng(d * 1000 + n)
    X = descriptors(rng, n, d)
    orc, gpu = build(tmp_path, X, nlist)
    Q = queries(rng, X, 300)
    for k, n_probe in [(10, 16), (1, 1), (64, 64), (100, 16), (10, 64)]:
        check(orc, gpu, Q, k, n_probe, 1)


def test_int8_rank_falls_back_per_batch(tmp_path):
    """a 255 or a non-integer anywhere in a batch sends that batch to the bf16 kernel; batches alternate on one handle"""
    rng = np.random.default_rng(5)
    X = descriptors(rng, 12000, 128)
    orc, gpu = build(tmp_path, X)
    Q = queries(rng, X, 260)
    Q255 = Q.copy()
    Q255[17, 33] = 255.0
    Qhalf = Q.copy()
    Qhalf[200, 5] = 7.5
    Qneg = Q.copy()
    Qneg[3, 0] = -1.0
    for _ in range(2):
        for Qb, int8 in [(Q, 1), (Q255, 0), (Q[::-1].copy(), 1), (Qhalf, 0), (Q, 1), (Qneg, 0)]:
            check(orc, gpu, Qb, 10, 16, int8)


def test_int8_rank_matches_the_bf16_kernel_bit_for_bit(tmp_path, monkeypatch):
    rng = np.random.default_rng(9)
    X = descriptors(rng, 16000, 128)
    orc, gpu = build(tmp_path, X, 0)
    Q = queries(rng, X, 400)
    for k, n_probe in [(10, 32), (100, 8), (1, 64)]:
        D1, I1 = check(orc, gpu, Q, k, n_probe, 1)
        monkeypatch.setenv("VI_RANK_I8", "0")
        D0, I0 = check(orc, gpu, Q, k, n_probe, 0)
        monkeypatch.delenv("VI_RANK_I8")
        assert (I0 == I1).all() and (bits(D0) == bits(D1)).all()


@pytest.mark.parametrize("placement", [0, 1])
def test_int8_rank_on_ranks_merges_to_the_single_gpu_result(placement, tmp_path):
    """stripes (block b of every list on rank b % world) and whole shard files per rank, each rank ranking its own
    int8 image: the merged per-rank top-k equal the oracle's"""
    from vector_indexer_py import _native
    world, d = 3, 48
    rng = np.random.default_rng(41 + placement)
    X = descriptors(rng, 15000, d)
    orc, full = build(tmp_path, X, 30)
    idx, sh = str(tmp_path / "index"), str(tmp_path / "shards")
    parts = [vip.load(idx, sh, d, rank=r, world_size=world, placement=placement) for r in range(world)]
    assert sum(p.num_vectors for p in parts) == X.shape[0]
    Q = queries(rng, X, 250)
    hip = _Hip()
    try:
        nq = Q.shape[0]
        xq = hip.upload(Q)
        for k, n_probe in [(10, 6), (3, 30), (40, 2)]:
            Dg, Ig, Tg = hip.alloc(world * nq * k * 4), hip.alloc(world * nq * k * 8), hip.alloc(world * nq * k * 8)
            for r, p in enumerate(parts):
                p.search_device(xq, nq, k, n_probe, Dg + r * nq * k * 4, Ig + r * nq * k * 8, Tg + r * nq * k * 8)
                if p.num_vectors:
                    assert p.last_stats()["rank_int8"] == 1, (r, p.last_stats())
            Dm, Im = hip.alloc(nq * k * 4), hip.alloc(nq * k * 8)
            _native.check(_native.lib().vi_merge_partials_device(0, nq, k, world, Dg, Ig, Tg, Dm, Im))
            rc, Do, Io = orc.search_batch(Q, k, n_probe)
            assert rc == O.ORC_OK
            assert (hip.download(Im, (nq, k), np.int64) == Io).all(), (k, n_probe)
            assert (bits(hip.download(Dm, (nq, k), np.float32)) == bits(Do)).all(), (k, n_probe)
    finally:
        hip.close()


@pytest.mark.parametrize("d,n", [(128, 16000), (48, 12000)])
def test_int8_rank_in_groups_of_256(d, n, tmp_path, monkeypatch):
    """VI_STREAM_GQ=256: rank_stream_i8_kernel<NC, 8>.  Groups of 256 are formed once the handle has seen that its batches'
    queries are bf16-exact, so the first batch of a shape still runs groups of 128 and the later ones run groups of 256"""
    monkeypatch.setenv("VI_STREAM_GQ", "256")
    rng = np.random.default_rng(256 + d)
    X = descriptors(rng, n, d)
    orc, gpu = build(tmp_path, X)
    Q = queries(rng, X, 1800)   # 220-254 lists: over 200 queries per list at n_probe 32, groups past 128 queries
    for batch, (k, n_probe) in enumerate([(10, 32), (10, 32), (100, 32), (1, 64)]):
        check(orc, gpu, Q, k, n_probe, 1)
        if batch:
            st = gpu.last_stats()
            assert st["rank_int8"] == 1 and st["group_queries"] == 256, (batch, st)
