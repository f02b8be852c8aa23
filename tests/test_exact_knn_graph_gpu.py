"""GPU: the exact k-NN graph of the stored records — vi_indexer_knn_graph_exact, host and device form.

The indexes are those of test_exact_search_gpu.py (its Case: lists of 0 / 1 / 64 / 65 and over 128 records).  The reference
is numpy on the export's rows: the reference's sequential f32 chain for every ORDERED pair (pair_bits of
test_exact_join_gpu.py), np.lexsort by (bits, ordinal) over the participants, the row's own ordinal removed when excluded,
the first k, padded.  Every comparison is for equality: uint32 views of D, ids, ordinals, counts."""
import numpy as np
import pytest

import vector_indexer_py as vip
from hiprt import Hip
from test_exact_join_gpu import pair_bits
from test_exact_search_gpu import NLIST, case, make_rows  # noqa: F401  (case: the fixture that shares the indexes)

pytestmark = pytest.mark.gpu
INF_BITS, U64_MAX = np.float32(np.inf).view(np.uint32), np.uint64((1 << 64) - 1)


def expect(c, k, exclude_self=True, admitted=None):
    """(D bits, I, ord, counts) the call must return; the sorted rows are kept on the case per (exclusion, filter)"""
    bits, n = pair_bits(c), len(c.X)
    tag = ("_knn", exclude_self, None if admitted is None else admitted.tobytes())
    if tag not in c.__dict__.setdefault("_knn_rows", {}):
        adm = np.ones(n, dtype=bool) if admitted is None else admitted
        far = bits.astype(np.uint64)
        far[~(adm[:, None] & adm[None, :])] = 1 << 40     # no participant: behind every distance
        if exclude_self:
            far[np.arange(n), np.arange(n)] = 1 << 40
        order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), far), axis=1)
        c._knn_rows[tag] = (order, (np.take_along_axis(far, order, axis=1) < (1 << 40)).sum(axis=1))
    order, avail = c._knn_rows[tag]
    counts = np.minimum(avail, k).astype(np.uint64)
    top = order[:, :k]
    real = np.arange(k)[None, :] < counts[:, None]
    D = np.where(real, np.take_along_axis(bits, top, axis=1), INF_BITS)
    I, R = np.where(real, c.ext[top].astype(np.int64), -1), np.where(real, top.astype(np.uint64), U64_MAX)
    return D, I, R, counts


def check(c, k, exclude_self=True, filter=None, admitted=None, opts=None):
    D, I, R, counts = c.idx.knn_graph_exact(k, exclude_self=exclude_self, filter=filter, opts=opts, with_ord=True)
    want = expect(c, k, exclude_self, admitted)
    for g, w in zip((D.view(np.uint32), I, R, counts), want):
        assert g.shape == w.shape and (g == w).all()
    return want


# dim 4 / 20: partial chunks of the image; 128: the register-resident limit; 144: the streaming form.  gauss: lo planes;
# sift: 8-bit data, no lo planes; offset: centred images.  Chunks of 192 rows start mid-block and mid-list, are no whole
# number of tiles, and the last one is a bare triangle.  k = 128 seeds 129 wide.
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("kind,dim", [("gauss", 4), ("gauss", 20), ("sift", 128), ("offset", 128), ("gauss", 144), ("sift", 144)])
def test_rows_equal_the_brute_force(case, kind, dim, k, monkeypatch):
    c = case(kind, dim)
    monkeypatch.setenv("VI_GRAPH_CHUNK", "192")
    check(c, k)
    st = c.idx.exact_knn_stats()
    assert st["rows"] == len(c.X) and st["k"] == k and st["chunk_rows"] == 192 and st["candidates"] >= len(c.X) * k
    assert st["sweeps"] == 1 or k > 10


def test_self_kept_at_the_default_chunk_and_the_device_form(case):
    c = case("gauss", 20)
    n, k = len(c.X), 10
    want = check(c, k, exclude_self=False)
    assert (want[2][:, 0] == np.arange(n)).all() and (want[0][:, 0] == 0).all()   # every row holds its own slot once, first
    hip = Hip()
    try:
        D, I, R, cnt = hip.alloc(n * k * 4), hip.alloc(n * k * 8), hip.alloc(n * k * 8), hip.alloc(n * 8)
        c.idx.knn_graph_exact_device(k, D, I, R, cnt)
        got = (hip.download(D, (n, k), np.uint32), hip.download(I, (n, k), np.int64), hip.download(R, (n, k), np.uint64),
               hip.download(cnt, (n,), np.uint64))
    finally:
        hip.close()
    for g, w in zip(got, expect(c, k)):
        assert (g == w).all()


def test_entries_only_the_other_record_wants(case):
    """(row v, neighbour u) with u before v and d(u, v) above u's own k-th distance: the pair's one visit is in u's frame,
    where nothing but v's bound lets it through — a compare against thr_u(B_u) alone loses these"""
    c = case("gauss", 20)
    D, _, R, _ = expect(c, 10)
    kth, u = D[:, 9], R.astype(np.int64)
    one_sided = (u < np.arange(len(c.X))[:, None]) & (D > kth[u])
    assert one_sided.sum() > 0
    check(c, 10)


@pytest.mark.parametrize("exclude_self", [True, False])
def test_every_vector_twice_keeps_the_copy_not_the_slot(tmp_path, exclude_self):
    X = make_rows("gauss", 700, 20, 3)
    c = type("C", (), {})()
    c.idx = vip.build(np.concatenate([X, X]), str(tmp_path), nlist=NLIST, now_secs=1_700_000_000)
    c.ext, c.X, _, _ = c.idx.export()
    for k in (1, 3):
        D, _, R, _ = check(c, k, exclude_self=exclude_self)
        assert (D[:, 0] == 0).all()                                     # the copy is there whichever slot goes
        assert ((R[:, 0] != np.arange(1400)).all() if exclude_self else (D[:, :2] == 0).all())


def test_copies_of_one_vector_are_cut_by_ordinal_after_a_second_sweep(tmp_path):
    X = make_rows("gauss", 700, 20, 3)
    c = type("C", (), {})()
    c.idx = vip.build(np.concatenate([X, np.repeat(X[:1], 600, axis=0)]), str(tmp_path), nlist=NLIST, now_secs=1_700_000_000)
    c.ext, c.X, _, _ = c.idx.export()
    D, _, R, _ = check(c, 3, opts={"pool_cap": 64})
    st = c.idx.exact_knn_stats()
    assert st["sweeps"] == 2 and st["pool_cap"] == st["candidates"] >= 601 * 600
    copies = np.flatnonzero((c.X == X[0]).all(axis=1))
    assert len(copies) == 601 and (D[copies] == 0).all() and (R[copies[5]] == copies[:3].astype(np.uint64)).all()


def test_filters_pad_the_rows_and_empty_those_of_the_rest(case, monkeypatch):
    c = case("gauss", 20)
    monkeypatch.setenv("VI_GRAPH_CHUNK", "192")
    five = c.ext[[0, 70, 500, 900, len(c.ext) - 1]]
    for ids, exclude_self in ((five, True), (five, False), (c.ext[::2], True)):
        admitted = np.isin(c.ext, ids)
        _, I, _, counts = check(c, 10, exclude_self=exclude_self, filter=c.idx.filter_ids(ids), admitted=admitted)
        assert (counts[~admitted] == 0).all() and np.isin(I[I >= 0], ids.astype(np.int64)).all()
        if len(ids) == 5:    # every admitted row is unbounded and padded
            assert (counts[admitted] == (4 if exclude_self else 5)).all() and c.idx.exact_knn_stats()["unbounded_rows"] == 5


def test_options_never_change_a_result(case):
    c = case("gauss", 20)
    for opts in ({"seed_probe": 1}, vip.ExactKnnOpts(NLIST, 0)):
        check(c, 10, opts=opts)
        assert c.idx.exact_knn_stats()["seed_probe"] == (1 if isinstance(opts, dict) else NLIST)


def test_equals_search_exact_of_the_rows_and_the_probed_graph_at_every_list(case):
    c = case("gauss", 20)
    D, I, R, _ = c.idx.knn_graph_exact(10, exclude_self=False, with_ord=True)
    Ds, Is, Rs = c.idx.search_exact_sync(c.X, 10, with_ordinals=True)
    assert (D.view(np.uint32) == Ds.view(np.uint32)).all() and (I == Is).all() and (R == Rs).all()
    De, Ie, _ = c.idx.knn_graph_exact(10)            # gaussian rows: no equal distances among a row's nearest
    Dp, Ip = c.idx.knn_graph(10, c.idx.num_centroids)
    assert (De.view(np.uint32) == Dp.view(np.uint32)).all() and (Ie == Ip).all()
