"""GPU: the five query-side exact sweeps where a workgroup walks MORE THAN ONE block — flat_sweep_kernel,
flat_range_sweep_kernel, flat_ip_sweep_kernel, flat_ip_range_sweep_kernel and the ladder's flat_ip_seed_kernel.

With up to 300 queries over about 30 blocks the automatic grid gives every block a workgroup of its own, so the other
files never take a block-to-block transition: the double-buffer parity, the second norm row, the accumulators' restart at
a block's first slab, the carried live word and the prefetch of the next block's.  Here VI_EXACT_BLOCK_SPLITS (read on
every call, so monkeypatch.setenv reaches the library) caps the splits: 1 is one workgroup per query tile walking every
block in storage order — through the 1-record block, from the 64-record list into the 65-record one — 2 and 3 are
strided walks of both parities.  One test leaves the variable unset and makes the walk with enough queries instead.

The indexes, references and comparisons are those of the files the helpers come from: test_exact_search_gpu.py's Case
(the sequential numpy-f32 chain over the index's own export(), np.lexsort with ties to the lower ordinal),
test_exact_ip_gpu.py's Ip, the expect / run / same of the two range files, test_exact_ip_seed_gpu.py's check_schedule.
Every comparison is for equality: uint32 views, ids, ordinals, counts, lims, padding."""
import numpy as np
import pytest

import test_exact_ip_range_gpu as ipr
import test_exact_range_gpu as l2r
from test_exact_ip_gpu import ip_of
from test_exact_ip_seed_gpu import check_schedule
from test_exact_search_gpu import Case, case, make_rows  # noqa: F401  (case: the fixture that shares the indexes)

pytestmark = pytest.mark.gpu

ENV = "VI_EXACT_BLOCK_SPLITS"
U64_MAX = np.uint64((1 << 64) - 1)
CALLS = ["knn", "range", "ip", "ip_range", "ladder"]
ROUNDS = {"knn": 2, "range": 4, "ip": 4, "ip_range": 4}   # workgroups per CU the automatic grid aims at
STATS = {"knn": "exact_stats", "range": "exact_range_stats", "ip": "exact_ip_stats", "ip_range": "exact_ip_range_stats"}

_wants = {}   # (call, case key, nq, k, filter name) -> what the call must return: made once, shared by the caps


def nblocks_of(c):
    return int(((c.lens + 63) // 64).sum())


def kth(values, nq, k, admitted, largest):
    """each query's k-th smallest (largest) value among the admitted rows, or the last there is: its own threshold"""
    v = values[:nq] if admitted is None else values[:nq][:, admitted]
    v = np.sort(-v if largest else v, axis=1)[:, min(k, v.shape[1]) - 1]
    return (-v if largest else v).copy()


def walk(call, c, ip, key, nq, k, flt=None, admitted=None, name=None):
    """one call of `call` on queries [0, nq) against its reference; range thresholds: each query's own 10th value.
    Returns the ordinals of everything returned."""
    wkey = (call, key, nq, k, name)
    if call == "knn":
        D, I, R = c.idx.search_exact_sync(c.Q[:nq], k, filter=flt, with_ordinals=True)
        if wkey not in _wants:
            _wants[wkey] = c.expect(nq, k, admitted)
        eD, eI, eR, _ = _wants[wkey]
        assert (D.view(np.uint32) == eD).all() and (I == eI).all() and (R == eR).all()
        return R[R != U64_MAX]
    if call == "range":
        if wkey not in _wants:
            radii = kth(c.distances(nq).view(np.float32), nq, 10, admitted, largest=False)
            _wants[wkey] = (radii, l2r.expect(c, nq, radii, admitted))
        radii, want = _wants[wkey]
        got = l2r.run(c, nq, 123.0, filter=flt, radii=radii)      # (the scalar is ignored)
        l2r.same(got, want)
        assert (np.diff(got[0]) >= min(10, len(c.X) if admitted is None else int(admitted.sum()))).all()
        return got[3]
    if call == "ip_range":
        if wkey not in _wants:
            t = kth(ip.S, nq, 10, admitted, largest=True)
            _wants[wkey] = (t, ipr.expect(ip, nq, t, admitted))
        t, want = _wants[wkey]
        got = ipr.run(ip, nq, float("-inf"), filter=flt, min_scores=t)   # (the scalar would return everything)
        ipr.same(got, want)
        assert (np.diff(got[0]) >= min(10, len(ip.X) if admitted is None else int(admitted.sum()))).all()
        return got[3]
    # ip: the final sweep behind the ladder at the default cand_cap; ladder: cand_cap 64, several sampled levels
    opts = {"cand_cap": 64} if call == "ladder" else None
    S, I, R = ip.idx.search_exact_ip_sync(ip.Q[:nq], k, filter=flt, opts=opts, with_ordinals=True)
    if ("ip", key, nq, k, name) not in _wants:     # (one reference for both forms)
        _wants["ip", key, nq, k, name] = ip.expect(nq, k, admitted)
    eS, eI, eR, _ = _wants["ip", key, nq, k, name]
    assert (S.view(np.uint32) == eS).all() and (I == eI).all() and (R == eR).all()
    st = check_schedule(ip.idx, max(64, k) if call == "ladder" else max(8 * k, 1024), k)
    assert call != "ladder" or st["levels"] >= 2
    return R[R != U64_MAX]


# the shapes of the one-block files that reach a chunk tail, the resident limit, data without a lo plane, centred images
# and the streaming form with an odd slab count (144: 9 chunks, 5 slabs of 2) — and two that are new: 132, streaming with
# a partial last chunk, and 192, six slabs, where every block of a walk begins in buffer 0
SHAPES = [("gauss", 20, 129, 10), ("gauss", 128, 300, 128), ("sift", 128, 129, 10), ("offset", 128, 129, 10),
          ("gauss", 144, 129, 10), ("gauss", 132, 129, 10), ("gauss", 192, 129, 10)]


@pytest.mark.parametrize("kind,dim,nq,k", SHAPES)
@pytest.mark.parametrize("cap", [1, 2, 3])
@pytest.mark.parametrize("call", CALLS)
def test_walks_under_the_cap(case, monkeypatch, call, cap, kind, dim, nq, k):
    c = case(kind, dim)
    ip = ip_of(c, (kind, dim))
    assert nblocks_of(c) > 2 * cap and {1, 64, 65} <= set(c.lens.tolist())
    monkeypatch.setenv(ENV, str(cap))
    walk(call, c, ip, (kind, dim), nq, k)
    if call in STATS:
        assert getattr(c.idx, STATS[call])()["block_splits"] == min(cap, nblocks_of(c))


@pytest.mark.parametrize("value", ["", "0", "x", "2x", "-2"])
def test_a_value_that_is_no_cap_leaves_the_automatic_grid(case, monkeypatch, value):
    c = case("gauss", 20)
    monkeypatch.delenv(ENV, raising=False)
    walk("knn", c, None, ("gauss", 20), 129, 10)
    automatic = c.idx.exact_stats()["block_splits"]
    monkeypatch.setenv(ENV, value)
    walk("knn", c, None, ("gauss", 20), 129, 10)
    assert c.idx.exact_stats()["block_splits"] == automatic > 3


def filters_of(c):
    """name -> mask over the exported rows.  blocks: a record is admitted iff (its position in its list // 64) is even,
    so live and dead blocks alternate inside every long list"""
    where = c.idx.export()[3]
    return {"five": np.isin(c.ext, c.ext[[0, 70, 500, 900, len(c.ext) - 1]]), "every_other": np.isin(c.ext, c.ext[::2]),
            "blocks": ((where & np.uint64(0xFFFFFFFF)) // np.uint64(64)) % np.uint64(2) == 0}


@pytest.mark.parametrize("dim", [20, 128])
@pytest.mark.parametrize("name", ["five", "every_other", "blocks"])
@pytest.mark.parametrize("call", CALLS)
def test_filters_under_the_walk(case, monkeypatch, call, name, dim):
    """a live word, an allow word or a norm row that lags one block behind admits a dead block's records here, or
    drops a live one's"""
    c = case("gauss", dim)
    admitted = filters_of(c)[name]
    assert 0 < admitted.sum() < len(admitted)
    monkeypatch.setenv(ENV, "1")
    R = walk(call, c, ip_of(c, ("gauss", dim)), ("gauss", dim), 129, 10, flt=c.idx.filter_ids(c.ext[admitted]),
             admitted=admitted, name=name)
    assert len(R) and admitted[R.astype(np.int64)].all()
    if call in STATS:
        assert getattr(c.idx, STATS[call])()["block_splits"] == 1


_wide = {}


def wide_case(c, nq):
    """the gauss-20 index under nq fresh queries: a Case over them, made once"""
    if nq not in _wide:
        w = Case.__new__(Case)
        w.idx, w.ext, w.X, w.lens, w.Q, w._dist = c.idx, c.ext, c.X, c.lens, make_rows("gauss", nq, 20, 9), {}
        _wide[nq] = w
    return _wide[nq]


@pytest.mark.parametrize("call", list(STATS))
def test_the_automatic_grid_walks_when_the_queries_fill_the_device(case, monkeypatch, call):
    """the variable unset: so many query tiles that the host's own choice gives a workgroup at least two blocks"""
    import torch
    c = case("gauss", 20)
    cus, nb = torch.cuda.get_device_properties(0).multi_processor_count, nblocks_of(c)
    nq = 128 * -(-ROUNDS[call] * cus // (nb // 2))
    assert nq <= 16384, f"{cus} CUs and {nb} blocks want {nq} queries: this test needs a larger index"
    monkeypatch.delenv(ENV, raising=False)
    w = wide_case(c, 128 * -(-max(ROUNDS.values()) * cus // (nb // 2)))
    walk(call, w, ip_of(w, ("gauss", 20, "wide")) if call.startswith("ip") else None, ("gauss", 20, "wide"), nq, 10)
    splits = getattr(c.idx, STATS[call])()["block_splits"]
    assert 1 <= splits and 2 * splits <= nb, (splits, nb)


@pytest.mark.parametrize("cap", [None, 1])
@pytest.mark.parametrize("call", ["knn", "ip"])
def test_the_dimension_limit(case, monkeypatch, call, cap):
    """dim 1536: 96 chunks, 48 slabs a block"""
    c = case("gauss", 1536)
    ip = ip_of(c, ("gauss", 1536, 129), lambda Q: Q[:129]) if call == "ip" else None
    if cap is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, str(cap))
    walk(call, c, ip, ("gauss", 1536), 129, 10)
    assert cap is None or getattr(c.idx, STATS[call])()["block_splits"] == cap
