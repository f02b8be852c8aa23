"""GPU: merging per-rank radius results on the device — vi_range_merge_device, vector_indexer_py.merge_range_results, and the
radius closures of distributed.gpu_searcher.

The contract: the merged result of the ranks of a partitioned index equals the unpartitioned handle's radius result in lims,
ids, distance bits and tie keys, which in turn equals the oracle's (test_range_search_gpu.expected).  The kernel itself is
checked on synthetic CSR parts against np.lexsort, bit for bit: keys from a small pool (equal distances and equal keys in
two parts are common), tie keys with bit 63 set, ids past 2^63, empty rows and parts, 64 parts, and rows far longer than a
workgroup."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import range_merge_cases as RC
import vector_indexer_py as vip
from range_merge_cases import bits
from test_filtered_search_gpu import HALF, TENTH, Fixture, base  # noqa: F401
from test_range_search_gpu import expected
from vector_indexer_py import _native as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hip():
    from hiprt import Hip
    h = Hip()
    yield h
    h.close()


def download(hip, res):
    lims = hip.download(res.lims_ptr, (res.nq + 1,), np.uint64)
    assert int(lims[-1]) == res.total
    return (lims, hip.download(res.D_ptr, (res.total,), np.float32), hip.download(res.I_ptr, (res.total,), np.int64),
            hip.download(res.tie_ptr, (res.total,), np.uint64))


# ---- synthetic parts: the kernel test -------------------------------------------------------------------------------------
POOL = np.array([0.0, 0.25, 1.0, 1.5, 2.0, 7.0, 3.0e38, np.inf], dtype=np.float32)
TIES = np.array([0, 1, 2, (3 << 32) | 5, 1 << 63, (1 << 63) + 1, (1 << 64) - 1], dtype=np.uint64)


def make_part(rng, counts, sort=True):
    """one CSR part with the given per-query counts, every row sorted by (distance bits, tie)"""
    counts = np.asarray(counts, dtype=np.int64)
    lims = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n = int(lims[-1])
    D, T = POOL[rng.integers(0, POOL.size, n)], TIES[rng.integers(0, TIES.size, n)]
    I = rng.integers(0, 1 << 64, size=n, dtype=np.uint64).view(np.int64)
    if sort:
        order = np.lexsort((T, bits(D), np.repeat(np.arange(counts.size), counts)))
        D, T = D[order], T[order]
    return lims, np.ascontiguousarray(D), I, np.ascontiguousarray(T)


def lexsort_merge(parts):
    """the rule: per query the union of the rows under a stable sort by (distance bits, tie), parts concatenated in order"""
    nq = parts[0][0].size - 1
    row = np.concatenate([np.repeat(np.arange(nq), np.diff(p[0].astype(np.int64))) for p in parts])
    D, I, T = (np.concatenate([p[c] for p in parts]) for c in (1, 2, 3))
    order = np.lexsort((T, bits(D), row))
    lims = np.sum([p[0] for p in parts], axis=0).astype(np.uint64)
    return lims, D[order], I[order], T[order]


def gpu_merge(hip, parts, nq):
    cols = [[hip.upload(p[c]) for p in parts] for c in range(4)]      # (an empty array still gets a buffer)
    return vip.merge_range_results_device(0, nq, *cols)


def spread(rng, total, nq):
    """`total` entries over nq queries, many of them empty"""
    return np.bincount(rng.integers(0, nq, total) // 2 * 2 % nq, minlength=nq) if nq > 1 else np.array([total])


def skewed(rng, parts, nq, total, heavy):
    """one query owns 90 % of `total`, split unevenly over the parts"""
    share = rng.dirichlet(np.ones(parts))
    out = []
    for p in range(parts):
        c = spread(rng, int(total * 0.1 / parts), nq)
        c[heavy] = int(total * 0.9 * share[p])
        out.append(c)
    return out


def synthetic(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "general_3x257":
        return 257, [spread(rng, 4000, 257) for _ in range(3)]
    if name == "one_part_one_query":
        return 1, [np.array([300])]
    if name == "64_parts":
        return 5, [rng.integers(0, 40, 5) * (rng.random(5) < 0.7) for _ in range(64)]
    if name == "nothing_at_all":
        return 7, [np.zeros(7, np.int64) for _ in range(2)]
    if name == "an_empty_part":
        return 33, [spread(rng, 900, 33), np.zeros(33, np.int64), spread(rng, 700, 33)]
    if name == "one_query_owns_most":
        return 50, skewed(rng, 4, 50, 200_000, 17)
    if name == "one_query_two_parts":
        return 1, [np.array([41_000]), np.array([29_000])]
    raise KeyError(name)


SYNTHETIC = ["general_3x257", "one_part_one_query", "64_parts", "nothing_at_all", "an_empty_part", "one_query_owns_most",
             "one_query_two_parts"]


@pytest.mark.parametrize("name", SYNTHETIC)
def test_synthetic_parts_against_lexsort(hip, name):
    nq, counts = synthetic(name)
    rng = np.random.default_rng(len(name))
    parts = [make_part(rng, c) for c in counts]
    want = lexsort_merge(parts)
    total = int(want[0][-1])
    assert total == sum(int(p[0][-1]) for p in parts)
    if name == "one_query_owns_most":
        assert 190_000 < total <= 200_000 and int(want[0][18] - want[0][17]) > 0.85 * total
    if name == "one_query_two_parts":
        assert total == 70_000
    if name == "nothing_at_all":
        assert total == 0
    res = gpu_merge(hip, parts, nq)
    assert res.total == total and res.nq == nq
    got = download(hip, res)
    RC.same(got, want)
    lims, D, I = res.copy()                                     # the host copy of a result that belongs to no index
    assert np.array_equal(lims, want[0]) and np.array_equal(bits(D), bits(want[1])) and np.array_equal(I, want[2])
    res.free()


def test_equal_keys_in_two_parts_come_out_lower_part_first(hip):
    """the same rank passed twice (a caller error): still a permutation of the union, every key's copies in part order"""
    rng = np.random.default_rng(5)
    lims, D, _, T = make_part(rng, spread(rng, 3000, 40))
    n = D.size
    parts = [(lims, D, np.arange(n, dtype=np.int64) + p * n, T) for p in range(3)]
    res = gpu_merge(hip, parts, 40)
    got = download(hip, res)
    RC.same(got, lexsort_merge(parts))
    assert np.array_equal(np.sort(got[2]), np.arange(3 * n))                                  # a permutation
    row = np.repeat(np.arange(40), np.diff(got[0].astype(np.int64)))
    same_key = (row[1:] == row[:-1]) & (bits(got[1])[1:] == bits(got[1])[:-1]) & (got[3][1:] == got[3][:-1])
    part = got[2] // n
    assert same_key.any() and (np.diff(part)[same_key] >= 0).all()                            # lower part first
    res.free()


def test_no_query(hip):
    res = gpu_merge(hip, [make_part(np.random.default_rng(0), np.zeros(0, np.int64)) for _ in range(2)], 0)
    assert res.total == 0 and res.nq == 0
    assert hip.download(res.lims_ptr, (1,), np.uint64).tolist() == [0]
    assert res.copy()[0].tolist() == [0]
    res.free()


# ---- the tie fixture: in-process ranks against the unpartitioned handle and the oracle ------------------------------------------
@pytest.fixture(scope="module")
def tie(tmp_path_factory):
    X, Q = RC.tie_data()
    return Fixture(tmp_path_factory.mktemp("tie"), X, RC.NLIST, Q)


class Ranks:
    """the partitioned handles of one fixture, loaded once per (world, placement)"""

    def __init__(self, fx):
        self.fx, self.loaded = fx, {}

    def __call__(self, world, placement):
        if (world, placement) not in self.loaded:
            fx = self.fx
            parts = [vip.load(fx.idx, fx.sh, fx.dim, rank=r, world_size=world, placement=placement) for r in range(world)]
            assert sum(p.num_vectors for p in parts) == fx.n
            self.loaded[world, placement] = parts
        return self.loaded[world, placement]


@pytest.fixture(scope="module")
def tie_ranks(tie):
    return Ranks(tie)


@pytest.fixture(scope="module")
def tie_whole(tie, hip):
    """the unpartitioned handle's own device result per (n_probe, radius), computed once"""
    xq, memo = hip.upload(tie.Q), {}

    def whole(n_probe, r):
        if (n_probe, r) not in memo:
            res = tie.gpu.range_search_device(xq, tie.Q.shape[0], r, n_probe)
            memo[n_probe, r] = download(hip, res)
            res.free()
        return memo[n_probe, r]
    whole.xq = xq
    return whole


@pytest.mark.parametrize("n_probe", RC.PROBES)
@pytest.mark.parametrize("placement", [0, 1])
@pytest.mark.parametrize("world", RC.WORLDS)
def test_tie_fixture_ranks_merge_to_the_unpartitioned_result(tie, tie_ranks, tie_whole, hip, world, placement, n_probe):
    nq = tie.Q.shape[0]
    Df, If, _ = tie.full(n_probe)
    radii = dict(RC.radii(Df, If), negative=-1.0, zero=0.0)
    ranks = tie_ranks(world, placement)
    for name, r in radii.items():
        results = [p.range_search_device(tie_whole.xq, nq, r, n_probe) for p in ranks]
        merged = vip.merge_range_results(0, results)
        got = download(hip, merged)
        if placement == 0 and name in ("r10", "r100", "inf"):      # the fixture is not degenerate
            parts = [download(hip, x) for x in results]
            assert all(x.total > 0 for x in results), (name, [x.total for x in results])
            assert RC.queries_with_cross_rank_ties(parts) >= nq // 2
            if name == "r10" and world >= 4:
                assert RC.empty_rows(parts) > 0
        for x in results:
            x.free()
        RC.same(got, tie_whole(n_probe, r))                                    # lims, ids, distance bits and tie keys
        lims_e, De, Ie, _ = expected(tie, r, nq, n_probe)
        RC.same(got, (lims_e, De, Ie), tie=False)                              # ... and the oracle's
        assert (int(lims_e[-1]) == 0) == (name == "negative")
        merged.free()


# ---- filters: every rank makes its own from the same predicate ---------------------------------------------------------------
@pytest.fixture(scope="module")
def base_ranks(base):
    return Ranks(base)


def predicates(fx):
    ids = fx.ext[np.random.default_rng(9).permutation(fx.n)[: fx.n // 3]]
    return {"window": lambda ix: ix.filter_timestamps(*HALF), "ids": lambda ix: ix.filter_ids(ids),
            "both": lambda ix: ix.filter_timestamps(*HALF) & ix.filter_ids(ids)}


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("which", ["window", "ids", "both"])
def test_filtered_ranks_merge_to_the_unpartitioned_filtered_result(base, base_ranks, hip, which, world):
    nq, p, k = 300, 8, 20
    make = predicates(base)[which]
    ranks = base_ranks(world, 0)
    whole_f, rank_f = make(base.gpu), [make(x) for x in ranks]
    assert 0 < whole_f.num_allowed < base.n and sum(f.num_allowed for f in rank_f) == whole_f.num_allowed
    xq = hip.upload(base.Q)
    Df, If, _ = base.full(p)
    # radius
    for r in (RC.median_kth(Df, If, 100), RC.INF):
        res = base.gpu.range_search_device(xq, nq, r, p, filter=whole_f)
        want = download(hip, res)
        res.free()
        assert 0 < int(want[0][-1]) < int(expected(base, r, nq, p)[0][-1])     # the filter does thin the result
        results = [x.range_search_device(xq, nq, r, p, filter=f) for x, f in zip(ranks, rank_f)]
        merged = vip.merge_range_results(0, results)
        RC.same(download(hip, merged), want)
        for x in results + [merged]:
            x.free()
    # top-k: per-rank filtered searches merged by vi_merge_partials_device
    Dp, Ip, Tp = hip.alloc(world * nq * k * 4), hip.alloc(world * nq * k * 8), hip.alloc(world * nq * k * 8)
    Dm, Im = hip.alloc(nq * k * 4), hip.alloc(nq * k * 8)
    for i, (x, f) in enumerate(zip(ranks, rank_f)):
        x.search_device(xq, nq, k, p, Dp + i * nq * k * 4, Ip + i * nq * k * 8, Tp + i * nq * k * 8, filter=f)
    N.check(N.lib().vi_merge_partials_device(0, nq, k, world, Dp, Ip, Tp, Dm, Im))
    De, Ie = base.gpu.search_sync(base.Q, k, p, filter=whole_f)
    assert np.array_equal(hip.download(Im, (nq, k), np.int64), Ie)
    assert np.array_equal(bits(hip.download(Dm, (nq, k), np.float32)), bits(De))


# ---- lifetime -------------------------------------------------------------------------------------------------------------------
def test_the_merged_result_outlives_its_parts_and_their_indexers(tie, tie_whole, hip):
    nq, p = tie.Q.shape[0], 3
    Df, If, _ = tie.full(p)
    r = RC.radii(Df, If)["r100"]
    ranks = [vip.load(tie.idx, tie.sh, tie.dim, rank=i, world_size=2) for i in range(2)]
    results = [x.range_search_device(tie_whole.xq, nq, r, p) for x in ranks]
    merged = vip.merge_range_results(0, results)
    for x in results:
        x.free()
    del results, ranks, x
    gc.collect()                                                # the indexers are gone
    for _ in range(8):                                          # (whatever they freed is handed out again and overwritten)
        hip.upload(np.full(1 << 16, 0xAB, dtype=np.uint8))
    lims_e, De, Ie, _ = expected(tie, r, nq, p)
    assert merged.total == int(lims_e[-1]) > 0
    RC.same(download(hip, merged), tie_whole(p, r))
    lims, D, I = merged.copy()
    RC.same((lims, D, I), (lims_e, De, Ie), tie=False)
    with pytest.raises(vip.ViError) as e:
        merged.copy(include_vectors=True)
    assert e.value.kind == "InvalidInput"
    V = np.zeros((merged.total, tie.dim), dtype=np.float32)                            # ... and through the C entry itself
    assert N.lib().vi_range_result_copy(merged._h, None, None, None, N.ptr(V)) == N.VI_ERR_INVALID_INPUT and N.lib().vi_last_error()
    merged.free()
    assert merged.D_ptr == 0


# ---- the closures of distributed.gpu_searcher -------------------------------------------------------------------------------------
def test_gpu_searcher_closures_with_in_process_ranks(tie, tmp_path):
    """torch has to initialise its HIP runtime before the library does, which a pytest process cannot arrange: the closures
    run in a child (range_merge_closures_child.py); here its merged results are compared with the oracle's"""
    nq, p, world = tie.Q.shape[0], 3, 4
    Df, If, _ = tie.full(p)
    radii = dict(RC.radii(Df, If), negative=-1.0)
    np.savez(tmp_path / "in.npz", Q=tie.Q, names=np.array(list(radii)), radii=np.array(list(radii.values()), dtype=np.float64),
             window=np.array(TENTH, dtype=np.uint64))
    out = tmp_path / "out.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "range_merge_closures_child.py"), tie.idx, tie.sh, str(tie.dim),
                    str(world), str(p), str(tmp_path / "in.npz"), str(out)], check=True, timeout=300)
    got = np.load(out)
    for name, r in radii.items():
        lims_e, De, Ie, _ = expected(tie, r, nq, p)
        RC.same((got[f"lims_{name}"].view(np.uint64), got[f"D_{name}"], got[f"I_{name}"]), (lims_e, De, Ie), tie=False)
        assert got[f"T_{name}"].shape == Ie.shape
    lims_e, De, Ie, _ = expected(tie, radii["r100"], nq, p, window=TENTH)          # filter= through local_range_search
    assert 0 < int(lims_e[-1])
    RC.same((got["lims_f"].view(np.uint64), got["D_f"], got["I_f"]), (lims_e, De, Ie), tie=False)
    De, Ie, _ = tie.expected(TENTH, nq, 10, p)                                      # filter= through local_search
    assert np.array_equal(got["I_k"], Ie) and np.array_equal(bits(got["D_k"]), bits(De))
