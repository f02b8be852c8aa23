"""GPU: the score-seeded ladder in front of the exact inner-product search's final sweep (flat_ip_seed.hip).

The ladder may only raise a query's bound, so every result stays what test_exact_ip_gpu.py checks: the numpy float32 chain
over the index's own export(), compared for equality of uint32 views, ids, ordinals and counts (its Ip).  What is new is
checked through exact_ip_seed_stats(): the number of levels the documented schedule gives for the index's block count,
strides that are decreasing powers of the ratio, rows tightened, and no row of a norm-spread index on the overflow path."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vector_indexer_py as vip
from test_exact_ip_gpu import Ip, ip_of, zero_one
from test_exact_search_gpu import NLIST, case, make_rows  # noqa: F401  (case: the fixture that shares the indexes)

pytestmark = pytest.mark.gpu


def schedule(where, cap, k):
    """(ratio, strides) of flat_ip_seed.hip's header for an index whose export gave `where`: r the largest power of two
    <= cap / (2 k) in [2, 4]; strides r^m .. r with m the smallest whose sample ceil(blocks / r^m) * 64 fits cap (or is one block); at most 8"""
    lens = np.bincount((where >> np.uint64(32)).astype(np.int64))
    nblocks = int(((lens + 63) // 64).sum())
    r = 4 if cap // (2 * k) >= 4 else 2
    if nblocks * 64 <= cap:
        return r, []
    strides = [r]
    while strides[-1] < nblocks and -(-nblocks // strides[-1]) * 64 > cap:
        strides.append(strides[-1] * r)
    return r, strides[::-1][-8:]


def check_schedule(idx, cap, k):
    st = idx.exact_ip_seed_stats()
    r, strides = schedule(idx.export()[3], cap, k)
    assert st["ratio"] == r and st["levels"] == len(strides) >= 1 and st["strides"] == strides, (st, strides)
    return st


# default cand_cap (1024): one level; cand_cap 64: several, and levels that meet more than 64 scores; sift: no lo plane;
# 144: the streaming form; offset: centred images against the uncentred query
@pytest.mark.parametrize("kind,dim,nq,k,cap", [("gauss", 20, 129, 10, None), ("gauss", 128, 300, 128, None), ("sift", 128, 129, 10, 64),
                                               ("gauss", 144, 129, 10, 64), ("offset", 128, 129, 4, 64)])
def test_results_are_unchanged_and_the_levels_are_the_documented_schedule(case, kind, dim, nq, k, cap):
    c = case(kind, dim)
    ip_of(c, (kind, dim)).check(nq, k, opts=None if cap is None else {"cand_cap": cap})
    st = check_schedule(c.idx, cap or max(8 * k, 1024), k)
    assert sum(st["level_survivors"]) >= sum(st["level_candidates"]) > 0


def test_rows_of_spread_norms_stay_off_the_overflow_path(tmp_path):
    """one level of stride 4: replayed on the CPU (any order of the lists, a fifth of the rows moved to other lists) it leaves
    at most 108 candidates per query of this seed to the final sweep and meets at most 533 scores: far from 1024"""
    X = make_rows("gauss", 2000, 20, 3) * np.random.default_rng(5).choice(np.float32([0.25, 1.0, 4.0]), size=(2000, 1))
    idx = vip.build(X, str(tmp_path), nlist=NLIST, now_secs=1_700_000_000)
    ext, Xe, _, _ = idx.export()
    Ip(idx, ext, Xe, make_rows("gauss", 33, 20, 4)).check(33, 10)
    assert check_schedule(idx, 1024, 10)["rows_tightened"] > 0 and idx.exact_ip_stats()["overflow_rows"] == 0


def test_filters_in_both_forms(case):
    c = case("gauss", 20)
    ip = ip_of(c, ("gauss", 20))
    five = c.ext[[0, 70, 500, 900, len(c.ext) - 1]]
    ip.check(129, 10, filter=c.idx.filter_ids(five), admitted=np.isin(c.ext, five))   # no level finds 10: padded rows
    assert c.idx.exact_ip_seed_stats()["rows_tightened"] == 0
    ip.check(129, 10, filter=c.idx.filter_ids(c.ext[::2]), admitted=np.isin(c.ext, c.ext[::2]))
    from hiprt import Hip
    hip = Hip()
    try:
        xq, S, I, R, n = hip.upload(ip.Q[:129].copy()), hip.alloc(1290 * 4), hip.alloc(1290 * 8), hip.alloc(1290 * 8), hip.alloc(129 * 8)
        for ids in (five, c.ext[::2]):
            c.idx.search_exact_ip_device(xq, 129, 10, S, I, R, n, filter=c.idx.filter_ids(ids))
            got = (hip.download(S, (129, 10), np.uint32), hip.download(I, (129, 10), np.int64),
                   hip.download(R, (129, 10), np.uint64), hip.download(n, (129,), np.uint64))
            for g, e in zip(got, ip.expect(129, 10, np.isin(c.ext, ids))):
                assert (g == e).all()
    finally:
        hip.close()


@pytest.mark.parametrize("name,transform", [("neg", lambda Q: -Q), ("zero", zero_one)])
def test_negated_and_zero_queries_at_a_small_cap(case, name, transform):
    ip = ip_of(case("gauss", 128), ("gauss", 128, name), transform)
    ip.check(129, 10, opts={"cand_cap": 64})
    check_schedule(ip.idx, 64, 10)
    if name == "zero":
        assert ip.idx.exact_ip_stats()["overflow_rows"] >= 1


def test_the_switch_skips_the_ladder_and_changes_no_row(tmp_path):
    Q = make_rows("gauss", 33, 20, 4)
    np.savez(tmp_path / "in.npz", X=make_rows("gauss", 1500, 20, 3), Q=Q)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "exact_ip_ladder_child.py")
    subprocess.run([sys.executable, child, str(tmp_path / "work"), str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                   check=True, timeout=300, env=dict(os.environ, VI_EXACT_IP_LADDER="0"))
    got = np.load(tmp_path / "out.npz")
    eS, eI, eR, _ = Ip(None, got["ext"], got["X"], Q).expect(33, 10)
    assert (got["S"].view(np.uint32) == eS).all() and (got["I"] == eI).all() and (got["R"] == eR).all() and got["levels"] == 0
