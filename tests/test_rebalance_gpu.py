"""GPU: vi_indexer_rebalance — a refine whose first iterations split overfull lists into the empty ones, in index.bin, in
the shard files and in the resident index.

Everything expected comes from the untouched oracle (rebalance_cases.py over refine_cases.py): the case directories from
its build and writer, the plan, the seeds, the sides and the two centres of every split from its scalar distance chain and
its update_centroids, the shard files from its writer, the searches from a fresh OracleIndex.load of the directories the
handle wrote.  Centroid bits, file bytes, ids, distance bits, timestamps and counts must match exactly; nothing here has a
tolerance."""
import os

import numpy as np
import pytest

import oracle_lib as O
import rebalance_cases as B
import refine_cases as R
import vector_indexer_py as vip
from vector_indexer_py import _native as N
from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig
from vector_indexer_py.harness import FaissStyleAdapter

from remove_cases import all_bytes, assert_same, bits
from test_refine_gpu import NOW, SHAPES, check_against_oracle, copy_dirs, dir_bytes, queries, want_list_stats
from test_remove_records_gpu import device_search, host_search, twice

pytestmark = pytest.mark.gpu


class Case:
    """a case of rebalance_cases, a handle on a copy of its directories that ran the case's rule, and the replay"""

    def __init__(self, name, root):
        self.name, self.root = name, root
        self.case = B.CASES[name]
        self.rule = self.case.rule
        idx, sh, self.st, self.info = B.make_state(self.case.state, root)
        self.dim = self.st.X.shape[1]
        self.kind = R.CASES[self.case.state][1] if self.case.state in R.CASES else "lattice"
        self.src = (idx, sh)
        self.base_sh = os.path.join(root, "base", "shards")
        self.dirs = copy_dirs(self.src, root, "one")
        self.gpu = vip.load(*self.dirs, self.dim, now_secs=NOW)
        self.stats_before = self.gpu.list_stats()
        self.old_filter = self.gpu.filter_timestamps(0, 1 << 40)
        self.returned = self.gpu.rebalance(**self.rule.fields())
        self.bstats = self.gpu.rebalance_stats()
        self.out = B.replay_rule(self.st, self.rule)
        self.after = self.out.state
        self.want = R.expected_files(self.after, self.base_sh, os.path.join(root, "want"))
        self.Q = queries(self.after, np.random.default_rng(7), 300, "real" if self.kind == "real" else "u8")


@pytest.fixture(scope="module", params=list(B.CASES))
def case(request, tmp_path_factory):
    return Case(request.param, str(tmp_path_factory.mktemp("rebalance_" + request.param)))


def test_index_bin_holds_the_replays_table(case):
    orc = O.OracleIndex.load(*case.dirs)
    C, c2s = orc.centroids()
    assert C.shape == case.after.C.shape
    differ = np.flatnonzero((bits(C) != bits(case.after.C)).any(axis=1))
    assert differ.size == 0, "centroids of lists %s differ from the replay" % differ.tolist()
    assert (c2s == case.st.c2s).all() and orc.num_centroids == case.st.k
    gC, gc2s = case.gpu.centroids()
    assert (bits(gC) == bits(case.after.C)).all() and (gc2s == case.st.c2s).all()
    assert sorted(os.listdir(case.dirs[0])) == ["index.bin"], "a temporary file was left behind"


def test_shard_files_are_byte_identical(case):
    got = all_bytes(case.dirs[1])
    assert sorted(os.listdir(case.dirs[1])) == sorted(case.want), "a temporary file was left behind, or a shard is missing"
    for f in case.want:
        assert got[f] == case.want[f], f
    back, ids = R.read_state(*case.dirs)
    assert (ids == np.arange(len(ids), dtype=np.uint64)).all()   # internal ids: the new list order


def test_export_equals_the_replay(case):
    a = case.after
    ext, X, ts, where = case.gpu.export()
    assert case.gpu.num_vectors == len(a.lab) == len(ext)
    assert (ext == a.ext).all() and (ts == a.ts).all() and (bits(X) == bits(a.X)).all()
    pos = np.concatenate([np.arange(m) for m in a.lens()])
    assert ((where >> np.uint64(32)).astype(np.int64) == a.lab).all() and ((where & np.uint64(0xFFFFFFFF)).astype(np.int64) == pos).all()


def test_counts_and_list_stats_equal_the_replay(case):
    st0, a, out = case.st, case.after, case.out
    assert case.returned == R.moved_between(st0, a) > 0
    bs = case.bstats
    assert bs["iterations_run"] == out.iterations_run == case.rule.iters and bs["moved"] == case.returned
    for f in ("pairs_planned", "splits_done", "splits_skipped"):
        assert bs[f] == out.count(f), f
    assert bs["pairs_planned"] >= 1 and bs["splits_done"] >= 1
    inner = sum(len(p["counts"]) for r in out.rounds for p in r)
    assert bs["inner_iterations"] == inner
    assert bs["lists_emptied"] == int(((st0.lens() > 0) & (a.lens() == 0)).sum())
    assert bs["split_bytes"] > 0 and bs["means_bytes"] > 0 and bs["rehome_bytes"] > 0
    assert bs["ms_total"] > 0 and bs["ms_split"] > 0 and 0 < bs["ms_split_kernels"] <= bs["ms_split"]
    assert case.stats_before == want_list_stats(st0.lens()) and case.gpu.list_stats() == want_list_stats(a.lens())
    assert case.gpu.list_stats()["empty_lists"] == (1 if case.name == "copies" else 0)
    assert case.gpu.refine_stats()["iterations_run"] == 0        # the stats of a refine are a refine's alone


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "nq%d_k%d_p%d" % s)
def test_searches_equal_the_oracle_of_the_written_files(case, shape):
    nq, k, p = shape
    Q = case.Q[:nq]
    rc, Do, Io = O.OracleIndex.load(*case.dirs).search_batch(Q, k, p)
    assert rc == O.ORC_OK
    Dh, Ih, cnt, _ = host_search(case.gpu, Q, k, p)
    assert_same(Dh, Ih, Do, Io, "host entry")
    Dd, Id = device_search(case.gpu, Q, k, p)
    assert_same(Dd, Id, Do, Io, "device entry")


def test_a_fresh_load_gives_the_same_index(case):
    fresh = vip.load(*case.dirs, case.dim)
    for nq, k, p in SHAPES[1:]:
        Q = case.Q[:nq]
        (Dg, Ig), sg = twice(case.gpu, Q, k, p)
        (Df, If), sf = twice(fresh, Q, k, p)
        assert_same(Dg, Ig, Df, If, "fresh load")
        for f in ("rank_mode", "rank_int8", "group_queries", "scanned_vectors", "coarse_candidates"):
            assert sg[f] == sf[f], f
    assert fresh.list_stats() == case.gpu.list_stats()


def test_a_filter_made_before_the_call_is_rejected(case):
    with pytest.raises(vip.ViError) as e:
        case.gpu.search_sync(case.Q[:5], 3, 4, filter=case.old_filter)
    assert e.value.status == N.VI_ERR_INVALID_INPUT
    flt = case.gpu.filter_timestamps(0, 1 << 40)
    assert flt.num_allowed == len(case.after.lab)
    assert_same(*case.gpu.search_sync(case.Q[:9], 5, 4, filter=flt), *case.gpu.search_sync(case.Q[:9], 5, 4), "a filter made after the call")


# ---- the calls against each other (on the states of refine_cases: the first five cases) ----
PLAIN = [n for n in B.CASES if n in R.CASES]


@pytest.fixture(scope="module", params=PLAIN)
def plain(request, tmp_path_factory):
    return Case(request.param, str(tmp_path_factory.mktemp("rebalance_calls_" + request.param)))


def test_split_rounds_zero_is_a_refine(plain):
    a = copy_dirs(plain.src, plain.root, "no_rounds")
    b = copy_dirs(plain.src, plain.root, "refine")
    ga, gb = vip.load(*a, plain.dim, now_secs=NOW), vip.load(*b, plain.dim, now_secs=NOW)
    moved_a = ga.rebalance(iters=2, split_rounds=0)
    moved_b = gb.refine(2)
    assert moved_a == moved_b > 0 and dir_bytes(a) == dir_bytes(b)
    sa = ga.rebalance_stats()
    assert sa["pairs_planned"] == sa["splits_done"] == sa["split_bytes"] == 0 and sa["iterations_run"] == 2
    Q = plain.Q[:33]
    assert_same(*ga.search_sync(Q, 10, 8), *gb.search_sync(Q, 10, 8), "rebalance without rounds against refine")


def test_three_rounds_in_one_call_equal_three_calls(plain):
    """the identity path (the first iteration of a call) against the gather path (the later ones)"""
    a = copy_dirs(plain.src, plain.root, "three_in_one")
    b = copy_dirs(plain.src, plain.root, "three_calls")
    ga, gb = vip.load(*a, plain.dim, now_secs=NOW), vip.load(*b, plain.dim, now_secs=NOW)
    rule = B.Rule(iters=3, split_rounds=3, receiver_max_len=1)
    moved_a = ga.rebalance(**rule.fields())
    sa = ga.rebalance_stats()
    planned = 0
    for _ in range(3):
        gb.rebalance(iters=1, split_rounds=1, receiver_max_len=1)
        planned += gb.rebalance_stats()["pairs_planned"]
    assert dir_bytes(a) == dir_bytes(b)
    out = B.replay_rule(plain.st, rule)
    want = R.expected_files(out.state, plain.base_sh, os.path.join(plain.root, "want3"))
    got = all_bytes(a[1])
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    C, _ = O.OracleIndex.load(*a).centroids()
    assert (bits(C) == bits(out.state.C)).all()
    assert moved_a == sa["moved"] == R.moved_between(plain.st, out.state) and sa["iterations_run"] == 3
    assert sa["pairs_planned"] == planned == out.count("pairs_planned") >= 3
    Q = plain.Q[:33]
    assert_same(*ga.search_sync(Q, 10, 8), *gb.search_sync(Q, 10, 8), "three rounds against three calls")


def new_rows(c, m):
    a = c.after
    new = np.ascontiguousarray(a.X[np.random.default_rng(11).integers(0, len(a.lab), m)] + np.float32(0.25), dtype=np.float32)
    if c.kind != "real":
        new = np.clip(np.rint(new), 0, 255).astype(np.float32)
    return new, np.uint64(9_000_000) + np.arange(m, dtype=np.uint64)


@pytest.mark.parametrize("call", ["add", "remove_ids", "upsert"])
def test_each_update_after_a_rebalance(plain, call):
    d = copy_dirs(plain.src, plain.root, "then_" + call)
    gpu = vip.load(*d, plain.dim, now_secs=NOW)
    gpu.rebalance()
    a, Q = plain.after, plain.Q[:33]
    n = len(a.lab)
    new, new_ext = new_rows(plain, 50)
    if call == "add":
        gpu.add(new, ext_ids=new_ext)
        back = check_against_oracle(gpu, d, Q, "add after rebalance")
        assert len(back.lab) == n + 50 == gpu.num_vectors
    elif call == "remove_ids":
        gone = a.ext[::9]
        assert gpu.remove_ids(gone) == len(gone)
        back = check_against_oracle(gpu, d, Q, "remove_ids after rebalance")
        assert len(back.lab) == n - len(gone)
    else:
        assert gpu.upsert(new[:40], a.ext[-40:]) == 40
        back = check_against_oracle(gpu, d, Q, "upsert after rebalance")
        assert len(back.lab) == n == gpu.num_vectors and np.isin(a.ext[-40:], back.ext).all()


def test_the_api_layers_rebalance(plain):
    d = copy_dirs(plain.src, plain.root, "api")
    ix = VectorIndexer.load(VectorIndexerConfig(plain.dim, index_dir=d[0], shards_dir=d[1]))
    assert ix.rebalance_lists() == plain.returned
    got = all_bytes(d[1])
    for f in plain.want:
        assert got[f] == plain.want[f], f
    e = copy_dirs(plain.src, plain.root, "adapter")
    gpu = vip.load(*e, plain.dim, now_secs=NOW)
    ad = FaissStyleAdapter(gpu)
    rep = ad.rebalance(vip.RebalanceRule())
    assert rep["moved"] == plain.returned
    assert rep["imbalance_before"] == R.imbalance(plain.st.lens()) and rep["imbalance_after"] == R.imbalance(plain.after.lens())
    assert rep["imbalance_after"] < rep["imbalance_before"] and ad.imbalance_factor() == rep["imbalance_after"]
    assert rep["empty_before"] == 1 and rep["empty_after"] == 0
    assert dir_bytes(e) == dir_bytes(d)
    with pytest.raises(TypeError):
        gpu.rebalance(vip.RebalanceRule(), iters=2)


def test_refusals_on_a_live_handle(plain):
    d = copy_dirs(plain.src, plain.root, "refused")
    gpu = vip.load(*d, plain.dim, now_secs=NOW)
    flt = gpu.filter_timestamps(0, 1 << 40)
    files = [os.path.join(x, f) for x in d for f in sorted(os.listdir(x))]
    before, mtimes = dir_bytes(d), [os.stat(f).st_mtime_ns for f in files]
    for fields in (dict(iters=0), dict(iters=1, split_rounds=2), dict(split_factor=0.5), dict(split_factor=float("nan")),
                   dict(split_factor=float("inf")), dict(split_iters=0), dict(split_iters=65)):
        with pytest.raises(vip.ViError) as e:
            gpu.rebalance(**fields)
        assert e.value.status == N.VI_ERR_INVALID_INPUT, fields
    assert dir_bytes(d) == before and [os.stat(f).st_mtime_ns for f in files] == mtimes
    Q = plain.Q[:9]
    assert_same(*gpu.search_sync(Q, 5, 4, filter=flt), *gpu.search_sync(Q, 5, 4), "the filter survives a refused call")
    part = vip.load(*plain.src, plain.dim, rank=0, world_size=2)
    with pytest.raises(vip.ViError) as e:
        part.rebalance()
    assert e.value.status == N.VI_ERR_INVALID_INPUT and "unpartitioned" in str(e.value)
    assert dir_bytes(plain.src) == dir_bytes(d)
