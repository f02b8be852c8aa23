"""GPU: vi_indexer_refine — the lists of a built index recentred on the records they hold and every record re-homed to
its nearest centroid, in index.bin, in the shard files and in the resident index.

Everything expected comes from the untouched oracle (refine_cases.py): the case directories from its build and writer,
one iteration from its update_centroids and its scalar distance chain, the shard files from its writer, the searches from a
fresh OracleIndex.load of the directories the handle wrote.  Centroid bits, file bytes, ids, distance bits, timestamps and
counts must match exactly; nothing here has a tolerance."""
import os
import shutil

import numpy as np
import pytest

import oracle_lib as O
import refine_cases as R
import vector_indexer_py as vip
from vector_indexer_py import _native as N
from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig
from vector_indexer_py.harness import FaissStyleAdapter

from remove_cases import all_bytes, assert_same, bits
from test_remove_records_gpu import device_search, host_search, twice

pytestmark = pytest.mark.gpu

NOW = R.NOW
SHAPES = [(1, 1, 1), (33, 10, 8), (300, 100, 20)]   # (nq, k, n_probe)


def copy_dirs(src, root, name):
    dst = (os.path.join(root, name, "index"), os.path.join(root, name, "shards"))
    shutil.copytree(src[0], dst[0])
    shutil.copytree(src[1], dst[1])
    return dst


def dir_bytes(dirs):
    """every file of the two directories (no temporary may be left: the names are compared too)"""
    out = {}
    for d in dirs:
        for f in sorted(os.listdir(d)):
            out[os.path.join(os.path.basename(d), f)] = open(os.path.join(d, f), "rb").read()
    return out


def replay_n(st, n):
    for _ in range(n):
        st, _ = R.replay(st)
    return st


def want_list_stats(lens):
    lens = np.asarray(lens)
    return dict(lists=len(lens), empty_lists=int((lens == 0).sum()), min_len=int(lens.min()), max_len=int(lens.max()),
                mean_len=float(lens.sum()) / len(lens), imbalance=R.imbalance(lens))


def queries(st, rng, nq, kind):
    """stored records themselves, and rows near them; integers 0..254 for the 8-bit-valued cases (the int8 images rank
    batches of such queries only)"""
    rows = st.X[rng.integers(0, len(st.X), nq)]
    noise = rng.standard_normal(rows.shape).astype(np.float32) * np.float32(0.3 * max(1.0, float(st.X.std()) / 4))
    noise[: nq // 3] = 0
    Q = rows + noise
    if kind != "real":
        Q = np.clip(np.rint(Q), 0, 254)
    return np.ascontiguousarray(Q, dtype=np.float32)


class Case:
    """a case of refine_cases, a handle on a copy of it that ran refine(1), and the replay of that iteration"""

    def __init__(self, name, root):
        self.name, self.root = name, root
        self.dim = R.CASES[name][0]
        idx, sh, self.st, self.info = R.make(name, root)
        self.src = (idx, sh)
        self.base_sh = os.path.join(root, "base", "shards")
        self.dirs = copy_dirs(self.src, root, "one")
        self.gpu = vip.load(*self.dirs, self.dim, now_secs=NOW)
        self.stats_before = self.gpu.list_stats()
        self.old_filter = self.gpu.filter_timestamps(0, 1 << 40)
        self.returned = self.gpu.refine(1)
        self.rstats = self.gpu.refine_stats()
        self.after, self.moved = R.replay(self.st)
        self.want = R.expected_files(self.after, self.base_sh, os.path.join(root, "want1"))
        self.Q = queries(self.after, np.random.default_rng(7), 300, R.CASES[name][1])

    def expected_dirs(self, st, name):
        """{file: bytes} of both directories holding `st` after a refine; index.bin by the handle that wrote it is compared
        through the oracle's reader (no oracle writes one alone)"""
        return R.expected_files(st, self.base_sh, os.path.join(self.root, name))


@pytest.fixture(scope="module", params=list(R.CASES))
def case(request, tmp_path_factory):
    return Case(request.param, str(tmp_path_factory.mktemp("refine_" + request.param)))


def test_index_bin_holds_the_replays_table(case):
    orc = O.OracleIndex.load(*case.dirs)
    C, c2s = orc.centroids()
    assert C.shape == case.after.C.shape and (bits(C) == bits(case.after.C)).all()
    assert (c2s == case.st.c2s).all() and orc.num_centroids == case.st.k
    gC, gc2s = case.gpu.centroids()
    assert (bits(gC) == bits(case.after.C)).all() and (gc2s == case.st.c2s).all()
    assert sorted(os.listdir(case.dirs[0])) == ["index.bin"], "a temporary file was left behind"
    e = case.info["emptied"]
    assert (bits(C[e]) == bits(case.st.C[e])).all()              # the list that stayed empty kept its centroid bits


def test_shard_files_are_byte_identical(case):
    got = all_bytes(case.dirs[1])
    assert sorted(os.listdir(case.dirs[1])) == sorted(case.want), "a temporary file was left behind, or a shard is missing"
    for f in case.want:
        assert got[f] == case.want[f], f
    back, ids = R.read_state(*case.dirs)
    assert (ids == np.arange(len(ids), dtype=np.uint64)).all()   # internal ids: the new list order


def test_every_record_sits_where_the_oracle_probes_first(case):
    orc = O.OracleIndex.load(*case.dirs)
    ext, X, ts, where = case.gpu.export()
    lists = (where >> np.uint64(32)).astype(np.int64)
    for i in range(len(X)):
        rc, p = orc.probe(X[i], 1)
        assert rc == O.ORC_OK and int(p[0]) == lists[i], i


def test_export_equals_the_replay(case):
    a = case.after
    ext, X, ts, where = case.gpu.export()
    assert case.gpu.num_vectors == len(a.lab) == len(ext)
    assert (ext == a.ext).all() and (ts == a.ts).all() and (bits(X) == bits(a.X)).all()
    lens = a.lens()
    pos = np.concatenate([np.arange(m) for m in lens]) if len(a.lab) else np.zeros(0)
    assert ((where >> np.uint64(32)).astype(np.int64) == a.lab).all() and ((where & np.uint64(0xFFFFFFFF)).astype(np.int64) == pos).all()
    counts, Xg, tsg, _ = case.gpu.get(a.ext[::17])
    assert (counts == 1).all() and (bits(Xg) == bits(a.X[::17])).all() and (tsg == a.ts[::17]).all()


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


def test_counts_and_list_stats_equal_the_replay(case):
    st0, a = case.st, case.after
    assert case.returned == case.moved == R.moved_between(st0, a) and case.moved > 0
    rs = case.rstats
    assert rs["iterations_run"] == 1 and rs["moved"] == case.moved
    assert rs["lists_emptied"] == int(((st0.lens() > 0) & (a.lens() == 0)).sum())
    with_lists = [f for f in case.want if len(R.shard_centroid_ids(case.dirs[1], int(f[len("shard_"):-len(".bin")])))]
    assert rs["shards_rewritten"] == len(with_lists) > 0
    assert rs["bytes_written"] == sum(len(case.want[f]) for f in with_lists) + os.path.getsize(os.path.join(case.dirs[0], "index.bin"))
    assert rs["means_bytes"] > 0 and rs["rehome_bytes"] > 0 and rs["ms_total"] > 0
    before, after = case.stats_before, case.gpu.list_stats()
    assert before == want_list_stats(st0.lens()) and after == want_list_stats(a.lens())
    assert after["empty_lists"] >= 1 and after["min_len"] == 0
    ad = FaissStyleAdapter.__new__(FaissStyleAdapter)
    ad._idx = case.gpu
    assert ad.imbalance_factor() == after["imbalance"]


def test_a_fresh_load_gives_the_same_index(case):
    """norms, images and rank modes of the swapped index are the ones a load of the written files makes"""
    fresh = vip.load(*case.dirs, case.dim)
    for nq, k, p in SHAPES[1:]:
        Q = case.Q[:nq]
        (Dg, Ig), sg = twice(case.gpu, Q, k, p)
        (Df, If), sf = twice(fresh, Q, k, p)
        assert_same(Dg, Ig, Df, If, "fresh load")
        for f in ("rank_mode", "rank_int8", "group_queries", "scanned_vectors", "coarse_candidates"):
            assert sg[f] == sf[f], f
    if case.name == "d128_u8":
        assert sg["rank_int8"] == 1, "the rebuilt 8-bit index ranks from its int8 image"
    assert fresh.list_stats() == case.gpu.list_stats()


def test_filters_across_a_refine(case):
    with pytest.raises(vip.ViError) as e:
        case.gpu.search_sync(case.Q[:5], 3, 4, filter=case.old_filter)
    assert e.value.status == N.VI_ERR_INVALID_INPUT
    # a window made after the call: the oracle's exhaustive search, cut to the window
    a = case.after
    lo, hi = 1200, 1700
    flt = case.gpu.filter_timestamps(lo, hi)
    inside = (a.ts >= lo) & (a.ts <= hi)
    assert flt.num_allowed == int(inside.sum()) > 0
    Q = case.Q[:20]
    Dg, Ig = case.gpu.search_sync(Q, 10, a.k, filter=flt)
    rc, Do, Io = O.OracleIndex.load(*case.dirs).search_batch(Q, len(a.lab), a.k)
    assert rc == O.ORC_OK
    ok = set(a.ext[inside].tolist())
    for i in range(len(Q)):
        keep = [j for j in range(Io.shape[1]) if int(Io[i, j]) in ok][:10]
        assert Ig[i, :len(keep)].tolist() == Io[i, keep].tolist() and (bits(Dg[i, :len(keep)]) == bits(Do[i, keep])).all(), i


def test_three_iterations_equal_three_calls(case):
    a = copy_dirs(case.src, case.root, "three_in_one")
    b = copy_dirs(case.src, case.root, "three_calls")
    ga, gb = vip.load(*a, case.dim, now_secs=NOW), vip.load(*b, case.dim, now_secs=NOW)
    moved_a = ga.refine(3)
    sa = ga.refine_stats()
    for _ in range(3):
        gb.refine(1)
    assert dir_bytes(a) == dir_bytes(b)
    st3 = replay_n(case.st, 3)
    want = case.expected_dirs(st3, "want3")
    got = all_bytes(a[1])
    assert sorted(got) == sorted(want)
    for f in want:
        assert got[f] == want[f], f
    C, _ = O.OracleIndex.load(*a).centroids()
    assert (bits(C) == bits(st3.C)).all()
    assert moved_a == sa["moved"] == R.moved_between(case.st, st3) and sa["iterations_run"] == 3
    Q = case.Q[:33]
    assert_same(*ga.search_sync(Q, 10, 8), *gb.search_sync(Q, 10, 8), "refine(3) against three refine(1)")


def test_a_fixed_point_is_found_and_kept(case):
    d = copy_dirs(case.src, case.root, "fixed")
    gpu = vip.load(*d, case.dim, now_secs=NOW)
    gpu.refine(400)
    n = gpu.refine_stats()["iterations_run"]
    assert 1 < n < 400                                      # stopped early: the replay needs as many (test_refine_cases_cpu)
    st, m = case.st, 0
    while True:
        nxt, moved = R.replay(st)
        m += 1
        if moved == 0 and (bits(nxt.C) == bits(st.C)).all():
            break
        st = nxt
    assert n == m
    before = dir_bytes(d)
    C, _ = O.OracleIndex.load(*d).centroids()
    assert (bits(C) == bits(st.C)).all()
    assert gpu.refine(5) == 0
    rs = gpu.refine_stats()
    assert rs["iterations_run"] == 1 and rs["moved"] == 0 and rs["lists_emptied"] == 0
    assert dir_bytes(d) == before


def test_zero_iterations_touch_nothing(case):
    d = copy_dirs(case.src, case.root, "zero")
    gpu = vip.load(*d, case.dim, now_secs=NOW)
    flt = gpu.filter_timestamps(0, 1 << 40)
    files = [os.path.join(x, f) for x in d for f in sorted(os.listdir(x))]
    before, mtimes = dir_bytes(d), [os.stat(f).st_mtime_ns for f in files]
    assert gpu.refine(0) == 0
    assert dir_bytes(d) == before and [os.stat(f).st_mtime_ns for f in files] == mtimes
    Q = case.Q[:9]
    assert_same(*gpu.search_sync(Q, 5, 4, filter=flt), *gpu.search_sync(Q, 5, 4), "the filter made before refine(0)")
    assert gpu.refine_stats()["iterations_run"] == 0


def check_against_oracle(gpu, dirs, Q, what, unique=True):
    rc, Do, Io = O.OracleIndex.load(*dirs).search_batch(Q, 10, 8)
    assert rc == O.ORC_OK
    assert_same(*gpu.search_sync(Q, 10, 8), Do, Io, what)
    back, ids = R.read_state(*dirs)
    if unique:
        assert len(np.unique(ids)) == len(ids), what + ": internal ids repeat"
    return back


def new_rows(case, m):
    a = case.after
    new = np.ascontiguousarray(a.X[np.random.default_rng(11).integers(0, len(a.lab), m)] + np.float32(0.25), dtype=np.float32)
    if R.CASES[case.name][1] != "real":
        new = np.clip(np.rint(new), 0, 255).astype(np.float32)
    return new, np.uint64(9_000_000) + np.arange(m, dtype=np.uint64)


@pytest.mark.parametrize("call", ["add", "remove_ids", "upsert"])
def test_each_update_after_a_refine(case, call):
    """a refine numbers the records 0..n-1, so the update calls number on from there as after a build.  (An upsert numbers
    its rows n - replaced + i, include/vi_amd.h: unique where the replaced records carry the highest internal ids — the
    last of the list order, which is what this test replaces; in general its ids may repeat)"""
    d = copy_dirs(case.src, case.root, "then_" + call)
    gpu = vip.load(*d, case.dim, now_secs=NOW)
    gpu.refine(1)
    a, Q = case.after, case.Q[:33]
    n = len(a.lab)
    new, new_ext = new_rows(case, 50)
    if call == "add":
        gpu.add(new, ext_ids=new_ext)
        back = check_against_oracle(gpu, d, Q, "add after refine")
        assert len(back.lab) == n + 50 == gpu.num_vectors
    elif call == "remove_ids":
        gone = a.ext[::9]
        assert gpu.remove_ids(gone) == len(gone)
        back = check_against_oracle(gpu, d, Q, "remove_ids after refine")
        assert len(back.lab) == n - len(gone)
    else:
        assert gpu.upsert(new[:40], a.ext[-40:]) == 40
        back = check_against_oracle(gpu, d, Q, "upsert after refine")
        assert len(back.lab) == n == gpu.num_vectors and np.isin(a.ext[-40:], back.ext).all()


def test_a_refine_of_what_updates_left(case):
    """add, remove_ids, upsert one after another on a refined index, then a refine of that: against the replay of the files
    the three left (their internal ids may repeat, section 4h; the refine renumbers them)"""
    d = copy_dirs(case.src, case.root, "then_all")
    gpu = vip.load(*d, case.dim, now_secs=NOW)
    gpu.refine(1)
    a, Q = case.after, case.Q[:33]
    new, new_ext = new_rows(case, 50)
    gpu.add(new, ext_ids=new_ext)
    assert gpu.remove_ids(a.ext[::9]) == len(a.ext[::9])
    assert gpu.upsert(new[:40], a.ext[1::9][:40]) == 40
    check_against_oracle(gpu, d, Q, "the three updates", unique=False)
    st, _ = R.read_state(*d)
    want, moved = R.replay(st)
    assert gpu.refine(1) == moved
    got = check_against_oracle(gpu, d, Q, "refine after the updates")
    assert (got.ext == want.ext).all() and (bits(got.X) == bits(want.X)).all() and (bits(got.C) == bits(want.C)).all()


def test_a_list_emptied_by_remove_ids(case):
    """emptied before the call: it keeps its centroid bits when it stays empty and receives records when the replay says so"""
    st = case.st
    lens = st.lens()
    outcome = R.emptied_outcomes(st)
    full = sorted(outcome)
    refilled = max(full, key=lambda l: outcome[l][0])
    stays = [l for l in full if outcome[l][0] == 0]
    assert (outcome[refilled][0] > 0) == (case.name in R.REFILLED_CASES) and stays
    for what, l in [("stays empty", stays[0])] + ([("refilled", refilled)] if outcome[refilled][0] else []):
        d = copy_dirs(case.src, case.root, "emptied_" + what.replace(" ", "_"))
        gpu = vip.load(*d, case.dim, now_secs=NOW)
        assert gpu.remove_ids(st.ext[st.lab == l]) == lens[l]
        n_after, cut, after = outcome[l]
        assert gpu.refine(1) == R.moved_between(cut, after)
        got, ids = R.read_state(*d)
        assert got.lens()[l] == n_after and (got.lab == after.lab).all() and (got.ext == after.ext).all(), what
        assert (bits(got.C) == bits(after.C)).all(), what
        if n_after == 0:
            assert (bits(got.C[l]) == bits(st.C[l])).all()
        assert gpu.list_stats() == want_list_stats(after.lens())


def test_refusals(case):
    part = vip.load(*case.src, case.dim, rank=0, world_size=2)
    before = dir_bytes(case.src)
    with pytest.raises(vip.ViError) as e:
        part.refine(1)
    assert e.value.status == N.VI_ERR_INVALID_INPUT and "unpartitioned" in str(e.value)
    assert dir_bytes(case.src) == before
    assert part.list_stats()["lists"] == case.st.k         # statistics work on any handle: the rank's part of every list
    assert part.list_stats()["max_len"] <= want_list_stats(case.st.lens())["max_len"]


def test_the_api_layer_refines(case):
    d = copy_dirs(case.src, case.root, "api")
    ix = VectorIndexer.load(VectorIndexerConfig(case.dim, index_dir=d[0], shards_dir=d[1]))
    assert ix.refine_lists(0) == 0
    assert ix.refine_lists(1) == case.moved
    got = all_bytes(d[1])
    for f in case.want:
        assert got[f] == case.want[f], f
