"""GPU: vi_indexer_upsert_records — records replaced by external id, in the shard files and in the resident index, from
one rewrite and one pass over the new blocks.

The contract: afterwards the index is the one vi_indexer_remove_ids followed by vi_indexer_add_records leaves.
Everything expected comes from the untouched oracle: the shard files from its reader and writer
(upsert_cases.expected_upsert: remove_cases.expected_remove, then add_cases.expected_append), the labels of new rows
from its coarse step, the search results from a fresh OracleIndex.load of the directories the handle wrote.  Ids,
distance bits, counts and padding must match exactly; the files byte for byte; and a second handle that ran the two
existing calls must agree in files, D, I and tie keys."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from vector_indexer_py import _native as N
from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig, VectorRecord
from vector_indexer_py.harness import FaissStyleAdapter

import upsert_cases as U
from remove_cases import all_bytes, assert_same, bits
from test_remove_records_gpu import (N0, NLIST, NOW, ODD, SHAPES, base_ext, base_ts, clustered, descriptors, device_search,
                                     host_search, list_ext_ids, twice)

pytestmark = pytest.mark.gpu


def device_search_tie(gpu, Q, k, p):
    from hiprt import Hip
    hip = Hip()
    try:
        nq = Q.shape[0]
        xq = hip.upload(np.ascontiguousarray(Q, dtype=np.float32))
        D, I, T = hip.alloc(nq * k * 4), hip.alloc(nq * k * 8), hip.alloc(nq * k * 8)
        gpu.search_device(xq, nq, k, p, D, I, T)
        return hip.download(D, (nq, k), np.float32), hip.download(I, (nq, k), np.int64), hip.download(T, (nq, k), np.uint64)
    finally:
        hip.close()


def copy_dirs(src_idx, src_sh, root, name):
    dst = (str(root / name / "index"), str(root / name / "shards"))
    shutil.copytree(src_idx, dst[0])
    shutil.copytree(src_sh, dst[1])
    return dst


def stored_ext(sh, c2s):
    """external ids of every list, in list order, by the oracle's reader"""
    return [list_ext_ids(sh, c2s, l) for l in range(len(c2s))]


def upsert_and_record(gpu, c2s, idx, sh, exp_dir, ext, aims, x, ts, dim):
    """one upsert through the product; what the oracle alone expects of it, and what the product did"""
    orc = O.OracleIndex.load(idx, sh)
    labels = U.oracle_labels(orc, x)
    assert (labels == np.asarray(aims, dtype=np.uint64)).all(), "a row is not nearest to the centroid it was made for"
    n_before = gpu.num_vectors
    replaced = int(sum(np.isin(l, ext).sum() for l in stored_ext(sh, c2s)))
    ids = np.uint64(n_before - replaced) + np.arange(len(ext), dtype=np.uint64)
    ts_stored = np.where(ts == 0, np.uint64(NOW), ts).astype(np.uint64)
    want, removed, received = U.expected_files(c2s, sh, exp_dir, labels, ids, ext, ts_stored, x, dim)
    assert sum(removed.values()) == replaced
    before = all_bytes(sh)
    returned = gpu.upsert(x, ext, ts)
    return dict(want=want, removed=removed, received=received, before=before, got=all_bytes(sh), names=os.listdir(sh),
                returned=returned, replaced=replaced, stats=gpu.upsert_stats(), n_total=gpu.num_vectors,
                n_want=n_before - replaced + len(ext), index_bin=open(os.path.join(idx, "index.bin"), "rb").read())


class Stage:
    """a copy of the base that ran the first k + 1 calls through upsert(), the oracle of what it wrote, and a second handle
    on another copy that ran remove_ids() then add() for each call"""

    def __init__(self, case, k):
        self.k = k
        self.idx, self.sh = copy_dirs(case.base_idx, case.base_sh, case.root, f"stage{k}")
        self.gpu = vip.load(self.idx, self.sh, case.dim, now_secs=NOW)
        self.pair_idx, self.pair_sh = copy_dirs(case.base_idx, case.base_sh, case.root, f"pair{k}")
        self.pair = vip.load(self.pair_idx, self.pair_sh, case.dim, now_secs=NOW)
        self.old_filter = self.gpu.filter_timestamps(0, 1 << 40)
        self.calls = []
        for ci in range(k + 1):
            ext, aims, x, ts = case.calls[ci]
            self.calls.append(upsert_and_record(self.gpu, case.c2s, self.idx, self.sh, str(case.root / f"exp{k}_{ci}"), ext, aims, x,
                                                ts, case.dim))
            assert self.pair.remove_ids(ext) == self.calls[-1]["replaced"]
            self.pair.add(x, ext_ids=ext, timestamps=ts)
        self.orc = O.OracleIndex.load(self.idx, self.sh)
        self.new_lens = np.array([self.orc.list_len(c) for c in range(len(case.cent))], dtype=np.int64)
        self.lists = stored_ext(self.sh, case.c2s)
        ext, aims, x, ts = case.calls[k]
        self.new_ext, self.new_x = ext, x
        rng = np.random.default_rng(100 + k)
        m = min(100, len(x))
        near = case.X[rng.integers(0, len(case.X), 300 - m)] + 0.3 * rng.standard_normal((300 - m, case.dim))
        Q = np.concatenate([x[:m], near]).astype(np.float32)        # new records themselves, and near rows
        self.Q = np.ascontiguousarray(Q[rng.permutation(300)])
        self._fresh = None

    @property
    def fresh(self):
        if self._fresh is None:
            self._fresh = vip.load(self.idx, self.sh, self.gpu.dimension)
        return self._fresh


class Case:
    """a base index written by the oracle and the two calls of upsert_cases.block_case_calls"""

    def __init__(self, root, X, seed):
        rng = np.random.default_rng(seed)
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.dim, self.root = X.shape[1], root
        self.base_idx, self.base_sh = str(root / "base" / "index"), str(root / "base" / "shards")
        O.OracleIndex.build(self.X, self.base_idx, self.base_sh, ext_ids=base_ext(len(X)), timestamps=base_ts(len(X)), nlist=NLIST, now=NOW)
        base_orc = O.OracleIndex.load(self.base_idx, self.base_sh)
        self.cent, self.c2s = base_orc.centroids()
        self.lens = np.array([base_orc.list_len(c) for c in range(len(self.cent))], dtype=np.int64)
        self.lists = stored_ext(self.base_sh, self.c2s)
        self.index_bin = open(os.path.join(self.base_idx, "index.bin"), "rb").read()
        self.aim, plan = U.block_case_calls(self.cent, self.lens, self.lists, rng)
        self.calls = []
        for ci, (ext, aims) in enumerate(plan):
            ts = np.uint64(5000 + 1000 * ci) + np.arange(len(ext), dtype=np.uint64)
            ts[::7] = 0                                               # the add's `now` rule
            self.calls.append((ext, aims, U.rows_near(self.cent, aims, rng), ts))
        self.stages = [Stage(self, 0), Stage(self, 1)]


@pytest.fixture(scope="module", params=[3, 16, 100, 128, 200], ids=lambda d: f"D{d}")
def case(request, tmp_path_factory):
    d = request.param
    return Case(tmp_path_factory.mktemp(f"upsert{d}"), clustered(d), seed=d)


@pytest.fixture(params=[0, 1], ids=["call1", "call2"])
def stage(request, case):
    return case.stages[request.param]


def test_calls_are_what_they_were_meant_to_be(case):
    """the lists come from the oracle's reader; this pins that the calls realise the block cases they were made for"""
    aim, old, L = case.aim, case.lens, case.lists
    a, b, c, d, e, g = (aim[k] for k in "ABCDEG")
    s0, s1 = case.stages
    new, now = s0.new_lens, s0.lists
    # call 1
    ext1 = case.calls[0][0]
    assert len(np.unique(ext1)) < len(ext1) and (np.diff(ext1.astype(np.float64)) < 0).any()      # duplicates, unsorted
    assert old[a] > 64 and new[a] == old[a]                                # A: same length ...
    assert now[a].tolist() == np.delete(L[a], 5).tolist() + [int(L[a][5])]   # ... every position from 5 on moved
    kept_b = old[b] // 64 * 64
    assert old[b] % 64 != 0 and kept_b > 0 and new[b] == old[b]
    assert now[b][:kept_b].tolist() == L[b][:kept_b].tolist() and set(now[b][kept_b:].tolist()) == set(L[b][kept_b:].tolist())
    assert new[c] == old[c] - 64 + 70 and (old[c] - 64) % 64 != 0 and (old[c] - 64) // 64 != (old[c] + 5) // 64
    assert now[c][:old[c] - 64].tolist() == L[c][64:].tolist()
    assert old[d] > 64 and new[d] == 5 and set(now[d].tolist()) <= set(L[d].tolist())
    assert old[e] > 0 and new[e] == 0
    assert new[g] == old[g] + (old[d] - 5) + old[e] + 1 and now[g][:old[g]].tolist() == L[g].tolist() and old[g] > 64
    others = [l for l in range(len(old)) if l not in aim.values()]
    assert len(others) >= 3 and (new[others] == old[others]).all()
    assert s0.calls[0]["replaced"] == 1 + (old[b] - kept_b) + 64 + old[d] + old[e]
    # call 2
    assert s1.new_lens[e] == 70 and s1.lists[e].tolist() == case.calls[1][0][case.calls[1][1] == e].tolist()
    assert s1.new_lens[a] == old[a] - 1 and s1.lists[a][:5].tolist() == now[a][3:8].tolist()
    assert s1.new_lens[g] == new[g] + 3 and s1.calls[1]["replaced"] == 3 + 2
    assert (s1.new_lens[others] == old[others]).all()


def test_files_are_byte_identical_after_each_call(case, stage):
    for call in stage.calls:
        assert sorted(call["got"]) == sorted(call["want"])
        for f in call["want"]:
            assert call["got"][f] == call["want"][f], f
        assert sorted(call["names"]) == sorted(call["want"]), "a temporary file was left behind"
        assert call["index_bin"] == case.index_bin
        assert call["returned"] == call["replaced"] == sum(call["removed"].values()) and call["n_total"] == call["n_want"]
        st = call["stats"]
        touched_files = [f for f in call["want"] if call["removed"][f] or call["received"][f]]
        assert st["n"] == sum(call["received"].values()) and st["n_replaced"] == call["replaced"]
        assert st["shards_rewritten"] == len(touched_files)
        assert st["bytes_written"] == sum(len(call["want"][f]) for f in touched_files)
        assert st["kernel_bytes"] > 0
        for f in call["want"]:                               # a shard that lost and received nothing was not rewritten
            assert (call["got"][f] == call["before"][f]) == (f not in touched_files)
    st = stage.calls[0]["stats"]
    assert (st["lists_touched"], st["lists_emptied"]) == (6, 1)
    if stage.k == 1:
        st = stage.calls[1]["stats"]
        assert (st["lists_touched"], st["lists_emptied"]) == (3, 0)


@pytest.mark.parametrize("engine", ["default", "VI_FILTER=0", "VI_FORCE_GENERIC=1"])
def test_searches_equal_the_oracle_of_the_written_files(case, stage, engine, monkeypatch):
    if engine != "default":
        monkeypatch.setenv(*engine.split("="))
    for nq, k, p in SHAPES:
        rc, Do, Io = stage.orc.search_batch(stage.Q[:nq], k, p)
        assert rc == O.ORC_OK
        Dg, Ig, cnt, _ = host_search(stage.gpu, stage.Q[:nq], k, p)
        assert_same(Dg, Ig, Do, Io, f"host {engine} {(nq, k, p)}")
        assert (cnt == (Io != -1).sum(axis=1)).all()      # (an id past 2^63 reads as a negative i64; only -1 pads)
        Dd, Id = device_search(stage.gpu, stage.Q[:nq], k, p)
        assert_same(Dd, Id, Do, Io, f"device {engine} {(nq, k, p)}")
    if stage.k == 0:      # the emptied list is still in the coarse table and still probed, and nothing is in it
        q = case.cent[case.aim["E"]][None, :]
        D, I, cnt, _ = host_search(stage.gpu, q, 10, 1)
        assert cnt[0] == 0 and (I == -1).all() and np.isinf(D).all()


def test_stored_vectors_and_radius_zero(case, stage):
    rows_of = {}      # external id -> the vectors stored under it now
    for e, v in zip(base_ext(N0).tolist(), case.X):
        rows_of[e] = [v]
    for ext, aims, x, ts in case.calls[:stage.k + 1]:
        for e in set(ext.tolist()):
            rows_of[e] = []
        for e, v in zip(ext.tolist(), x):
            rows_of[e].append(v)
    D, I, cnt, V = host_search(stage.gpu, stage.Q[:33], 10, 8, include_vectors=True)
    hit = np.argwhere(I != -1)
    assert len(hit) and np.isin(I[I != -1], stage.new_ext.astype(np.int64)).any()
    for q, r in hit:
        assert any(np.array_equal(bits(V[q, r]), bits(v)) for v in rows_of[int(I[q, r]) & ((1 << 64) - 1)]), (q, r)
    pick = np.arange(0, len(stage.new_ext), max(1, len(stage.new_ext) // 20))
    lims, Dr, Ir = stage.gpu.range_search_sync(stage.new_x[pick], 0.0, len(case.cent))
    for i, e in enumerate(stage.new_ext[pick].astype(np.int64).tolist()):      # (results carry ids as i64)
        assert e in Ir[int(lims[i]):int(lims[i + 1])].tolist(), i
    assert (bits(Dr) == 0).all()


def test_the_two_existing_calls_give_the_same_index(case, stage):
    assert all_bytes(stage.sh) == all_bytes(stage.pair_sh)
    assert stage.gpu.num_vectors == stage.pair.num_vectors
    for nq, k, p in SHAPES:
        Da, Ia, Ta = device_search_tie(stage.gpu, stage.Q[:nq], k, p)
        Db, Ib, Tb = device_search_tie(stage.pair, stage.Q[:nq], k, p)
        assert_same(Da, Ia, Db, Ib, f"remove_ids + add {(nq, k, p)}")
        assert np.array_equal(Ta[Ia != -1], Tb[Ib != -1]), (nq, k, p)
    (_, _), sa = twice(stage.gpu, stage.Q[:300], 100, NLIST)
    (_, _), sb = twice(stage.pair, stage.Q[:300], 100, NLIST)
    assert (sa["rank_mode"], sa["rank_int8"]) == (sb["rank_mode"], sb["rank_int8"])


def test_fresh_load_gives_the_same_index(case, stage):
    assert stage.fresh.num_vectors == stage.gpu.num_vectors == stage.calls[-1]["n_want"]
    for nq, k, p in SHAPES:
        (Da, Ia), sa = twice(stage.gpu, stage.Q[:nq], k, p)
        (Df, If), sf = twice(stage.fresh, stage.Q[:nq], k, p)
        assert_same(Da, Ia, Df, If, f"fresh load {(nq, k, p)}")
        for f in ("rank_mode", "rank_int8", "group_queries", "scanned_vectors"):
            assert sa[f] == sf[f], (f, (nq, k, p), sa[f], sf[f])


def test_filters_across_an_upsert(case, stage):
    q = stage.Q[:33]
    with pytest.raises(vip.ViError) as e:
        stage.gpu.search_sync(q, 10, 8, filter=stage.old_filter)
    assert e.value.status == N.VI_ERR_INVALID_INPUT
    flt = stage.gpu.filter_ids(stage.new_ext)
    assert flt.num_allowed == len(stage.new_ext)
    D, I = stage.gpu.search_sync(q, 10, 8, filter=flt)
    assert (I != -1).any() and np.isin(I[I != -1], stage.new_ext.astype(np.int64)).all()
    assert stage.gpu.filter_ids(stage.new_ext, exclude=True).num_allowed == stage.gpu.num_vectors - len(stage.new_ext)


# ---- 8-bit data: the int8 image across upserts ---------------------------------------------------------------------------
def test_8bit_index_keeps_loses_and_regains_its_int8_image(tmp_path):
    rng = np.random.default_rng(12)
    X = descriptors(rng, N0)
    idx, sh = str(tmp_path / "index"), str(tmp_path / "shards")
    O.OracleIndex.build(X, idx, sh, ext_ids=base_ext(N0), timestamps=base_ts(N0), nlist=NLIST, now=NOW)
    gpu = vip.load(idx, sh, 128, now_secs=NOW)
    Q = np.clip(X[rng.integers(0, N0, 300)] + rng.integers(-3, 4, size=(300, 128)), 0, 254).astype(np.float32)

    def check(want_i8, what):
        orc = O.OracleIndex.load(idx, sh)
        for nq, k, p in SHAPES[:3]:
            rc, Do, Io = orc.search_batch(Q[:nq], k, p)
            (Dg, Ig), st = twice(gpu, Q[:nq], k, p)
            assert_same(Dg, Ig, Do, Io, f"{what} {(nq, k, p)}")
        fresh = vip.load(idx, sh, 128)
        (Df, If), sf = twice(fresh, Q[:nq], k, p)
        assert_same(Df, If, Do, Io, f"{what}, fresh load")
        assert (st["rank_mode"], st["rank_int8"]) == (sf["rank_mode"], sf["rank_int8"])
        assert st["rank_int8"] == want_i8, (what, st)

    check(1, "the base")
    some = np.arange(100, 300)
    assert gpu.upsert(descriptors(rng, len(some)), base_ext(N0)[some]) == len(some)
    check(1, "records replaced by integer rows")
    odd = X[ODD:ODD + 1].copy()
    odd[0, 5] += 0.5
    assert gpu.upsert(odd, base_ext(N0)[ODD:ODD + 1]) == 1
    check(0, "one fractional row")
    assert gpu.upsert(X[ODD:ODD + 1], base_ext(N0)[ODD:ODD + 1]) == 1
    check(1, "that row upserted back to integers")
    assert gpu.num_vectors == N0


# ---- no-ops, refusals, everything replaced, wrappers -----------------------------------------------------------------------
@pytest.fixture()
def small(tmp_path):
    X = clustered(16)
    idx, sh = str(tmp_path / "index"), str(tmp_path / "shards")
    O.OracleIndex.build(X, idx, sh, ext_ids=base_ext(N0), timestamps=base_ts(N0), nlist=NLIST, now=NOW)
    orc = O.OracleIndex.load(idx, sh)
    cent, c2s = orc.centroids()
    return dict(root=tmp_path, X=X, idx=idx, sh=sh, Q=X[:100] + np.float32(0.1), cent=cent, c2s=c2s)


def test_replacing_every_record_in_one_call(small):
    """the two-call form stops at "an index keeps at least one record"; lists that receive nothing become empty"""
    rng = np.random.default_rng(3)
    gpu = vip.load(small["idx"], small["sh"], 16, now_secs=NOW)
    with pytest.raises(vip.ViError):
        gpu.remove_ids(base_ext(N0))
    ext = base_ext(N0)[rng.permutation(N0)]
    aims = rng.choice(np.array([2, 7, 11]), N0)
    x = U.rows_near(small["cent"], aims, rng)
    ts = np.uint64(9000) + np.arange(N0, dtype=np.uint64)
    rec = upsert_and_record(gpu, small["c2s"], small["idx"], small["sh"], str(small["root"] / "exp"), ext, aims, x, ts, 16)
    assert rec["returned"] == N0 == rec["n_total"] and rec["got"] == rec["want"] and sorted(rec["names"]) == sorted(rec["want"])
    nl = len(small["cent"])
    assert nl > 11 and (rec["stats"]["lists_touched"], rec["stats"]["lists_emptied"]) == (nl, nl - 3)
    orc = O.OracleIndex.load(small["idx"], small["sh"])
    lens = np.array([orc.list_len(c) for c in range(nl)])
    assert lens.sum() == N0 and (lens > 0).sum() == 3
    Q = np.concatenate([x[:150], small["Q"]]).astype(np.float32)
    for nq, k, p in SHAPES:
        rc, Do, Io = orc.search_batch(Q[:nq], k, p)
        Dg, Ig, cnt, _ = host_search(gpu, Q[:nq], k, p)
        assert_same(Dg, Ig, Do, Io, f"everything replaced {(nq, k, p)}")
    fresh = vip.load(small["idx"], small["sh"], 16)
    assert_same(*fresh.search_sync(Q[:33], 10, 8), *gpu.search_sync(Q[:33], 10, 8), "fresh load")


def test_no_ops_and_refusals_leave_files_and_handle(small):
    L = N.lib()
    gpu = vip.load(small["idx"], small["sh"], 16, now_secs=NOW)
    flt = gpu.filter_timestamps(1000, 1499)
    D0, I0 = gpu.search_sync(small["Q"], 10, 8, filter=flt)
    before = all_bytes(small["sh"])
    ids = np.ascontiguousarray(base_ext(N0)[:4])
    x = np.ascontiguousarray(small["X"][:4])
    bad = x.copy()
    bad[2, 3] = np.nan
    replaced = C.c_uint64(9)

    def unchanged(what):
        assert all_bytes(small["sh"]) == before and sorted(os.listdir(small["sh"])) == sorted(before), what
        assert gpu.num_vectors == N0, what
        assert_same(*gpu.search_sync(small["Q"], 10, 8, filter=flt), D0, I0, what)      # the old filter is still this index's

    assert L.vi_indexer_upsert_records(gpu._h, None, None, None, 0, C.byref(replaced)) == 0 and replaced.value == 0
    assert gpu.upsert(np.zeros((0, 16), dtype=np.float32), []) == 0
    unchanged("n == 0")
    assert gpu.upsert_stats()["n"] == 0
    for what, args in (("null ids", (None, N.ptr(x), None, 4)), ("null values", (N.ptr(ids), None, None, 4)),
                       ("a NaN", (N.ptr(ids), N.ptr(bad), None, 4)), ("past 2^32 - 2", (N.ptr(ids), N.ptr(x), None, 1 << 32))):
        replaced = C.c_uint64(9)
        assert L.vi_indexer_upsert_records(gpu._h, *args, C.byref(replaced)) == N.VI_ERR_INVALID_INPUT, what
        assert replaced.value == 0
        unchanged(what)
    part = vip.load(small["idx"], small["sh"], 16, rank=0, world_size=2)
    with pytest.raises(vip.ViError) as e:
        part.upsert(x, ids)
    assert e.value.status == N.VI_ERR_INVALID_INPUT
    unchanged("a partitioned handle")
    # a shard file whose list no longer has its resident length: one record taken out of the file behind the handle
    l = int(U.oracle_labels(O.OracleIndex.load(small["idx"], small["sh"]), small["X"][:1])[0])
    in_list = list_ext_ids(small["sh"], small["c2s"], l)
    victim = np.ascontiguousarray(in_list[-1:])
    assert L.vi_shard_remove_from(small["sh"].encode(), int(small["c2s"][l]), N.ptr(victim), 1, None) == 0
    before = all_bytes(small["sh"])
    with pytest.raises(vip.ViError) as e:
        gpu.upsert(small["X"][:1], in_list[:1])
    assert e.value.status == N.VI_ERR_INVALID_DATA
    unchanged("a file that no longer matches")


def test_python_wrappers_equal_the_c_abi_path(small):
    rng = np.random.default_rng(8)
    ext = np.concatenate([base_ext(N0)[::7], np.array([5, 6], dtype=np.uint64)])
    n_known = len(base_ext(N0)[::7])
    x = (small["X"][rng.integers(0, N0, len(ext))] + 0.05 * rng.standard_normal((len(ext), 16))).astype(np.float32)
    ts = np.full(len(ext), NOW, dtype=np.uint64)
    roots = {name: copy_dirs(small["idx"], small["sh"], small["root"], name) for name in ("abi", "index", "indexer", "faiss")}
    # the C ABI itself
    abi = vip.load(*roots["abi"], 16, now_secs=NOW)
    replaced = C.c_uint64(0)
    N.check(N.lib().vi_indexer_upsert_records(abi._h, N.ptr(ext), N.ptr(x), N.ptr(ts), len(ext), C.byref(replaced)))
    assert replaced.value == n_known and abi.num_vectors == N0 + 2
    Da, Ia = abi.search_sync(small["Q"], 10, 8)
    orc = O.OracleIndex.load(*roots["abi"])
    rc, Do, Io = orc.search_batch(small["Q"], 10, 8)
    assert_same(Da, Ia, Do, Io, "C entry")
    want = all_bytes(roots["abi"][1])
    # VectorIndex.upsert
    vx = vip.load(*roots["index"], 16, now_secs=NOW)
    assert vx.upsert(x, ext.tolist(), ts) == n_known
    assert all_bytes(roots["index"][1]) == want
    assert_same(*vx.search_sync(small["Q"], 10, 8), Da, Ia, "VectorIndex.upsert")
    st = vx.upsert_stats()
    assert (st["n"], st["n_replaced"]) == (len(ext), n_known) and st["shards_rewritten"] > 0
    # VectorIndexer.upsert_records
    vi = VectorIndexer.load(VectorIndexerConfig(16, *roots["indexer"]))
    req = vi.search_request(small["Q"][0]).with_k(10).with_n_probe(8).with_timestamp_range(0, 1 << 40)
    assert len(vi.search(req)) == 10                                   # (caches a filter of the old index)
    assert vi.upsert_records([VectorRecord(int(e), v.tolist(), NOW) for e, v in zip(ext, x)]) == n_known
    assert all_bytes(roots["indexer"][1]) == want
    for qi in (0, 30):
        got = vi.search(vi.search_request(small["Q"][qi]).with_k(10).with_n_probe(8).with_timestamp_range(0, 1 << 40))
        assert [r.external_id for r in got] == Ia[qi].tolist()
        assert np.array_equal(bits([r.distance for r in got]), bits(Da[qi]))
    assert vi.upsert_records([]) == 0
    # FaissStyleAdapter.update_vectors
    fa = FaissStyleAdapter(vip.load(*roots["faiss"], 16, now_secs=NOW))
    fa.nprobe = 8
    assert fa.update_vectors(ext, x) == n_known and fa.ntotal == N0 + 2
    assert all_bytes(roots["faiss"][1]) == want
    assert_same(*fa.search(small["Q"], 10), Da, Ia, "FaissStyleAdapter.update_vectors")
    assert fa.update_vectors(ext, x) == len(ext) and fa.ntotal == N0 + 2      # now every id is known


def test_upsert_of_unknown_ids_equals_add(small):
    """filter present with every bit set against filter absent, through the one block kernel: an upsert whose ids no record
    carries drops nothing, so it must leave what add leaves — files, ids, distance bits and tie keys"""
    rng = np.random.default_rng(14)
    orc = O.OracleIndex.load(small["idx"], small["sh"])
    lens = np.array([orc.list_len(c) for c in range(len(small["cent"]))], dtype=np.int64)
    # 66 rows behind a list whose last block is partly filled: that block mixes old and new lanes, the next holds new rows
    # only; 4 rows that fit into the last block of another list
    a = int(np.flatnonzero(lens % 64 != 0)[0])
    b = int(np.flatnonzero((lens % 64 != 0) & (lens % 64 <= 60) & (np.arange(len(lens)) != a))[0])
    aims = np.array([a] * 66 + [b] * 4, dtype=np.int64)[rng.permutation(70)]
    x = U.rows_near(small["cent"], aims, rng)
    assert (U.oracle_labels(orc, x) == aims.astype(np.uint64)).all(), "a row is not nearest to the centroid it was made for"
    assert 0 < lens[a] % 64 and 0 < lens[b] % 64 <= 60      # (64 - r of the 66 fill a's block, the other 2 + r have their own)
    ext = np.uint64(U.NEW_EXT0) + np.arange(70, dtype=np.uint64)
    ts = np.uint64(7000) + np.arange(70, dtype=np.uint64)
    ts[::7] = 0                                                       # the add's `now` rule
    roots = {name: copy_dirs(small["idx"], small["sh"], small["root"], name) for name in ("added", "upserted")}
    added = vip.load(*roots["added"], 16, now_secs=NOW)
    upserted = vip.load(*roots["upserted"], 16, now_secs=NOW)
    added.add(x, ext_ids=ext, timestamps=ts)
    assert upserted.upsert(x, ext, ts) == 0 and upserted.upsert_stats()["n_replaced"] == 0
    assert added.num_vectors == upserted.num_vectors == N0 + 70
    want = all_bytes(roots["added"][1])
    assert want != all_bytes(small["sh"]) and all_bytes(roots["upserted"][1]) == want
    new = O.OracleIndex.load(*roots["upserted"])
    assert new.list_len(a) == lens[a] + 66 and new.list_len(b) == lens[b] + 4
    Q = np.concatenate([x, small["Q"]]).astype(np.float32)
    for nq, k, p in SHAPES:
        Da, Ia, Ta = device_search_tie(added, Q[:nq], k, p)
        Du, Iu, Tu = device_search_tie(upserted, Q[:nq], k, p)
        assert_same(Du, Iu, Da, Ia, f"upsert against add {(nq, k, p)}")
        assert np.array_equal(Tu[Iu != -1], Ta[Ia != -1]), (nq, k, p)
        assert np.isin(Iu[Iu != -1], ext.astype(np.int64)).any(), (nq, k, p)      # (the first queries are new rows themselves)
