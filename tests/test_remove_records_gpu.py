"""GPU: vi_indexer_retain / vi_indexer_remove_ids — records removed from a built index, in the shard files and in the
resident index.

The contract: afterwards the index is the one the reference would search if the removed records had been deleted from
their inverted lists, the remaining records of each list closing up in their old order.  Everything expected comes from
the untouched oracle: the shard files from shard_get + numpy mask + shard_save (remove_cases.expected_remove), the search
results from a fresh OracleIndex.load of the directories the handle wrote.  Ids, distance bits, counts and padding must
match exactly; the files byte for byte."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from vector_indexer_py import _native as N
from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig
from vector_indexer_py.harness import FaissStyleAdapter

import add_cases as A
import remove_cases as R
from remove_cases import all_bytes, assert_same, bits

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000
N0, NLIST = 3000, 20
SHAPES = [(1, 1, 1), (33, 10, 8), (300, 100, 20), (33, 400, 1)]     # the add tests' shapes
EXT0 = 10_000_000


def base_ext(n):
    return np.uint64(EXT0) + np.uint64(3) * np.arange(n, dtype=np.uint64)


def base_ts(n):
    return np.uint64(1000) + (np.arange(n, dtype=np.uint64) * np.uint64(7919)) % np.uint64(1000)


def row_of_ext(ext):
    return (np.asarray(ext, dtype=np.int64) - EXT0) // 3


def host_search(gpu, Q, k, p, include_vectors=False):
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nq = Q.shape[0]
    D, I = np.zeros((nq, k), dtype=np.float32), np.zeros((nq, k), dtype=np.int64)
    V = np.zeros((nq, k, Q.shape[1]), dtype=np.float32) if include_vectors else None
    cnt = np.zeros(nq, dtype=np.uint64)
    N.check(N.lib().vi_indexer_search(gpu._h, N.ptr(Q), nq, Q.shape[1], k, p, N.ptr(D), N.ptr(I), N.ptr(V), N.ptr(cnt), None))
    return D, I, cnt, V


def device_search(gpu, Q, k, p):
    from hiprt import Hip
    hip = Hip()
    try:
        nq = Q.shape[0]
        xq, D, I = hip.upload(np.ascontiguousarray(Q, dtype=np.float32)), hip.alloc(nq * k * 4), hip.alloc(nq * k * 8)
        gpu.search_device(xq, nq, k, p, D, I)
        return hip.download(D, (nq, k), np.float32), hip.download(I, (nq, k), np.int64)
    finally:
        hip.close()


def twice(gpu, Q, k, p):
    """the second of two equal searches and its stats (handles with different pasts compare from the second batch on)"""
    gpu.search_sync(Q, k, p)
    out = gpu.search_sync(Q, k, p)
    return out, gpu.last_stats()


def list_ext_ids(sh, c2s, l):
    """external ids of list l in list order, by the oracle's reader"""
    rc, got = O.shard_get(sh, int(c2s[l]), [l])
    assert rc == O.ORC_OK
    return got[0][2][:, 1].copy()


class Case:
    """a base index written by the oracle, opened by the product, and the remove calls make_calls plans; what the tests
    compare is recorded while it is made"""

    def __init__(self, root, X, make_calls, nlist=NLIST, queries="real", seed=0, shapes=SHAPES):
        rng = np.random.default_rng(seed)
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.dim, self.shapes = X.shape[1], shapes
        self.root, self.idx, self.sh = root, str(root / "index"), str(root / "shards")
        O.OracleIndex.build(self.X, self.idx, self.sh, ext_ids=base_ext(len(X)), timestamps=base_ts(len(X)), nlist=nlist, now=NOW)
        base_orc = O.OracleIndex.load(self.idx, self.sh)
        self.cent, self.c2s = base_orc.centroids()
        self.lens = np.array([base_orc.list_len(c) for c in range(len(self.cent))], dtype=np.int64)
        self.lists = [list_ext_ids(self.sh, self.c2s, l) for l in range(len(self.cent))]
        self.index_bin = open(os.path.join(self.idx, "index.bin"), "rb").read()
        shutil.copytree(self.idx, str(root / "base" / "index"))      # the base, for the tests that remove in other ways
        shutil.copytree(self.sh, str(root / "base" / "shards"))
        self.gpu = vip.load(self.idx, self.sh, self.dim, now_secs=NOW)
        assert self.gpu.num_vectors == len(X)
        self.ids_of_call = [np.asarray(c, dtype=np.uint64) for c in make_calls(self, rng)]
        self.removed = np.unique(np.concatenate(self.ids_of_call))
        self.removed = self.removed[np.isin(self.removed, base_ext(len(X)))]
        # queries: removed records themselves (they would lead their results if they were still there), and near rows
        m = min(100, len(self.removed))
        near = self.X[rng.integers(0, len(X), 300 - m)]
        near = near + (0.3 * rng.standard_normal(near.shape) if queries == "real" else rng.integers(-3, 4, size=near.shape))
        Q = np.concatenate([self.X[row_of_ext(rng.choice(self.removed, m, replace=False))], near]).astype(np.float32)
        if queries != "real":       # whole numbers ("u8": in 0..254, what the int8 rank kernel takes)
            Q = np.rint(Q)
            Q = np.clip(Q, 0, 254) if queries == "u8" else Q
        self.Q = np.ascontiguousarray(Q[rng.permutation(300)], dtype=np.float32)
        # made before any removal: two filters (to be rejected later) and the results through a filter admitting exactly
        # the records that stay
        self.old_ts_filter = self.gpu.filter_timestamps(0, 1 << 40)
        self.old_id_filter = self.gpu.filter_ids(base_ext(len(X))[:100])
        deny = self.gpu.filter_ids(self.removed, exclude=True)
        assert deny.num_allowed == len(X) - len(self.removed)
        self.pre = {s: self.gpu.search_sync(self.Q[:s[0]], s[1], s[2], filter=deny) for s in shapes}
        self.gpu.search_sync(self.Q[:300], 100, nlist)
        self.pre_stats = self.gpu.last_stats()
        del deny
        # ---- the removals ----
        self.calls, n_now = [], len(X)
        for ci, ids in enumerate(self.ids_of_call):
            want, counts = R.expected_files(self.sh, str(root / f"expected{ci}"), ids, self.dim)
            before = all_bytes(self.sh)
            returned = self.gpu.remove_ids(ids)
            n_now -= sum(counts.values())
            self.calls.append(dict(want=want, counts=counts, before=before, got=all_bytes(self.sh), names=os.listdir(self.sh),
                                   returned=returned, stats=self.gpu.remove_stats(), n_total=self.gpu.num_vectors, n_want=n_now,
                                   index_bin=open(os.path.join(self.idx, "index.bin"), "rb").read()))
        self.n_total = n_now
        self.orc = O.OracleIndex.load(self.idx, self.sh)
        self.new_lens = np.array([self.orc.list_len(c) for c in range(len(self.cent))], dtype=np.int64)
        self._fresh = None

    @property
    def fresh(self):
        if self._fresh is None:
            self._fresh = vip.load(self.idx, self.sh, self.dim)
        return self._fresh

    def copy_of(self, what, name):
        """a copy of the base directories ("base") or of the directories as they are now ("now") -> (index, shards)"""
        src = (str(self.root / "base" / "index"), str(self.root / "base" / "shards")) if what == "base" else (self.idx, self.sh)
        dst = (str(self.root / name / "index"), str(self.root / name / "shards"))
        shutil.copytree(src[0], dst[0])
        shutil.copytree(src[1], dst[1])
        return dst


def block_case_calls(case, rng):
    """call 1, one list each: A loses one record of its first block (every later record crosses a block border); B its
    tail, down to a multiple of 64 (its last block disappears); C its first 64 records (an aligned shift); D all but
    every fifth of its first 200 (more than 64 records become fewer than 64); E everything; the other lists nothing.
    call 2: ten more of A's head, and ids that no longer exist"""
    order = np.argsort(case.lens, kind="stable")
    e = int(order[0])
    long = [int(l) for l in order if case.lens[l] > 64 and l != e]
    ragged = [l for l in long if case.lens[l] % 64 != 0]
    b = ragged[0]
    a, c, d = [l for l in long if l != b][:3]
    assert len({a, b, c, d, e}) == 5 and len(case.lens) - 5 >= 3
    case.aim = dict(A=a, B=b, C=c, D=d, E=e)
    L = case.lists
    keep_d = np.zeros(len(L[d]), dtype=bool)
    keep_d[:200:5] = True
    call1 = np.concatenate([L[a][5:6], L[b][len(L[b]) - len(L[b]) % 64:], L[c][:64], L[d][~keep_d], L[e]])
    left_a = np.delete(L[a], 5)
    call2 = np.concatenate([left_a[:10], L[c][:3], L[e][:2], np.array([1, 2, (1 << 64) - 1], dtype=np.uint64)])
    return [rng.permutation(np.concatenate([call1, call1[:7]])), call2]      # unsorted, with duplicates


@pytest.fixture(scope="module", params=[3, 16, 100, 128, 200], ids=lambda d: f"D{d}")
def case(request, tmp_path_factory):
    d = request.param
    return Case(tmp_path_factory.mktemp(f"remove{d}"), clustered(d), block_case_calls, seed=d)


def clustered(d):
    """N0 points around NLIST centres: at every D most lists are a few blocks long (unclustered points in 100 or more
    dimensions leave all but three or four lists with a single record, too few for the block cases)"""
    rng = np.random.default_rng(d)
    centres = 3.0 * rng.standard_normal((NLIST, d))
    return (centres[rng.integers(0, NLIST, N0)] + rng.standard_normal((N0, d))).astype(np.float32)


def test_removal_set_is_what_it_was_meant_to_be(case):
    """the lists come from the oracle's reader; this pins that the set realises the block cases it was made for"""
    aim, old, new = case.aim, case.lens, case.new_lens
    assert old[aim["A"]] > 64 and new[aim["A"]] == old[aim["A"]] - 11
    assert old[aim["B"]] % 64 != 0 and new[aim["B"]] % 64 == 0 and new[aim["B"]] == old[aim["B"]] // 64 * 64 > 0
    assert new[aim["C"]] == old[aim["C"]] - 64 > 0
    assert old[aim["D"]] > 64 > new[aim["D"]] > 0
    assert old[aim["E"]] > 0 and new[aim["E"]] == 0
    others = [l for l in range(len(old)) if l not in aim.values()]
    assert len(others) >= 3 and (new[others] == old[others]).all()
    assert case.calls[0]["counts"] != case.calls[1]["counts"] and sum(case.calls[1]["counts"].values()) == 10


def test_files_are_byte_identical_after_each_call(case):
    for call, ids in zip(case.calls, case.ids_of_call):
        assert sorted(call["got"]) == sorted(call["want"])
        for f in call["want"]:
            assert call["got"][f] == call["want"][f], f
        assert sorted(call["names"]) == sorted(call["want"]), "a temporary file was left behind"
        assert call["index_bin"] == case.index_bin
        n_removed = sum(call["counts"].values())
        assert call["returned"] == n_removed and call["n_total"] == call["n_want"]
        st = call["stats"]
        touched_files = [f for f, n in call["counts"].items() if n]
        assert st["n_removed"] == n_removed and st["shards_rewritten"] == len(touched_files)
        assert st["bytes_written"] == sum(len(call["want"][f]) for f in touched_files)
        for f in call["want"]:                               # a shard that lost nothing was not rewritten
            assert (call["got"][f] == call["before"][f]) == (f not in touched_files)
    st = case.calls[0]["stats"]
    assert (st["lists_touched"], st["lists_emptied"]) == (5, 1)
    assert (case.calls[1]["stats"]["lists_touched"], case.calls[1]["stats"]["lists_emptied"]) == (1, 0)


@pytest.mark.parametrize("engine", ["default", "VI_FILTER=0", "VI_FORCE_GENERIC=1"])
def test_searches_equal_the_oracle_of_the_written_files(case, engine, monkeypatch):
    if engine != "default":
        monkeypatch.setenv(*engine.split("="))
    for nq, k, p in SHAPES:
        rc, Do, Io = case.orc.search_batch(case.Q[:nq], k, p)
        assert rc == O.ORC_OK
        Dg, Ig, cnt, _ = host_search(case.gpu, case.Q[:nq], k, p)
        assert_same(Dg, Ig, Do, Io, f"host {engine} {(nq, k, p)}")
        assert (cnt == (Io >= 0).sum(axis=1)).all()
        Dd, Id = device_search(case.gpu, case.Q[:nq], k, p)
        assert_same(Dd, Id, Do, Io, f"device {engine} {(nq, k, p)}")
    assert (Io[:, 399] == -1).any() and np.isinf(Do[Io == -1]).all()   # the last shape pads
    # the emptied list is still in the coarse table and still probed: its own centroid finds it first, and nothing in it
    q = case.cent[case.aim["E"]][None, :]
    rc, probed = case.orc.probe(q[0], 1)
    assert rc == O.ORC_OK and probed.tolist() == [case.aim["E"]]
    D, I, cnt, _ = host_search(case.gpu, q, 10, 1)
    assert cnt[0] == 0 and (I == -1).all() and np.isinf(D).all()
    Dd, Id = device_search(case.gpu, q, 10, 1)
    assert (Id == -1).all() and np.isinf(Dd).all()


def test_fresh_load_gives_the_same_index(case):
    assert case.fresh.num_vectors == case.gpu.num_vectors == case.n_total
    for nq, k, p in SHAPES:
        (Da, Ia), sa = twice(case.gpu, case.Q[:nq], k, p)
        (Df, If), sf = twice(case.fresh, case.Q[:nq], k, p)
        assert_same(Da, Ia, Df, If, f"fresh load {(nq, k, p)}")
        for f in ("rank_mode", "rank_int8", "group_queries", "scanned_vectors"):
            assert sa[f] == sf[f], (f, (nq, k, p), sa[f], sf[f])


def test_results_equal_the_filtered_results_of_before(case):
    """ids and distance bits of a search through a deny filter of the removed ids, recorded before the removal"""
    for (nq, k, p), (Dp, Ip) in case.pre.items():
        Dg, Ig = case.gpu.search_sync(case.Q[:nq], k, p)
        assert_same(Dg, Ig, Dp, Ip, f"deny set of the removed ids, before {(nq, k, p)}")


def test_stored_vectors_and_radius_zero(case):
    D, I, cnt, V = host_search(case.gpu, case.Q[:33], 10, 8, include_vectors=True)
    hit = I >= 0
    assert hit.any() and not np.isin(I[hit], case.removed.astype(np.int64)).any()
    assert np.array_equal(bits(V[hit]), bits(case.X[row_of_ext(I[hit])]))      # the stored vectors of kept neighbours
    nl = len(case.cent)
    gone = case.removed[:: max(1, len(case.removed) // 20)]
    lims, Dr, Ir = case.gpu.range_search_sync(case.X[row_of_ext(gone)], 0.0, nl)
    for i, e in enumerate(gone):
        assert int(e) not in Ir[int(lims[i]):int(lims[i + 1])].tolist(), i
    left = np.setdiff1d(base_ext(N0), case.removed)[::137]
    lims, Dr, Ir = case.gpu.range_search_sync(case.X[row_of_ext(left)], 0.0, nl)
    for i, e in enumerate(left):
        assert int(e) in Ir[int(lims[i]):int(lims[i + 1])].tolist(), i
    assert (bits(Dr) == 0).all()


def test_filters_across_a_remove(case):
    q = case.Q[:33]
    for old in (case.old_ts_filter, case.old_id_filter):
        with pytest.raises(vip.ViError) as e:
            case.gpu.search_sync(q, 10, 8, filter=old)
        assert e.value.status == N.VI_ERR_INVALID_INPUT
        with pytest.raises(vip.ViError) as e:
            case.gpu.retain(old)
        assert e.value.status == N.VI_ERR_INVALID_INPUT
    assert case.gpu.filter_ids(case.removed).num_allowed == 0
    assert case.gpu.filter_ids(case.removed, exclude=True).num_allowed == case.n_total
    assert case.gpu.num_vectors == case.n_total


def test_retain_of_a_timestamp_window_equals_remove_ids_of_the_complement(case):
    lo, hi = 1200, 1699
    ts = base_ts(N0)
    outside = base_ext(N0)[(ts < lo) | (ts > hi)]
    a = vip.load(*case.copy_of("base", "retain"), case.dim)
    b = vip.load(*case.copy_of("base", "complement"), case.dim)
    flt = a.filter_timestamps(lo, hi)
    assert a.retain(flt) == len(outside) == b.remove_ids(outside)
    assert a.num_vectors == b.num_vectors == N0 - len(outside)
    assert all_bytes(str(case.root / "retain" / "shards")) == all_bytes(str(case.root / "complement" / "shards"))
    with pytest.raises(vip.ViError) as e:      # `keep` itself is a filter of the replaced index
        a.search_sync(case.Q[:4], 10, 8, filter=flt)
    assert e.value.status == N.VI_ERR_INVALID_INPUT
    orc = O.OracleIndex.load(str(case.root / "retain" / "index"), str(case.root / "retain" / "shards"))
    for nq, k, p in SHAPES[:3]:
        rc, Do, Io = orc.search_batch(case.Q[:nq], k, p)
        assert_same(*a.search_sync(case.Q[:nq], k, p), Do, Io, f"retain {(nq, k, p)}")
        assert_same(*b.search_sync(case.Q[:nq], k, p), Do, Io, f"complement {(nq, k, p)}")


def test_remove_then_add_then_search(case):
    """added records go behind the compacted lists, the emptied one included; add still numbers VectorMeta.id from
    num_vectors"""
    idx, sh = case.copy_of("now", "then_add")
    gpu = vip.load(idx, sh, case.dim, now_secs=NOW)
    rng = np.random.default_rng(5)
    aims = np.array([case.aim["E"]] * 3 + [case.aim["A"]] * 70 + [case.aim["B"]] * 2)
    x = (case.cent[aims] + 1e-3 * rng.standard_normal((len(aims), case.dim))).astype(np.float32)
    orc = O.OracleIndex.load(idx, sh)
    labels = np.array([orc.probe(v, 1)[1][0] for v in x], dtype=np.uint64)
    assert (labels == aims).all()
    ext = np.uint64(50_000_000) + np.arange(len(x), dtype=np.uint64)
    ts = np.uint64(5000) + np.arange(len(x), dtype=np.uint64)
    ids = np.arange(case.n_total, case.n_total + len(x), dtype=np.uint64)
    want = all_bytes(sh)
    for s in np.unique(case.c2s[labels]):
        pick = np.flatnonzero(case.c2s[labels] == s)
        want[f"shard_{int(s)}.bin"] = A.expected_append(sh, str(case.root / "then_add_exp"), int(s), labels[pick], ids[pick],
                                                        ext[pick], ts[pick], x[pick])
    gpu.add(x, ext_ids=ext, timestamps=ts)
    assert all_bytes(sh) == want and gpu.num_vectors == case.n_total + len(x)
    assert list_ext_ids(sh, case.c2s, case.aim["E"]).tolist() == ext[:3].tolist()
    kept_a = list_ext_ids(case.sh, case.c2s, case.aim["A"])
    assert list_ext_ids(sh, case.c2s, case.aim["A"]).tolist() == kept_a.tolist() + ext[3:73].tolist()
    orc = O.OracleIndex.load(idx, sh)
    Q = np.concatenate([x[::5], case.Q[:80]])
    for nq, k, p in [(33, 10, 8), (len(Q), 100, NLIST)]:
        rc, Do, Io = orc.search_batch(Q[:nq], k, p)
        Dg, Ig, cnt, _ = host_search(gpu, Q[:nq], k, p)
        assert_same(Dg, Ig, Do, Io, f"after remove + add {(nq, k, p)}")


# ---- long lists: the prefix search has depth ---------------------------------------------------------------------------
def test_every_third_record_of_two_long_lists(tmp_path):
    """nlist = 2: some 24 blocks per list (more than 4 is what the prefix search needs for a few levels); every third
    record goes, so the sources of a new block span several old ones"""
    rng = np.random.default_rng(31)
    X = rng.standard_normal((N0, 16)).astype(np.float32)
    case = Case(tmp_path, X, lambda c, r: [np.concatenate([l[::3] for l in c.lists])], nlist=2, seed=31,
                shapes=[(33, 10, 2), (300, 100, 2)])
    assert (case.lens > 64 * 4).all() and (case.new_lens == case.lens - (case.lens + 2) // 3).all()
    call = case.calls[0]
    assert call["got"] == call["want"] and sorted(call["names"]) == sorted(call["want"])
    assert call["returned"] == N0 - case.n_total == call["stats"]["n_removed"] and call["stats"]["lists_touched"] == 2
    for nq, k, p in case.shapes:
        rc, Do, Io = case.orc.search_batch(case.Q[:nq], k, p)
        Dg, Ig, cnt, _ = host_search(case.gpu, case.Q[:nq], k, p)
        assert_same(Dg, Ig, Do, Io, f"oracle {(nq, k, p)}")
        assert_same(*case.fresh.search_sync(case.Q[:nq], k, p), Do, Io, f"fresh {(nq, k, p)}")
        assert_same(Dg, Ig, *case.pre[(nq, k, p)], f"filtered before {(nq, k, p)}")


# ---- rank-mode transitions: the add tests' recipes, backwards ------------------------------------------------------------
def check_against_oracle_and_fresh(case, want_mode=None, want_i8=None):
    for nq, k, p in SHAPES[:3]:
        rc, Do, Io = case.orc.search_batch(case.Q[:nq], k, p)
        (Dg, Ig), sa = twice(case.gpu, case.Q[:nq], k, p)
        (Df, If), sf = twice(case.fresh, case.Q[:nq], k, p)
        assert_same(Dg, Ig, Do, Io, f"oracle {(nq, k, p)}")
        assert_same(Df, If, Do, Io, f"fresh {(nq, k, p)}")
        assert (sa["rank_mode"], sa["rank_int8"], sa["group_queries"]) == (sf["rank_mode"], sf["rank_int8"], sf["group_queries"])
    if want_i8 is not None:
        assert sa["rank_int8"] == want_i8, sa
    if want_mode is not None:
        assert want_mode(sa["rank_mode"]), sa
    for call in case.calls:
        assert call["got"] == call["want"]


def descriptors(rng, n):
    centers = rng.integers(40, 216, size=(NLIST, 128))
    return np.clip(centers[rng.integers(0, NLIST, n)] + rng.integers(-40, 41, size=(n, 128)), 0, 255).astype(np.float32)


ODD = 1234      # the row that spoils the base of a transition test


def test_8bit_index_regains_its_int8_image_without_its_fractional_record(tmp_path):
    rng = np.random.default_rng(12)
    X = descriptors(rng, N0)
    X[ODD, 5] += 0.5
    case = Case(tmp_path, X, lambda c, r: [base_ext(N0)[ODD:ODD + 1]], queries="u8", seed=12)
    assert case.pre_stats["rank_int8"] == 0, "the base of this test is meant to rank without an int8 image"
    check_against_oracle_and_fresh(case, want_mode=lambda m: m == 3, want_i8=1)


def test_bf16_exact_index_returns_to_mode_3_without_its_inexact_record(tmp_path):
    rng = np.random.default_rng(13)
    X = rng.integers(-100, 101, size=(N0, 32)).astype(np.float32)      # bf16-exact (|v| <= 128 integers), not 8-bit
    X[ODD, 7] = np.float32(0.1)                                          # 0.1 is not a bf16 value
    case = Case(tmp_path, X, lambda c, r: [base_ext(N0)[ODD:ODD + 1]], queries="int", seed=13)
    assert case.pre_stats["rank_mode"] != 3, "the base of this test is meant not to rank from the hi planes alone"
    check_against_oracle_and_fresh(case, want_mode=lambda m: m == 3)


# ---- no-ops, refusals, wrappers --------------------------------------------------------------------------------------
@pytest.fixture()
def small(tmp_path):
    rng = np.random.default_rng(21)
    X = rng.standard_normal((N0, 16)).astype(np.float32)
    idx, sh = str(tmp_path / "index"), str(tmp_path / "shards")
    O.OracleIndex.build(X, idx, sh, ext_ids=base_ext(N0), timestamps=base_ts(N0), nlist=NLIST, now=NOW)
    return dict(root=tmp_path, X=X, idx=idx, sh=sh, Q=X[:100] + np.float32(0.1))


def test_removing_nothing_changes_nothing(small):
    gpu = vip.load(small["idx"], small["sh"], 16)
    flt = gpu.filter_timestamps(1000, 1499)
    before = all_bytes(small["sh"])
    D0, I0 = gpu.search_sync(small["Q"], 10, 8, filter=flt)
    removed = C.c_uint64(9)
    assert N.lib().vi_indexer_remove_ids(gpu._h, None, 0, C.byref(removed)) == 0 and removed.value == 0     # n == 0
    assert gpu.remove_ids([]) == 0
    assert gpu.remove_ids([1, 2, 3, (1 << 64) - 1, 1]) == 0                                                  # nobody's ids
    assert gpu.retain(gpu.filter_timestamps(0, 1 << 40)) == 0                                                # admits all
    assert gpu.retain(gpu.filter_ids([], exclude=True)) == 0
    D1, I1 = gpu.search_sync(small["Q"], 10, 8, filter=flt)      # the old filter is still this index's
    assert_same(D1, I1, D0, I0, "after removing nothing")
    assert all_bytes(small["sh"]) == before and sorted(os.listdir(small["sh"])) == sorted(before)
    assert gpu.num_vectors == N0 and gpu.remove_stats()["n_removed"] == 0
    assert N.lib().vi_indexer_remove_ids(gpu._h, None, 3, None) == N.VI_ERR_INVALID_INPUT                    # null set, n > 0
    assert N.lib().vi_indexer_retain(gpu._h, None, None) == N.VI_ERR_INVALID_INPUT                            # null keep


def test_refusals_leave_files_and_handle(small):
    before = all_bytes(small["sh"])
    part = vip.load(small["idx"], small["sh"], 16, rank=0, world_size=2)
    for call in (lambda: part.remove_ids(base_ext(10)), lambda: part.retain(part.filter_ids(base_ext(10), exclude=True))):
        with pytest.raises(vip.ViError) as e:
            call()
        assert e.value.status == N.VI_ERR_INVALID_INPUT
    gpu, other = vip.load(small["idx"], small["sh"], 16), vip.load(small["idx"], small["sh"], 16)
    for call in (lambda: gpu.remove_ids(base_ext(N0)),                       # every record
                 lambda: gpu.retain(gpu.filter_ids([], exclude=False)),      # a filter that admits nothing
                 lambda: gpu.retain(other.filter_ids(base_ext(10)))):        # a filter of another handle
        with pytest.raises(vip.ViError) as e:
            call()
        assert e.value.status == N.VI_ERR_INVALID_INPUT
    assert all_bytes(small["sh"]) == before and sorted(os.listdir(small["sh"])) == sorted(before)
    assert gpu.num_vectors == N0
    flt = gpu.filter_ids(base_ext(10))                                       # the handle still has its index
    assert flt.num_allowed == 10 and gpu.retain(flt) == N0 - 10 and gpu.num_vectors == 10


def test_python_wrappers_equal_the_c_abi_path(small):
    gone = np.concatenate([base_ext(N0)[::7], np.array([5, 6], dtype=np.uint64)])
    n_gone = len(base_ext(N0)[::7])
    roots = {}
    for name in ("abi", "index", "indexer", "faiss"):
        roots[name] = small["root"] / name
        shutil.copytree(small["idx"], roots[name] / "index")
        shutil.copytree(small["sh"], roots[name] / "shards")
    dirs = lambda name: (str(roots[name] / "index"), str(roots[name] / "shards"))  # noqa: E731
    # the C ABI itself
    abi = vip.load(*dirs("abi"), 16)
    removed = C.c_uint64(0)
    N.check(N.lib().vi_indexer_remove_ids(abi._h, N.ptr(gone), len(gone), C.byref(removed)))
    assert removed.value == n_gone and abi.num_vectors == N0 - n_gone
    Da, Ia = abi.search_sync(small["Q"], 10, 8)
    orc = O.OracleIndex.load(*dirs("abi"))
    rc, Do, Io = orc.search_batch(small["Q"], 10, 8)
    assert_same(Da, Ia, Do, Io, "C entry")
    # VectorIndex.remove_ids
    vx = vip.load(*dirs("index"), 16)
    assert vx.remove_ids(gone.tolist()) == n_gone
    assert all_bytes(dirs("index")[1]) == all_bytes(dirs("abi")[1])
    assert_same(*vx.search_sync(small["Q"], 10, 8), Da, Ia, "VectorIndex.remove_ids")
    # VectorIndexer.remove_records
    vi = VectorIndexer.load(VectorIndexerConfig(16, *dirs("indexer")))
    req = vi.search_request(small["Q"][0]).with_k(10).with_n_probe(8).with_timestamp_range(0, 1 << 40)
    assert len(vi.search(req)) == 10                                   # (caches a filter of the old index)
    assert vi.remove_records(gone) == n_gone
    assert all_bytes(dirs("indexer")[1]) == all_bytes(dirs("abi")[1])
    for qi in (0, 30):
        got = vi.search(vi.search_request(small["Q"][qi]).with_k(10).with_n_probe(8).with_timestamp_range(0, 1 << 40))
        assert [r.external_id for r in got] == Ia[qi].tolist()
        assert np.array_equal(bits([r.distance for r in got]), bits(Da[qi]))
    assert vi.remove_records([]) == 0
    # FaissStyleAdapter.remove_ids
    fa = FaissStyleAdapter(vip.load(*dirs("faiss"), 16))
    fa.nprobe = 8
    assert fa.ntotal == N0
    assert fa.remove_ids(gone) == n_gone and fa.ntotal == N0 - n_gone
    assert all_bytes(dirs("faiss")[1]) == all_bytes(dirs("abi")[1])
    assert_same(*fa.search(small["Q"], 10), Da, Ia, "FaissStyleAdapter.remove_ids")
    assert fa.remove_ids(gone) == 0 and fa.ntotal == N0 - n_gone
