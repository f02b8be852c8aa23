"""GPU: vi_indexer_add_records — records appended to a built index, in the shard files and in the resident index.

The contract: afterwards the index is the one the reference would search if each new record had been appended to the
inverted list of its nearest kept centroid (the first probe of the coarse step).  Everything expected comes from the
untouched oracle: the labels from OracleIndex.probe(x, 1), the shard files from shard_get + numpy append + shard_save
(add_cases.expected_append), the search results from a fresh OracleIndex.load of the directories the handle wrote.  Ids,
distance bits, counts and padding must match exactly; the files byte for byte."""
import os
import shutil

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from vector_indexer_py import _native as N
from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig, VectorRecord
from vector_indexer_py.harness import FaissStyleAdapter

import add_cases as A

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000
N0, NLIST = 3000, 20
# the issue's shapes, and one whose k exceeds the probed list (padding; the sort-everything path)
SHAPES = [(1, 1, 1), (33, 10, 8), (300, 100, 20), (33, 400, 1)]
NEW_EXT, NEW_TS = 50_000_000, 5000      # external ids / timestamps of added records: apart from the base's


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def base_ext(n):
    return np.uint64(10_000_000) + np.uint64(3) * np.arange(n, dtype=np.uint64)


def base_ts(n):
    return np.uint64(1000) + (np.arange(n, dtype=np.uint64) * np.uint64(7919)) % np.uint64(1000)


def shard_files(sh):
    return sorted(f for f in os.listdir(sh) if f.startswith("shard_"))


def all_bytes(sh):
    return {f: open(os.path.join(sh, f), "rb").read() for f in shard_files(sh)}


def oracle_labels(orc, x):
    out = np.zeros(len(x), dtype=np.uint64)
    for i, v in enumerate(x):
        rc, p = orc.probe(v, 1)
        assert rc == O.ORC_OK and len(p) == 1
        out[i] = p[0]
    return out


def expected_files(idx_c2s, sh, exp_dir, labels, ids, ext, ts, x):
    """every shard file after the append, by the oracle's reader and writer alone; untouched shards as they are"""
    want = all_bytes(sh)
    for s in np.unique(idx_c2s[labels]):
        pick = np.flatnonzero(idx_c2s[labels] == s)
        want[f"shard_{int(s)}.bin"] = A.expected_append(sh, exp_dir, int(s), labels[pick], ids[pick], ext[pick], ts[pick], x[pick])
    return want


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
    """the second of two equal searches and its stats: the group size of a batch follows what the previous batch of its
    shape measured on the handle, so handles with different pasts compare from the second batch on"""
    gpu.search_sync(Q, k, p)
    out = gpu.search_sync(Q, k, p)
    return out, gpu.last_stats()


def assert_same(Dg, Ig, Do, Io, what):
    bad = np.nonzero((Ig != Io).any(axis=1) | (bits(Dg) != bits(Do)).any(axis=1))[0]
    assert bad.size == 0, (f"{what}: {bad.size} queries differ, first {bad[0]}: got {Ig[bad[0]][:8]} {Dg[bad[0]][:8]} "
                           f"expected {Io[bad[0]][:8]} {Do[bad[0]][:8]}")


class Case:
    """a base index written by the oracle, opened by the product, and two add calls; what the tests compare is recorded
    while it is made"""

    def __init__(self, root, X, make_batches, queries="real", seed=0):
        rng = np.random.default_rng(seed)
        self.X = np.ascontiguousarray(X, dtype=np.float32)
        self.dim = X.shape[1]
        self.root, self.idx, self.sh = root, str(root / "index"), str(root / "shards")
        O.OracleIndex.build(self.X, self.idx, self.sh, ext_ids=base_ext(len(X)), timestamps=base_ts(len(X)), nlist=NLIST, now=NOW)
        self.base_orc = O.OracleIndex.load(self.idx, self.sh)
        self.cent, self.c2s = self.base_orc.centroids()
        self.lens = np.array([self.base_orc.list_len(c) for c in range(len(self.cent))], dtype=np.int64)
        self.index_bin = open(os.path.join(self.idx, "index.bin"), "rb").read()
        self.gpu = vip.load(self.idx, self.sh, self.dim, now_secs=NOW)
        assert self.gpu.num_vectors == len(X)
        # made before any add: two filters (to be rejected later) and the results the deny set must bring back
        self.old_ts_filter = self.gpu.filter_timestamps(0, 1 << 40)
        self.old_id_filter = self.gpu.filter_ids(base_ext(len(X))[:100])
        self.batches = make_batches(self, rng)
        added = np.concatenate([b[0] for b in self.batches])
        m = min(100, len(added))
        near = self.X[rng.integers(0, len(X), 300 - m)]
        near = near + (0.3 * rng.standard_normal(near.shape) if queries == "real" else rng.integers(-3, 4, size=near.shape))
        Q = np.concatenate([added[rng.choice(len(added), m, replace=False)], near]).astype(np.float32)
        if queries != "real":       # whole numbers ("u8": in 0..254, what the int8 rank kernel takes)
            Q = np.rint(Q)
            Q = np.clip(Q, 0, 254) if queries == "u8" else Q
        self.Q = np.ascontiguousarray(Q[rng.permutation(300)], dtype=np.float32)
        self.pre = {}
        for nq, k, p in SHAPES:
            self.pre[(nq, k, p)] = self.gpu.search_sync(self.Q[:nq], k, p)
            if (nq, k, p) == SHAPES[2]:
                self.pre_stats = self.gpu.last_stats()
        # ---- the adds ----
        self.calls, n_before = [], len(X)
        for ci, (x, ext, ts) in enumerate(self.batches):
            orc = O.OracleIndex.load(self.idx, self.sh)
            labels = oracle_labels(orc, x)
            ids = np.arange(n_before, n_before + len(x), dtype=np.uint64)
            want = expected_files(self.c2s, self.sh, str(root / f"expected{ci}"), labels, ids, ext, ts, x)
            self.gpu.add(x, ext_ids=ext, timestamps=ts)
            self.calls.append(dict(want=want, got=all_bytes(self.sh), names=os.listdir(self.sh), stats=self.gpu.add_stats(),
                                   index_bin=open(os.path.join(self.idx, "index.bin"), "rb").read(), labels=labels,
                                   n_total=self.gpu.num_vectors))
            n_before += len(x)
        self.n_total = n_before
        self.added_x, self.added_ext = added, np.concatenate([b[1] for b in self.batches])
        self.orc = O.OracleIndex.load(self.idx, self.sh)
        self._fresh = None

    @property
    def fresh(self):
        if self._fresh is None:
            self._fresh = vip.load(self.idx, self.sh, self.dim)
        return self._fresh


def near_centroids(case, rng, counts, noise):
    """vectors aimed at lists: centroid + small noise, interleaved and shuffled"""
    aims = rng.permutation(np.repeat(np.array(list(counts), dtype=np.int64), list(counts.values())))
    return (case.cent[aims] + noise * rng.standard_normal((len(aims), case.dim))).astype(np.float32), aims


def layout_batches(case, rng):
    """call 1: list A filled to the end of its last block, B one past it, C 130 records, D one; call 2: one more to A (a
    block behind an exactly full one) and 70 to D"""
    ragged = [int(l) for l in np.flatnonzero(case.lens % 64 != 0)]
    a, b, c, d = ragged[0], ragged[len(ragged) // 2], ragged[-1], ragged[1]
    assert len({a, b, c, d}) == 4
    case.aim = dict(A=a, B=b, C=c, D=d)
    r = case.lens % 64
    plan = [{a: 64 - int(r[a]), b: 64 - int(r[b]) + 1, c: 130, d: 1}, {a: 1, d: 70}]
    out, at = [], 0
    for counts in plan:
        x, aims = near_centroids(case, rng, counts, 1e-3)
        n = len(x)
        out.append((x, np.uint64(NEW_EXT + at) + np.arange(n, dtype=np.uint64), np.uint64(NEW_TS + at) + np.arange(n, dtype=np.uint64)))
        case.plan = plan
        at += n
    return out


@pytest.fixture(scope="module", params=[3, 16, 100, 128, 200], ids=lambda d: f"D{d}")
def case(request, tmp_path_factory):
    d = request.param
    rng = np.random.default_rng(d)
    X = rng.standard_normal((N0, d)).astype(np.float32)
    return Case(tmp_path_factory.mktemp(f"add{d}"), X, layout_batches, seed=d)


def test_layout_batch_is_what_it_was_meant_to_be(case):
    """the labels come from the oracle's probe; this pins that they realise the block cases the batch was made for"""
    for call, counts in zip(case.calls, case.plan):
        got = {int(l): int(n) for l, n in zip(*np.unique(call["labels"], return_counts=True))}
        assert got == counts
    r = case.lens % 64
    assert (case.lens[case.aim["A"]] + case.plan[0][case.aim["A"]]) % 64 == 0 and r[case.aim["B"]] != 0


def test_files_are_byte_identical_after_each_call(case):
    n = N0
    for call, batch in zip(case.calls, case.batches):
        n += len(batch[0])
        assert sorted(call["got"]) == sorted(call["want"])
        for f in call["want"]:
            assert call["got"][f] == call["want"][f], f
        assert sorted(call["names"]) == sorted(call["want"]), "a temporary file was left behind"
        assert call["index_bin"] == case.index_bin
        assert call["n_total"] == n
        st = call["stats"]
        touched = np.unique(call["labels"])
        assert st["n"] == len(batch[0]) and st["lists_touched"] == len(touched)
        assert st["shards_rewritten"] == len(np.unique(case.c2s[touched]))
        assert st["bytes_written"] == sum(len(call["want"][f"shard_{int(s)}.bin"]) for s in np.unique(case.c2s[touched]))


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


def test_fresh_load_gives_the_same_index(case):
    assert case.fresh.num_vectors == case.gpu.num_vectors == case.n_total
    for nq, k, p in SHAPES:
        (Da, Ia), sa = twice(case.gpu, case.Q[:nq], k, p)
        (Df, If), sf = twice(case.fresh, case.Q[:nq], k, p)
        assert_same(Da, Ia, Df, If, f"fresh load {(nq, k, p)}")
        for f in ("rank_mode", "rank_int8", "group_queries", "scanned_vectors"):
            assert sa[f] == sf[f], (f, (nq, k, p), sa[f], sf[f])


def test_stored_vectors_and_radius_zero(case):
    x, ext = case.added_x[::37], case.added_ext[::37]
    D, I, cnt, V = host_search(case.gpu, x, 1, 1, include_vectors=True)
    assert (cnt == 1).all() and (bits(D) == 0).all()
    assert np.array_equal(bits(V[:, 0, :]), bits(x))
    lims, Dr, Ir = case.gpu.range_search_sync(x, 0.0, 1)
    for i in range(len(x)):
        assert int(ext[i]) in Ir[int(lims[i]):int(lims[i + 1])].tolist(), i
    assert (bits(Dr) == 0).all()


def test_filters_across_an_add(case):
    q = case.Q[:33]
    for old in (case.old_ts_filter, case.old_id_filter):
        with pytest.raises(vip.ViError) as e:
            case.gpu.search_sync(q, 10, 8, filter=old)
        assert e.value.status == N.VI_ERR_INVALID_INPUT
    n_added = len(case.added_x)
    new_only = case.gpu.filter_timestamps(NEW_TS, NEW_TS + n_added - 1)
    assert new_only.num_allowed == n_added
    D, I = case.gpu.search_sync(q, 10, NLIST, filter=new_only)
    assert np.isin(I[I >= 0], case.added_ext.astype(np.int64)).all() and (I >= 0).any()
    deny = case.gpu.filter_ids(case.added_ext, exclude=True)
    assert deny.num_allowed == N0
    for (nq, k, p), (Dp, Ip) in case.pre.items():
        Dg, Ig = case.gpu.search_sync(case.Q[:nq], k, p, filter=deny)
        assert_same(Dg, Ig, Dp, Ip, f"deny set of the added ids {(nq, k, p)}")


# ---- rank-mode transitions --------------------------------------------------------------------------------------------
def one_list_batches(*specs):
    """specs: per call a function (case, rng) -> x"""
    def make(case, rng):
        out, at = [], 0
        for spec in specs:
            x = np.ascontiguousarray(spec(case, rng), dtype=np.float32)
            n = len(x)
            out.append((x, np.uint64(NEW_EXT + at) + np.arange(n, dtype=np.uint64), np.uint64(NEW_TS + at) + np.arange(n, dtype=np.uint64)))
            at += n
        return out
    return make


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


def test_8bit_index_keeps_its_int8_image_with_integer_records(tmp_path):
    rng = np.random.default_rng(11)
    X = descriptors(rng, N0)
    case = Case(tmp_path, X, one_list_batches(lambda c, r: descriptors(r, 90)), queries="u8", seed=11)
    check_against_oracle_and_fresh(case, want_mode=lambda m: m == 3, want_i8=1)


def test_8bit_index_loses_its_int8_image_with_one_fractional_record(tmp_path):
    rng = np.random.default_rng(12)
    X = descriptors(rng, N0)

    def one_fractional(c, r):
        x = descriptors(r, 1)
        x[0, 5] += 0.5
        return x
    case = Case(tmp_path, X, one_list_batches(lambda c, r: descriptors(r, 90), one_fractional), queries="u8", seed=12)
    assert case.pre_stats["rank_int8"] == 1, "the base of this test is meant to rank with its int8 image"
    check_against_oracle_and_fresh(case, want_i8=0)


def test_bf16_exact_index_leaves_mode_3_with_one_inexact_record(tmp_path):
    rng = np.random.default_rng(13)
    X = rng.integers(-100, 101, size=(N0, 32)).astype(np.float32)      # bf16-exact (|v| <= 128 integers), not 8-bit

    def one_inexact(c, r):
        x = r.integers(-100, 101, size=(1, 32)).astype(np.float32)
        x[0, 7] = np.float32(0.1)                                        # 0.1 is not a bf16 value
        return x
    case = Case(tmp_path, X, one_list_batches(one_inexact), queries="int", seed=13)
    assert case.pre_stats["rank_mode"] == 3, "the base of this test is meant to rank from the hi planes alone"
    check_against_oracle_and_fresh(case, want_mode=lambda m: m != 3 and m >= 1)


# ---- defaults, no-ops, refusals, wrappers --------------------------------------------------------------------------
@pytest.fixture()
def small(tmp_path):
    rng = np.random.default_rng(21)
    X = rng.standard_normal((N0, 16)).astype(np.float32)
    idx, sh = str(tmp_path / "index"), str(tmp_path / "shards")
    orc = O.OracleIndex.build(X, idx, sh, ext_ids=base_ext(N0), timestamps=base_ts(N0), nlist=NLIST, now=NOW)
    cent, c2s = orc.centroids()
    x = (cent[rng.integers(0, len(cent), 75)] + 1e-3 * rng.standard_normal((75, 16))).astype(np.float32)
    return dict(root=tmp_path, X=X, idx=idx, sh=sh, orc=orc, c2s=c2s, x=x, Q=np.concatenate([x[:20], X[:80]]))


def test_default_ids_and_timestamps(small):
    """ext_ids None: N_before + i; timestamps None, or a 0 entry: now"""
    gpu = vip.load(small["idx"], small["sh"], 16, now_secs=NOW + 5)
    x = small["x"]
    labels = oracle_labels(small["orc"], x)
    ids = np.arange(N0, N0 + 75, dtype=np.uint64)
    want = expected_files(small["c2s"], small["sh"], str(small["root"] / "e1"), labels, ids, ids, np.full(75, NOW + 5, dtype=np.uint64), x)
    gpu.add(x)
    assert all_bytes(small["sh"]) == want
    ts = np.arange(75, dtype=np.uint64) * np.uint64(2)      # ts[0] == 0: now
    ids2 = ids + np.uint64(75)
    want_ts = np.where(ts == 0, np.uint64(NOW + 5), ts)
    want = expected_files(small["c2s"], small["sh"], str(small["root"] / "e2"), labels, ids2, ids2, want_ts, x)
    gpu.add(x, timestamps=ts)
    assert all_bytes(small["sh"]) == want
    assert gpu.num_vectors == N0 + 150


def test_adding_nothing_changes_nothing(small):
    gpu = vip.load(small["idx"], small["sh"], 16)
    flt = gpu.filter_timestamps(1000, 1499)
    before = all_bytes(small["sh"])
    D0, I0 = gpu.search_sync(small["Q"], 10, 8, filter=flt)
    gpu.add(np.zeros((0, 16), dtype=np.float32))
    assert N.lib().vi_indexer_add_records(gpu._h, None, None, None, 0) == 0
    D1, I1 = gpu.search_sync(small["Q"], 10, 8, filter=flt)      # the old filter is still this index's
    assert_same(D1, I1, D0, I0, "after an empty add")
    assert all_bytes(small["sh"]) == before and gpu.num_vectors == N0


def test_partitioned_handle_refuses(small):
    part = vip.load(small["idx"], small["sh"], 16, rank=0, world_size=2)
    before = all_bytes(small["sh"])
    with pytest.raises(vip.ViError) as e:
        part.add(small["x"])
    assert e.value.status == N.VI_ERR_INVALID_INPUT
    assert all_bytes(small["sh"]) == before and sorted(os.listdir(small["sh"])) == sorted(before)


def test_python_wrappers_equal_the_c_abi_path(small):
    x, ext = small["x"], np.uint64(NEW_EXT) + np.arange(75, dtype=np.uint64)
    ts = np.uint64(NEW_TS) + np.arange(75, dtype=np.uint64)
    roots = {}
    for name in ("abi", "indexer", "faiss"):
        roots[name] = small["root"] / name
        shutil.copytree(small["idx"], roots[name] / "index")
        shutil.copytree(small["sh"], roots[name] / "shards")
    dirs = lambda name: (str(roots[name] / "index"), str(roots[name] / "shards"))  # noqa: E731
    # the C ABI itself
    abi = vip.load(*dirs("abi"), 16, now_secs=NOW)
    N.check(N.lib().vi_indexer_add_records(abi._h, N.ptr(ext), N.ptr(x), N.ptr(ts), 75))
    Da, Ia = abi.search_sync(small["Q"], 10, 8)
    # VectorIndexer.add_records
    cfg = VectorIndexerConfig(16, *dirs("indexer"), now_secs=NOW)
    vi = VectorIndexer.load(cfg)
    req = vi.search_request(small["Q"][0]).with_k(10).with_n_probe(8).with_timestamp_range(0, 1 << 40)
    assert len(vi.search(req)) == 10                                   # (caches a filter of the old index)
    vi.add_records([VectorRecord(int(ext[i]), x[i].tolist(), int(ts[i])) for i in range(75)])
    assert all_bytes(dirs("indexer")[1]) == all_bytes(dirs("abi")[1])
    for qi in (0, 30):
        got = vi.search(vi.search_request(small["Q"][qi]).with_k(10).with_n_probe(8).with_timestamp_range(0, 1 << 40))
        assert [r.external_id for r in got] == Ia[qi].tolist()
        assert np.array_equal(bits([r.distance for r in got]), bits(Da[qi]))
    with pytest.raises(vip.ViError):
        vi.add_records([VectorRecord(1, [0.0] * 15)])
    # FaissStyleAdapter.add_with_ids (timestamps: now)
    fa = FaissStyleAdapter(vip.load(*dirs("faiss"), 16, now_secs=NOW))
    fa.nprobe = 8
    fa.add_with_ids(x, ext)
    Df, If = fa.search(small["Q"], 10)
    assert_same(Df, If, Da, Ia, "FaissStyleAdapter.add_with_ids")
    fa.add(x[:3])
    assert fa._idx.num_vectors == N0 + 78
    D3, I3 = fa.search(x[:3], 2)
    assert (np.sort(I3, axis=1) == np.stack([np.arange(N0 + 75, N0 + 78), ext[:3].astype(np.int64)], axis=1)).all()
