"""GPU: reading records back from a resident index — vi_indexer_get_records (by external id) and vi_indexer_export_records
(a range of the list order), host and device forms, on whole and partitioned handles, after updates and from threads.

The oracle is the shard files read on the CPU: the expected list order is the concatenation over l = 0 .. k'-1 of
oracle_lib.shard_get(shards, c2s[l], [l]), with where = (l << 32) | position.  Every comparison is exact: ids, counts,
timestamps and where as integers, vectors as uint32 bit patterns."""
import shutil
import threading

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from vector_indexer_py import _native as N
from test_id_filter_gpu import ext_ids_for, timestamps_for

pytestmark = pytest.mark.gpu

NOW = 1_700_000_000
U64_MAX = (1 << 64) - 1
NONE = np.uint64(U64_MAX)
SHAPES = [(3000, 17, 24), (2000, 128, 16), (1500, 130, 8), (700, 1, 4), (900, 3, 1)]
HAND_LENS = [1, 63, 64, 65, 0, 0, 200, 0, 129]
SET_NAMES = ["empty", "one", "all", "n63", "n64", "n65", "mostly_absent", "repeated", "odd"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


class Order:
    """the records of an index in list order, read from its files by the oracle's reader"""

    def __init__(self, idx, sh):
        _, c2s = O.OracleIndex.load(idx, sh).centroids()
        ext, ts, X, where, self.lens = [], [], [], [], []
        for l in range(len(c2s)):
            rc, lists = O.shard_get(sh, int(c2s[l]), [l])
            assert rc == O.ORC_OK
            _, cent, metas, vecs = lists[0]
            n = len(metas)
            ext.append(metas[:, 1]), ts.append(metas[:, 2]), X.append(vecs.reshape(n, len(cent)))
            where.append((np.uint64(l) << np.uint64(32)) + np.arange(n, dtype=np.uint64))
            self.lens.append(n)
        self.ext, self.ts, self.where = (u64(np.concatenate(a)) for a in (ext, ts, where))
        self.X = np.ascontiguousarray(np.concatenate(X), dtype=np.float32)
        self.n, self.dim = self.X.shape
        self._by_id = np.argsort(self.ext, kind="stable")   # (stable: among equal ids, list order)
        self._sorted = self.ext[self._by_id]
        for a in (self.ext, self.ts, self.where, self.X):
            a.setflags(write=False)

    def subset(self, keep):
        """the records of `keep` (a mask) alone, still in list order: what one rank of a partitioned index holds"""
        o = Order.__new__(Order)
        o.ext, o.ts, o.where, o.X = self.ext[keep], self.ts[keep], self.where[keep], self.X[keep]
        o.n, o.dim = o.X.shape
        o._by_id = np.argsort(o.ext, kind="stable")
        o._sorted = o.ext[o._by_id]
        return o

    def get(self, ids):
        """(counts, X, timestamps, where) a get of `ids` must return"""
        ids = u64(ids)
        lo, hi = np.searchsorted(self._sorted, ids, "left"), np.searchsorted(self._sorted, ids, "right")
        cnt = (hi - lo).astype(np.uint32)
        hit = cnt > 0
        row = self._by_id[np.minimum(lo, max(self.n - 1, 0))] if self.n else np.zeros(len(ids), dtype=np.int64)
        X = np.zeros((len(ids), self.dim), dtype=np.float32)
        ts, where = np.zeros(len(ids), dtype=np.uint64), np.full(len(ids), NONE, dtype=np.uint64)
        X[hit], ts[hit], where[hit] = self.X[row[hit]], self.ts[row[hit]], self.where[row[hit]]
        return cnt, X, ts, where


def same_get(got, want, what):
    for name, g, w in zip(("counts", "X", "timestamps", "where"), got, want):
        if name == "X":
            g, w = bits(g), bits(w)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1)) if len(g) else np.zeros(0, dtype=np.int64)
        assert g.shape == w.shape and bad.size == 0, (f"{what}: {name} differs in {bad.size} rows, first {bad[:1]}: "
                                                      f"got {g[bad[:1]]} expected {w[bad[:1]]}")


def same_export(got, want, lo, hi, what):
    e, X, t, w = got
    assert np.array_equal(e, want.ext[lo:hi]), what
    assert np.array_equal(bits(X), bits(want.X[lo:hi])), what
    assert np.array_equal(t, want.ts[lo:hi]) and np.array_equal(w, want.where[lo:hi]), what


def special_values(X):
    X = np.array(X, dtype=np.float32)
    X[5, 0], X[6, 0], X[7, -1] = -0.0, 1e-42, -1e-45     # a negative zero and two denormals
    return X


class Fx:
    def __init__(self, root, idx, sh, dim, seed):
        self.root, self.idx, self.sh, self.dim = root, idx, sh, dim
        self.want = Order(idx, sh)
        self.n = self.want.n
        self.gpu = vip.load(idx, sh, dim)
        assert self.gpu.num_vectors == self.n
        self.sets = self.make_sets(np.random.default_rng(seed))

    def make_sets(self, rng):
        ext, n = np.unique(self.want.ext), self.n
        pick = lambda m: ext[rng.choice(len(ext), min(m, len(ext)), replace=False)]  # noqa: E731
        absent = (np.uint64(1) << np.uint64(50)) + np.arange(19_400, dtype=np.uint64) * np.uint64(0x10000001)
        flipped = pick(300) ^ (np.uint64(1) << np.uint64(40))
        flipped = flipped[~np.isin(flipped, ext)]
        near = u64([1, U64_MAX - 1, 1 << 63, U64_MAX ^ (1 << 40)])
        near = near[~np.isin(near, ext)]
        assert not np.isin(absent, ext).any() and flipped.size >= 100 and near.size >= 3
        sets = {"empty": np.zeros(0, dtype=np.uint64), "one": ext[17:18].copy(), "all": rng.permutation(self.want.ext),
                "n63": pick(63), "n64": pick(64), "n65": pick(65),
                "mostly_absent": rng.permutation(np.concatenate([pick(600), absent])),
                "repeated": np.full(20_000, ext[len(ext) // 2], dtype=np.uint64),
                "odd": np.concatenate([u64([0, U64_MAX]), near, flipped])}
        for s in sets.values():
            s.setflags(write=False)
        return sets


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "N%d_D%d_L%d" % s)
def built(request, tmp_path_factory):
    """an index built by the oracle: ids as in the id-filter tests plus one 2^64 - 1, values with -0.0 and denormals"""
    n, d, nlist = request.param
    rng = np.random.default_rng(n + d)
    X = special_values(rng.standard_normal((n, d)))
    ext = ext_ids_for(n)
    ext[n // 2] = U64_MAX
    assert np.unique(ext).size == n and (ext == 0).sum() == 1
    root = tmp_path_factory.mktemp("get%d" % d)
    idx, sh = str(root / "index"), str(root / "shards")
    O.OracleIndex.build(X, idx, sh, ext_ids=ext, timestamps=timestamps_for(n), nlist=nlist, now=NOW)
    return Fx(root, idx, sh, d, seed=n)


DUP3, DUP64 = 777_000_000_777, 888_000_000_888


def hand_made(root, lens, d, duplicates):
    """nine lists of exactly `lens` records: the oracle writes an index of nine lists, then every shard file is rewritten
    through the oracle's writer with lists of these lengths (an empty list last in its file)"""
    rng = np.random.default_rng(77)
    centres = 8.0 * rng.standard_normal((9, d))
    X0 = (centres[np.arange(900) % 9] + 0.1 * rng.standard_normal((900, d))).astype(np.float32)
    idx, sh = str(root / "index"), str(root / "shards")
    orc = O.OracleIndex.build(X0, idx, sh, nlist=9, now=NOW)
    cent, c2s = orc.centroids()
    assert len(c2s) == len(lens)
    total = sum(lens)
    X = special_values(rng.standard_normal((total, d)))
    ext = ext_ids_for(total) + np.uint64(1)
    ext[0], ext[400] = 0, U64_MAX
    ts = timestamps_for(total)
    off = np.concatenate([[0], np.cumsum(lens)])
    if duplicates:
        ext[off[2]:off[3]] = DUP64
        for l, p in ((1, 40), (3, 64), (8, 128), (6, 70), (6, 199)):
            ext[off[l] + p] = DUP3
    for s in sorted(set(int(x) for x in c2s)):
        mine = [l for l in range(9) if int(c2s[l]) == s]
        mine.sort(key=lambda l: (lens[l] == 0, l))
        lists = [(np.arange(off[l], off[l + 1], dtype=np.uint64), ext[off[l]:off[l + 1]], ts[off[l]:off[l + 1]],
                  X[off[l]:off[l + 1]]) for l in mine]
        assert O.shard_save(sh, s, d, mine, cent[mine], lists) == O.ORC_OK
    fx = Fx(root, idx, sh, d, seed=7)
    assert fx.want.lens == lens and fx.n == total
    return fx


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    """nine lists of 1, 63, 64, 65, 0, 0, 200, 0, 129 records.  DUP3 is carried by one record of lists 1, 3 and 8 and by
    two of list 6; DUP64 by every record of list 2."""
    return hand_made(tmp_path_factory.mktemp("hand"), HAND_LENS, 20, duplicates=True)


def raw_get(ix, ids, outputs="cvtw", dim=None):
    """vi_indexer_get_records with the outputs named in `outputs` (c, v, t, w), NULL for the others; poisoned buffers"""
    ids = u64(ids)
    n, dim = ids.size, dim or ix.dimension
    c = np.full(n, 0xABCD, dtype=np.uint32) if "c" in outputs else None
    v = np.full((n, dim), np.float32(7.5)) if "v" in outputs else None
    t = np.full(n, 12345, dtype=np.uint64) if "t" in outputs else None
    w = np.full(n, 54321, dtype=np.uint64) if "w" in outputs else None
    N.check(N.lib().vi_indexer_get_records(ix._h, N.ptr(ids) if n else None, n, N.ptr(c), N.ptr(v), N.ptr(t), N.ptr(w)))
    return c, v, t, w


def device_call(call, shapes, outputs, skew=0):
    """runs call(pointers) with one poisoned device buffer per (letter, shape, dtype) of `shapes` whose letter is in
    `outputs` (0 for the others) and returns the buffers' contents (None for the others).  Device memory comes from
    hiprt.Hip: torch would bring a second HIP runtime into the test process, which does not see the GPU.  skew: bytes
    the float buffer starts past its 256-byte aligned allocation."""
    from hiprt import Hip
    hip = Hip()
    try:
        ptrs = []
        for ch, shape, dt in shapes:
            n = int(np.prod(shape))
            off = skew if dt == np.float32 else 0
            ptrs.append(hip.upload(np.full(n + off // 4 + 1, 0x4B, dtype=np.uint8).repeat(np.dtype(dt).itemsize).view(dt)) + off
                        if ch in outputs else 0)
        call(hip, ptrs)
        return tuple(hip.download(p, shape, dt) if p else None for p, (ch, shape, dt) in zip(ptrs, shapes))
    finally:
        hip.close()


def device_get(ix, ids, outputs="cvtw", skew=0):
    """vi_indexer_get_records_device: ids and outputs in device memory"""
    ids = u64(ids)
    n = ids.size
    shapes = [("c", (n,), np.uint32), ("v", (n, ix.dimension), np.float32), ("t", (n,), np.uint64), ("w", (n,), np.uint64)]
    return device_call(lambda hip, p: ix.get_device(hip.upload(ids) if n else 0, n, *p), shapes, outputs, skew)


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SET_NAMES)
def test_every_request_set_host_and_device(built, name):
    ids = built.sets[name]
    want = built.want.get(ids)
    present = int(np.isin(ids, built.want.ext).sum())
    if name == "mostly_absent":
        assert ids.size == 20_000 and present == 600
    if name == "odd":
        assert present == 2 and ids[0] == 0 and ids[1] == NONE      # 0 and 2^64 - 1 are stored; no near-miss is
    if name == "repeated":
        assert ids.size == 20_000 and present == 20_000
    got = built.gpu.get(ids)
    same_get(got, want, f"host {name}")
    assert int((got[0] > 0).sum()) == present
    if ids.size:
        assert built.gpu.fetch_stats()["n"] == ids.size and built.gpu.fetch_stats()["n_found"] == present
        assert built.gpu.fetch_stats()["slots_scanned"] == built.n
    absent = got[0] == 0
    assert (got[3][absent] == NONE).all() and (got[2][absent] == 0).all() and (bits(got[1][absent]) == 0).all()
    same_get(device_get(built.gpu, ids), got, f"device {name}")


def test_every_combination_of_null_outputs(built):
    ids = np.concatenate([built.sets["n65"], built.sets["odd"][:40], built.sets["n65"][:7]])
    want = dict(zip("cvtw", built.want.get(ids)))
    for mask in range(16):
        outputs = "".join(ch for i, ch in enumerate("cvtw") if mask >> i & 1)
        for form, call in (("host", raw_get), ("device", device_get)):
            got = dict(zip("cvtw", call(built.gpu, ids, outputs)))
            for ch in "cvtw":
                if ch not in outputs:
                    assert got[ch] is None
                elif ch == "v":
                    assert np.array_equal(bits(got[ch]), bits(want[ch])), (form, outputs)
                else:
                    assert np.array_equal(got[ch], want[ch]), (form, outputs, ch)
    for skew in (4, 8):    # rows that do not start on 16 bytes: the element-wise stores
        got = device_get(built.gpu, ids, "cv", skew=skew)
        assert np.array_equal(got[0], want["c"]) and np.array_equal(bits(got[1]), bits(want["v"])), skew
    counts, X, _, _ = built.gpu.get(ids, vectors=False)        # "contains / how many"
    assert X is None and np.array_equal(counts, want["c"])


def test_n_zero_reads_and_writes_nothing(built):
    L = N.lib()
    poison = np.full(4, 0xABCD, dtype=np.uint32)
    assert L.vi_indexer_get_records(built.gpu._h, None, 0, N.ptr(poison), None, None, None) == N.VI_OK
    assert L.vi_indexer_get_records_device(built.gpu._h, None, 0, None, None, None, None) == N.VI_OK
    assert (poison == 0xABCD).all()
    assert L.vi_indexer_get_records(built.gpu._h, None, 3, N.ptr(poison), None, None, None) == N.VI_ERR_INVALID_INPUT
    assert L.vi_indexer_get_records(built.gpu._h, N.ptr(poison), (1 << 40) + 1, None, None, None, None) == N.VI_ERR_INVALID_INPUT
    c, X, t, w = built.gpu.get([])
    assert c.size == 0 and X.shape == (0, built.dim)


def export_ranges(fx):
    n = fx.n
    return [(0, n), (0, 0), (n, 0), (63, 2), (64, 64), (n - 1, 1)]


def device_export(ix, first, count, outputs="evtw", skew=0):
    """vi_indexer_export_records_device: outputs in device memory"""
    shapes = [("e", (count,), np.uint64), ("v", (count, ix.dimension), np.float32), ("t", (count,), np.uint64),
              ("w", (count,), np.uint64)]
    return device_call(lambda hip, p: ix.export_device(first, count, *p), shapes, outputs, skew)


def check_exports(fx, ranges):
    for first, count in ranges:
        got = fx.gpu.export(first, count)
        same_export(got, fx.want, first, first + count, (first, count))
        dev = device_export(fx.gpu, first, count)
        assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                  b.view(np.uint32) if b.dtype == np.float32 else b) for a, b in zip(dev, got)), (first, count)
        if count:
            st = fx.gpu.fetch_stats()
            assert st["n"] == st["n_found"] == count and st["ms_match"] == 0 and st["ms_table"] == 0


def test_export_ranges(built):
    check_exports(built, export_ranges(built))
    same_export(built.gpu.export(), built.want, 0, built.n, "defaults")
    same_export(built.gpu.export(100), built.want, 100, built.n, "first only")


def test_export_past_the_end_is_invalid_input(built):
    n = built.n
    for first, count in ((0, n + 1), (n, 1), (n + 1, 0), (1, n), (U64_MAX, 2)):
        for entry in (N.lib().vi_indexer_export_records, N.lib().vi_indexer_export_records_device):
            assert entry(built.gpu._h, first, count, None, None, None, None) == N.VI_ERR_INVALID_INPUT, (first, count)
            assert N.lib().vi_last_error()
    with pytest.raises(vip.ViError) as e:
        built.gpu.export(1, n)
    assert e.value.kind == "InvalidInput"


def test_export_with_null_outputs(built):
    first, count = 37, min(500, built.n - 37)
    want = dict(zip("evtw", built.gpu.export(first, count)))
    for mask in range(16):
        outputs = "".join(ch for i, ch in enumerate("evtw") if mask >> i & 1)
        got = dict(zip("evtw", device_export(built.gpu, first, count, outputs)))
        for ch in outputs:
            assert np.array_equal(got[ch].view(np.uint32), want[ch].view(np.uint32)), outputs
    for skew in (4, 8):    # rows that do not start on 16 bytes: the element-wise stores
        got = device_export(built.gpu, first, count, "vw", skew=skew)
        assert np.array_equal(bits(got[1]), bits(want["v"])) and np.array_equal(got[3], want["w"]), skew
    e = np.zeros(count, dtype=np.uint64)
    N.check(N.lib().vi_indexer_export_records(built.gpu._h, first, count, N.ptr(e), None, None, None))
    assert np.array_equal(e, want["e"])


# ---- the hand-made layout ----
def test_hand_made_lists_get_and_export(hand):
    off = np.concatenate([[0], np.cumsum(HAND_LENS)])
    for name in ("all", "odd", "n65", "repeated"):
        same_get(hand.gpu.get(hand.sets[name]), hand.want.get(hand.sets[name]), name)
        same_get(device_get(hand.gpu, hand.sets[name]), hand.want.get(hand.sets[name]), name + " device")
    mid = (int(off[6]) + 70, int(off[8]) + 100 - (int(off[6]) + 70))     # from inside the 200-list into the 129-list
    assert mid[0] % 64 != 0 and mid[0] + mid[1] < hand.n
    check_exports(hand, export_ranges(hand) + [mid, (int(off[3]), 65), (int(off[4]) - 1, 2), (0, 1), (int(off[8]), 129)])
    where = hand.gpu.export()[3]
    assert sorted(set((where >> np.uint64(32)).tolist())) == [0, 1, 2, 3, 6, 8]
    assert int(where[-1]) == (8 << 32) | 128


def test_stored_duplicates(hand):
    off = np.concatenate([[0], np.cumsum(HAND_LENS)])
    ids = u64([DUP3, DUP64, DUP3, 5])
    for got in (hand.gpu.get(ids), device_get(hand.gpu, ids)):
        same_get(got, hand.want.get(ids), "duplicates")
        counts, X, ts, where = got
        assert counts.tolist() == [5, 64, 5, 0]
        assert int(where[0]) == (1 << 32) | 40 and int(where[1]) == 2 << 32 and where[2] == where[0]
        assert np.array_equal(bits(X[0]), bits(hand.want.X[off[1] + 40])) and np.array_equal(bits(X[1]), bits(hand.want.X[off[2]]))
    assert hand.gpu.fetch_stats()["n_found"] == 3


# ---- every case of the walk over the resident slots (csrc/list_layout.hpp), by a get and by an id filter ----
WALK_LENS = [0, 1, 63, 64, 65, 2113, 0, 0, 0]   # 2113 = 32 blocks + 65: a workgroup column of the walk takes a second pass


def test_the_slot_walk_of_a_get_and_of_an_id_filter(tmp_path_factory):
    fx = hand_made(tmp_path_factory.mktemp("walk"), WALK_LENS, 8, duplicates=False)
    assert np.unique(fx.want.ext).size == fx.n
    for name in ("all", "n65", "mostly_absent", "odd"):
        same_get(fx.gpu.get(fx.sets[name]), fx.want.get(fx.sets[name]), name)
    counts, _, _, where = fx.gpu.get(fx.want.ext)
    assert (counts == 1).all() and np.array_equal(where, fx.want.where)     # every resident slot, first to last
    # the filters of a third of the records, and the oracle's whole candidate sequence (k = N, every list probed) less
    # what a filter removes
    rng = np.random.default_rng(5)
    ids = fx.want.ext[rng.random(fx.n) < 1 / 3]
    Q = np.concatenate([fx.want.X[[0, 1, 64, 65, 129, 193, 194, 2305]], rng.standard_normal((8, 8)).astype(np.float32)])
    rc, D, I = O.OracleIndex.load(fx.idx, fx.sh).search_batch(Q, fx.n, 9)
    assert rc == O.ORC_OK and I.shape == (len(Q), fx.n)
    member = np.isin(np.ascontiguousarray(I).view(np.uint64), ids)    # (the id 2^64 - 1 reads as -1 here and on the GPU)
    for exclude in (False, True):
        flt = fx.gpu.filter_ids(ids, exclude=exclude)
        assert flt.num_allowed == (fx.n - ids.size if exclude else ids.size)
        Dg, Ig = fx.gpu.search_sync(Q, 10, 9, filter=flt)
        for q in range(len(Q)):
            keep = np.flatnonzero(member[q] != exclude)[:10]
            assert np.array_equal(Ig[q], I[q][keep]) and np.array_equal(bits(Dg[q]), bits(D[q][keep])), (exclude, q)


# ---- after updates ----
def writable(fx, name):
    root = fx.root / name
    shutil.copytree(fx.idx, str(root / "index"))
    shutil.copytree(fx.sh, str(root / "shards"))
    return str(root / "index"), str(root / "shards")


def check_against_files(gpu, idx, sh, ids):
    """the handle, a fresh load and the re-read files agree on a get of `ids` and on the whole export"""
    want = Order(idx, sh)
    fresh = vip.load(idx, sh, gpu.dimension)
    assert gpu.num_vectors == fresh.num_vectors == want.n
    for ix in (gpu, fresh):
        same_get(ix.get(ids), want.get(ids), "after the update")
        same_export(ix.export(), want, 0, want.n, "after the update")
    return want


def test_after_add_remove_and_upsert(hand):
    idx, sh = writable(hand, "updates")
    gpu = vip.load(idx, sh, hand.dim, now_secs=NOW)
    before = Order(idx, sh)
    rng = np.random.default_rng(5)
    # add: rows near stored ones, new ids, one id that is already stored (a duplicate across the add)
    rows = rng.choice(before.n, 150, replace=False)
    xa = (before.X[rows] + 0.01 * rng.standard_normal((150, hand.dim))).astype(np.float32)
    ea = u64(np.arange(150) + (1 << 45))
    ea[3] = before.ext[10]
    gpu.add(xa, ext_ids=ea, timestamps=u64(np.arange(150) + 9000))
    probe = np.concatenate([ea, before.ext[::5], u64([1 << 46])])
    after_add = check_against_files(gpu, idx, sh, probe)
    assert after_add.n == before.n + 150 and gpu.get(ea[3:4])[0][0] == 2
    # remove: the whole 63-list and the one record of list 0 (both lists end empty), and some added rows
    off = np.concatenate([[0], np.cumsum(after_add.lens)])
    gone = np.concatenate([after_add.ext[off[1]:off[2]], after_add.ext[off[0]:off[1]], ea[20:40]])
    gone = gone[gone != DUP3]
    removed = gpu.remove_ids(gone)
    after_rm = check_against_files(gpu, idx, sh, probe)
    assert removed == after_add.n - after_rm.n > 0
    assert (gpu.get(gone)[0] == 0).all() and (gpu.get(gone)[3] == NONE).all()
    assert after_add.lens[0] > 0 and after_rm.lens[0] == 0     # a list emptied entirely
    # upsert: the new vector and timestamp come back, from the end of the list
    target = after_rm.ext[[50, 300]]
    target = target[(target != DUP3) & (target != DUP64)]
    assert target.size >= 1 and (after_rm.get(target)[0] == 1).all()
    old = after_rm.get(target)
    xu = (old[1] + np.float32(0.001)).astype(np.float32)
    tu = u64(np.arange(target.size) + 777_000)
    assert gpu.upsert(xu, target, timestamps=tu) == target.size
    after_up = check_against_files(gpu, idx, sh, np.concatenate([probe, target]))
    counts, X, ts, where = gpu.get(target)
    assert (counts == 1).all() and np.array_equal(bits(X), bits(xu)) and np.array_equal(ts, tu)
    for w in where:
        l, p = int(w) >> 32, int(w) & 0xFFFFFFFF
        assert p >= after_up.lens[l] - target.size       # at the end of its list


# ---- partitioned handles ----
def check_partitioned(fx, world, placement):
    want = fx.want
    parts = [vip.load(fx.idx, fx.sh, fx.dim, rank=r, world_size=world, placement=placement) for r in range(world)]
    assert sum(p.num_vectors for p in parts) == fx.n
    ids = fx.sets["all"]
    seen_where, total = [], np.zeros(ids.size, dtype=np.uint64)
    best = np.full(ids.size, NONE, dtype=np.uint64)
    best_X, best_ts = np.zeros((ids.size, fx.dim), dtype=np.float32), np.zeros(ids.size, dtype=np.uint64)
    for p in parts:
        e, X, t, w = p.export()
        assert len(e) == p.num_vectors and (w[1:] > w[:-1]).all()      # the rank's records, in ascending where
        # the rank's records are the records of the full order that carry its where values, in that order
        mine = np.isin(want.where, w)
        assert int(mine.sum()) == len(w)
        same_export((e, X, t, w), want.subset(mine), 0, len(w), f"world {world} placement {placement}")
        seen_where.append(w)
        same_get(p.get(ids), want.subset(mine).get(ids), "rank get")
        c, X, t, w = p.get(ids)
        total += c
        better = w < best
        best[better], best_X[better], best_ts[better] = w[better], X[better], t[better]
    assert np.array_equal(np.sort(np.concatenate(seen_where)), np.sort(want.where))
    # per-rank answers combine by the lowest where and the sum of the counts
    same_get((total.astype(np.uint32), best_X, best_ts, best), want.get(ids), "combined")
    uniq = np.unique(ids, return_index=True)[1]
    single = want.get(ids)[0][uniq] == 1
    assert (total[uniq][single] == 1).all()
    return seen_where


@pytest.mark.parametrize("placement", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_handles(built, world, placement):
    check_partitioned(built, world, placement)


@pytest.mark.parametrize("placement", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_partitioned_handles_of_the_hand_made_lists(hand, world, placement):
    seen_where = check_partitioned(hand, world, placement)
    if placement == 0:   # stripes: the 200-list has four blocks, so every rank holds a part of it, with full-list positions
        assert all(((w >> np.uint64(32)) == 6).any() for w in seen_where)
        assert [int(w[(w >> np.uint64(32)) == 6][0]) & 0xFFFFFFFF for w in seen_where] == [64 * r for r in range(world)]


# ---- threads ----
def test_four_threads_get_while_a_fifth_searches(built):
    rng = np.random.default_rng(3)
    reqs = [built.sets["all"], built.sets["mostly_absent"], built.sets["n65"], built.sets["repeated"][:5000]]
    want = [built.gpu.get(r) for r in reqs]
    Q = rng.standard_normal((16, built.dim)).astype(np.float32)
    Dw, Iw = built.gpu.search_sync(Q, 10, 4)
    errors, stop = [], threading.Event()

    def getter(t):
        try:
            for rep in range(6):
                same_get(built.gpu.get(reqs[t]), want[t], f"thread {t}")
                same_export(built.gpu.export(t * 10, 200), built.want, t * 10, t * 10 + 200, f"thread {t}")
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def searcher():
        try:
            while not stop.is_set():
                D, I = built.gpu.search_sync(Q, 10, 4)
                assert np.array_equal(I, Iw) and np.array_equal(bits(D), bits(Dw))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    s = threading.Thread(target=searcher)
    threads = [threading.Thread(target=getter, args=(t,)) for t in range(4)]
    s.start()
    [t.start() for t in threads]
    [t.join() for t in threads]
    stop.set()
    s.join()
    assert not errors, errors


def test_the_first_export_of_a_handle_beside_three_gets(built):
    """a fresh handle: the export that reads the list layout back runs while three threads get, and all four answer as
    they do alone"""
    gpu = vip.load(built.idx, built.sh, built.dim)
    reqs = [built.sets["all"], built.sets["mostly_absent"], built.sets["n65"]]
    want = [built.want.get(r) for r in reqs]
    errors = []

    def run(check):
        try:
            check()
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    checks = [lambda: same_export(gpu.export(), built.want, 0, built.n, "export")]
    checks += [lambda t=t: same_get(gpu.get(reqs[t]), want[t], f"get {t}") for t in range(3)]
    threads = [threading.Thread(target=run, args=(c,)) for c in checks]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    same_export(gpu.export(7, 100), built.want, 7, 107, "a later export")


# ---- adapters ----
def test_python_surface(built):
    from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig
    from vector_indexer_py.harness import FaissStyleAdapter
    want = built.want
    ix = VectorIndexer.load(VectorIndexerConfig.new(built.dim).with_index_dir(built.idx).with_shards_dir(built.sh))
    ids = [int(want.ext[3]), 1 << 50, 0, U64_MAX, int(want.ext[3])]
    recs = ix.get_records(ids)
    assert recs[1] is None and [r is not None for r in recs] == [True, False, True, True, True]
    wc, wX, wt, _ = want.get(ids)
    for i, r in enumerate(recs):
        if r is not None:
            assert r.external_id == ids[i] and r.timestamp == int(wt[i])
            assert np.array_equal(bits(r.values), bits(wX[i]))
    assert ix.get_records([]) == []

    adapter = FaissStyleAdapter(built.gpu)
    rows = [0, 11, want.n - 1]
    got = adapter.reconstruct_batch(want.ext[rows])
    assert np.array_equal(bits(got), bits(want.X[rows]))
    assert np.array_equal(bits(adapter.reconstruct(int(want.ext[11]))), bits(want.X[11]))
    assert np.array_equal(bits(adapter.reconstruct(U64_MAX)), bits(want.get([U64_MAX])[1][0]))
    with pytest.raises(KeyError) as e:
        adapter.reconstruct((1 << 50) + 1)
    assert str((1 << 50) + 1) in str(e.value)
    with pytest.raises(KeyError) as e:
        adapter.reconstruct_batch([int(want.ext[0]), (1 << 50) + 2, (1 << 50) + 3])
    assert str((1 << 50) + 2) in str(e.value)
    built.gpu.get(u64([int(want.ext[0]), 1 << 50, int(want.ext[0])]))
    st = built.gpu.fetch_stats()
    assert st["n"] == 3 and st["n_found"] == 2 and st["bytes_moved"] > 0


def test_timing_fills_the_event_times(built):
    built.gpu.enable_timing(True)
    try:
        built.gpu.get(built.sets["all"])
        st = built.gpu.fetch_stats()
        assert st["ms_total"] > 0 and st["ms_match"] > 0 and st["ms_table"] > 0 and st["ms_gather"] > 0
        assert st["ms_total"] >= st["ms_match"]
        built.gpu.export()
        st = built.gpu.fetch_stats()
        assert st["ms_gather"] > 0 and st["ms_match"] == 0 and st["ms_table"] == 0
    finally:
        built.gpu.enable_timing(False)
    built.gpu.get(built.sets["one"])
    assert built.gpu.fetch_stats()["ms_total"] == 0
