"""GPU parity of the grouping scatter that builds the streaming rank kernel's work items itself (grouping.hip:
item_push_kernel, VI_ITEM_PUSH): every pair writes its column of every work item it sits in, a wave per probed list
writes the items' descriptors and the dead columns.  One small index with the shapes that matter — lists probed by more
than 128 and more than 256 queries of the batch (several query groups, partial last groups), lists of several
segments, an item count that is no multiple of 64 (the partial cycle of the dealing to the XCDs) — checked here from
the oracle's own probes and list lengths.  Every case: the oracle's ids AND distance bits, and rank_mode 3."""
import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip

pytestmark = pytest.mark.gpu

D = 128
NQ = 300
GQ = 128   # queries per work item of the streaming rank kernel


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def _default_engine(monkeypatch):
    for name in ("VI_FILTER", "VI_FILTER_BF16", "VI_FILTER_HI_ONLY", "VI_RANK_STREAM", "VI_RANK_I8", "VI_ITEM_PUSH", "VI_ITEM_RUN",
                 "VI_FILTER_SEGB", "VI_FILTER_GQ", "VI_STREAM_GQ", "VI_COARSE_FILTER", "VI_COARSE_DIRECT", "VI_FORCE_GENERIC",
                 "VI_RANK_APPROX"):
        monkeypatch.delenv(name, raising=False)
    yield


def make_data():
    """1 150 clusters of integer points: one of 700, one of 300, the others of 12 each; 300 queries, 200 of them at the
    first cluster and 60 at the second"""
    rng = np.random.default_rng(1150)
    centres = rng.integers(20, 200, size=(1150, D))
    sizes = np.full(1150, 12)
    sizes[0], sizes[1] = 700, 300
    X = np.concatenate([centres[c] + rng.integers(-6, 7, size=(sizes[c], D)) for c in range(1150)])
    X = X[rng.permutation(X.shape[0])]
    near = np.concatenate([np.zeros(200, dtype=np.int64), np.ones(60, dtype=np.int64), rng.integers(0, 1150, 40)])
    Q = np.clip(centres[near] + rng.integers(-6, 7, size=(NQ, D)), 0, 254)
    return np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(Q, dtype=np.float32)


class Fixture:
    def __init__(self, tmp):
        self.X, self.Q = make_data()
        self.idx, self.sh = str(tmp / "index"), str(tmp / "shards")
        self.orc = O.OracleIndex.build(self.X, self.idx, self.sh, nlist=1150, seed=42)
        self.gpu = self.load()
        self.nlists = self.orc.num_centroids
        self.lens = np.array([self.orc.list_len(c) for c in range(self.nlists)], dtype=np.int64)
        self._probes, self._expected = {}, {}

    def load(self):
        return vip.load(self.idx, self.sh, D)

    def probed_by(self, Q, n_probe):
        """queries of the batch probing each list (the oracle's coarse step)"""
        key = (Q.tobytes(), n_probe)
        if key not in self._probes:
            cnt = np.zeros(self.nlists, dtype=np.int64)
            for q in Q:
                rc, p = self.orc.probe(q, n_probe)
                assert rc == O.ORC_OK
                cnt[p.astype(np.int64)] += 1
            self._probes[key] = cnt
        return self._probes[key]

    def items(self, Q, n_probe, segb):
        """work items of the batch: (query groups) x (segments) over the probed lists (scan.hpp: list_segments)"""
        cnt = self.probed_by(Q, n_probe)
        nblk = (self.lens + 63) // 64
        sb = np.maximum((nblk + 63) // 64, segb)
        nseg = (nblk + sb - 1) // sb
        live = self.lens > 0
        return int((((cnt + GQ - 1) // GQ) * nseg)[live].sum()), nseg

    def expected(self, Q, k, n_probe):
        key = (Q.tobytes(), k, n_probe)
        if key not in self._expected:
            rc, Do, Io = self.orc.search_batch(Q, k, n_probe)
            assert rc == O.ORC_OK
            Do.setflags(write=False)
            Io.setflags(write=False)
            self._expected[key] = (Do, Io)
        return self._expected[key]

    def check(self, gpu, Q, k, n_probe, int8=1, segb=32):
        Do, Io = self.expected(Q, k, n_probe)
        Dg, Ig = gpu.search_sync(Q, k, n_probe)
        bad = np.nonzero((Ig != Io).any(axis=1) | (bits(Dg) != bits(Do)).any(axis=1))[0]
        assert bad.size == 0, f"{bad.size} queries differ, first {bad[0]}: gpu {Ig[bad[0]]} {Dg[bad[0]]} oracle {Io[bad[0]]} {Do[bad[0]]}"
        st = gpu.last_stats()
        assert st["rank_mode"] == 3, st
        assert st["rank_int8"] == int8 and st["group_queries"] == GQ, st
        assert st["scan_items"] == self.items(Q, n_probe, segb)[0], st
        return Dg, Ig


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("item_push"))


def test_fixture_has_the_shapes_that_matter(fx):
    assert fx.nlists >= 1024, "below 1024 lists the coarse step leaves no pair ranks: the scatter would not build the items"
    assert fx.lens.sum() == fx.X.shape[0] == 14776
    assert (fx.lens > 64).sum() >= 6 and fx.lens.max() > 13 * 64   # lists of several blocks, the longest of 14
    c1 = fx.probed_by(fx.Q, 1)
    assert c1.max() == 200                                   # query groups of 128 + 72
    c32 = fx.probed_by(fx.Q, 32)
    assert (c32 > GQ).sum() >= 30
    assert c32[np.argmax(fx.lens)] == NQ                     # 128 + 128 + 44 on the longest list
    rem = c32[c32 > 0] % GQ                                  # partial last groups: dead columns of one wave's stride and of two
    assert ((rem > 0) & (rem < 32)).any() and ((rem > 32) & (rem < 64)).any() and (rem > 64).any(), sorted(set(rem.tolist()))
    for n_probe in (1, 8, 32):
        for segb in (32, 1):
            n, nseg = fx.items(fx.Q, n_probe, segb)
            assert n % 64 != 0, (n_probe, segb, n)           # the last cycle of the dealing to the XCDs is partial
            long_lists = nseg[fx.lens > 640]
            assert long_lists.size >= 2 and (((long_lists >= 11) & (long_lists <= 14)).all() if segb == 1 else (long_lists == 1).all())
    assert fx.items(fx.Q, 32, 1)[0] > fx.items(fx.Q, 32, 32)[0] > 64 * 8   # whole cycles of the dealing and a partial one


@pytest.mark.parametrize("segb", [None, 1])
@pytest.mark.parametrize("k,n_probe", [(10, 32), (1, 1), (64, 8)])
def test_pushed_items_match_the_oracle(fx, k, n_probe, segb, monkeypatch):
    if segb:
        monkeypatch.setenv("VI_FILTER_SEGB", str(segb))    # 11-14 segments in the long lists: every pair writes several items
    fx.check(fx.gpu, fx.Q, k, n_probe, segb=segb or 32)


def test_pushed_items_of_a_bf16_batch(fx):
    """a 255 in the batch: the bf16 streaming kernel, the same work items"""
    Q = fx.Q.copy()
    Q[17, 33] = 255.0
    fx.check(fx.gpu, Q, 10, 32, int8=0)
    fx.check(fx.gpu, fx.Q, 10, 32, int8=1)


def test_item_push_off_returns_the_same_bits(fx, monkeypatch):
    D1, I1 = fx.check(fx.gpu, fx.Q, 10, 32)
    monkeypatch.setenv("VI_ITEM_PUSH", "0")
    D0, I0 = fx.check(fx.gpu, fx.Q, 10, 32)
    monkeypatch.delenv("VI_ITEM_PUSH")
    D2, I2 = fx.check(fx.gpu, fx.Q, 10, 32)
    assert (I0 == I1).all() and (bits(D0) == bits(D1)).all() and (I2 == I1).all() and (bits(D2) == bits(D1)).all()


def test_buffers_grow_and_the_push_is_repeated(fx):
    """a fresh handle: the first batch finds no room, the second needs more than the first left, the third fits"""
    gpu = fx.load()
    fx.check(gpu, fx.Q[:256], 1, 1)
    fx.check(gpu, fx.Q, 10, 32)
    fx.check(gpu, fx.Q, 64, 8)
