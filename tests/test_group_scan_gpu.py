"""GPU parity of the grouping in two launches (grouping.hip: list_totals_kernel with GroupScanArgs, then
item_push_kernel — GroupingRoute::ScansPush): a workgroup of list_totals_kernel leaves every list's counts relative to its 64 lists and the sums of
the 64, a few more workgroups scan the queries' record totals (a run of whole tiles each), and every workgroup of
item_push_kernel scans the sums.  One small index of 1 150 clusters — 18 workgroups of lists, the last a partial one —
and batches whose probes, taken from the oracle's own coarse step, leave one whole workgroup of 64 (non-empty) lists in
the middle unprobed: a zero among the sums.  Batches of 256 (the smallest the path takes), 300 and 1 501 queries (the
query scan's tile is 1 024 words, four to a lane: a second workgroup on a partial tile that ends inside a lane's four),
and one of 70 001 repeated queries (more tiles than one round of a query workgroup holds).  Every case: the oracle's ids
AND distance bits, rank_mode 3, and the statistics that change hands — work items, scanned vectors, tile blocks —
against counts derived from the oracle's probes and list lengths.
(The group-record count itself is no field of last_stats(): it sizes the record buffers of the searches checked here.)
VI_SCAN_IN_TOTALS=0 (group_prepare_kernel, three launches) and VI_ITEM_PUSH=0 must return the same bits."""
import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip

pytestmark = pytest.mark.gpu

D = 128
NLIST = 1150
P = 8      # probes per query: few enough that a pool of queries avoiding 64 given lists is large
GQ = 128   # queries per work item of the streaming rank kernel
SIZES = (256, 300, 1501)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def _default_engine(monkeypatch):
    for name in ("VI_FILTER", "VI_FILTER_BF16", "VI_FILTER_HI_ONLY", "VI_RANK_STREAM", "VI_RANK_I8", "VI_ITEM_PUSH", "VI_ITEM_RUN",
                 "VI_SCAN_IN_TOTALS", "VI_FILTER_SEGB", "VI_FILTER_GQ", "VI_STREAM_GQ", "VI_COARSE_FILTER", "VI_COARSE_DIRECT",
                 "VI_FORCE_GENERIC", "VI_RANK_APPROX"):
        monkeypatch.delenv(name, raising=False)
    yield


def make_data():
    """1 150 clusters of integer points (one of 700, one of 300, the others of 12 each) and a pool of candidate queries:
    600 at the first cluster, 150 at the second, two at every other one"""
    rng = np.random.default_rng(1150)
    centres = rng.integers(20, 200, size=(NLIST, D))
    sizes = np.full(NLIST, 12)
    sizes[0], sizes[1] = 700, 300
    X = np.concatenate([centres[c] + rng.integers(-6, 7, size=(sizes[c], D)) for c in range(NLIST)])
    X = X[rng.permutation(X.shape[0])]
    near = np.concatenate([np.zeros(600, dtype=np.int64), np.ones(150, dtype=np.int64), np.repeat(np.arange(2, NLIST), 2)])
    pool = np.clip(centres[near] + rng.integers(-6, 7, size=(near.size, D)), 0, 254)
    return np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(pool, dtype=np.float32), near


class Fixture:
    def __init__(self, tmp):
        self.X, pool, near = make_data()
        self.idx, self.sh = str(tmp / "index"), str(tmp / "shards")
        self.orc = O.OracleIndex.build(self.X, self.idx, self.sh, nlist=NLIST, seed=42)
        self.nlists = self.orc.num_centroids
        self.lens = np.array([self.orc.list_len(c) for c in range(self.nlists)], dtype=np.int64)
        # the oracle's probes of every candidate; the unprobed workgroup: a middle one that holds none of the first probes
        # of the two big clusters' queries and costs the fewest candidates
        probes = np.stack([self.probe(q) for q in pool])
        wg = probes // 64
        nwg = (self.nlists + 63) // 64
        big = set(wg[near < 2].ravel().tolist())
        lost = [np.inf if (w in big or w == 0 or w == nwg - 1) else int((wg == w).any(axis=1).sum()) for w in range(nwg)]
        self.hole = int(np.argmin(lost))
        keep = ~(wg == self.hole).any(axis=1)
        a, b, c = (pool[keep & (near == 0)], pool[keep & (near == 1)], pool[keep & (near >= 2)])
        # queries may repeat: the batches are cut from one sequence
        self.batches = {
            256: np.concatenate([a[:200], b[:56]]),
            300: np.concatenate([a[:200], b[:60], c[:40]]),
            1501: np.concatenate([a[:400], b[:100], np.resize(c, (1001, D))]),
        }
        for q in self.batches.values():
            q.setflags(write=False)
        self.gpu = self.load()
        self._probes, self._expected = {}, {}

    def load(self):
        return vip.load(self.idx, self.sh, D)

    def probe(self, q):
        rc, p = self.orc.probe(q, P)
        assert rc == O.ORC_OK
        return p.astype(np.int64)

    def probed_by(self, Q):
        """queries of the batch probing each list (the oracle's coarse step)"""
        key = Q.tobytes()
        if key not in self._probes:
            cnt = np.zeros(self.nlists, dtype=np.int64)
            for q in Q:
                cnt[self.probe(q)] += 1
            self._probes[key] = cnt
        return self._probes[key]

    def counts(self, Q, segb):
        """work items, scanned vectors, tile blocks of the batch (scan.hpp: list_segments; grouping.hip: list_group_counts)"""
        cnt = np.where(self.lens > 0, self.probed_by(Q), 0)
        nblk = (self.lens + 63) // 64
        sb = np.maximum((nblk + 63) // 64, segb)
        nseg = (nblk + sb - 1) // sb
        chunks = (cnt + GQ - 1) // GQ
        return dict(scan_items=int((chunks * nseg).sum()), scanned_vectors=int((cnt * self.lens).sum()),
                    filter_tile_blocks=int((chunks * nblk).sum())), nseg

    def expected(self, Q, k):
        key = (Q.tobytes(), k)
        if key not in self._expected:
            rc, Do, Io = self.orc.search_batch(Q, k, P)
            assert rc == O.ORC_OK
            Do.setflags(write=False)
            Io.setflags(write=False)
            self._expected[key] = (Do, Io)
        return self._expected[key]

    def check(self, gpu, Q, k, int8=1, segb=32):
        Do, Io = self.expected(Q, k)
        Dg, Ig = gpu.search_sync(Q, k, P)
        bad = np.nonzero((Ig != Io).any(axis=1) | (bits(Dg) != bits(Do)).any(axis=1))[0]
        assert bad.size == 0, f"{bad.size} queries differ, first {bad[0]}: gpu {Ig[bad[0]]} {Dg[bad[0]]} oracle {Io[bad[0]]} {Do[bad[0]]}"
        st = gpu.last_stats()
        assert st["rank_mode"] == 3, st
        assert st["rank_int8"] == int8 and st["group_queries"] == GQ, st
        want, _ = self.counts(Q, segb)
        assert {name: st[name] for name in want} == want, st
        return Dg, Ig


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return Fixture(tmp_path_factory.mktemp("group_scan"))


def test_fixture_has_the_shapes_that_matter(fx):
    assert fx.nlists >= 1024 and fx.nlists % 64 != 0 and fx.nlists <= 256 * 64   # a partial last workgroup of lists
    nwg = (fx.nlists + 63) // 64
    assert fx.lens.sum() == fx.X.shape[0] == 14776
    assert 0 < fx.hole < nwg - 1
    assert (fx.lens[64 * fx.hole:64 * fx.hole + 64] > 0).all()          # the unprobed lists are no empty ones
    assert (fx.lens > 64).sum() >= 2 and fx.lens.max() > 8 * 64          # lists of several blocks
    for nq in SIZES:
        Q = fx.batches[nq]
        assert Q.shape == (nq, D) and Q.min() >= 0 and Q.max() <= 254
        cnt = fx.probed_by(Q)
        per_wg = np.add.reduceat(cnt, np.arange(0, fx.nlists, 64))
        assert per_wg[fx.hole] == 0 and (per_wg[:fx.hole] > 0).any() and (per_wg[fx.hole + 1:] > 0).any()
        assert (per_wg > 0).sum() >= 3
        assert per_wg[-1] > 0 or nq == 256                               # ... the partial workgroup among them
        rem = cnt[cnt > 0] % GQ
        assert (rem > 0).any()                                           # partial last query groups
        for segb in (32, 1):
            n, nseg = fx.counts(Q, segb)
            long_lists = nseg[fx.lens > 640]
            assert long_lists.size >= 1 and ((long_lists >= 10).all() if segb == 1 else (long_lists == 1).all())
    assert fx.probed_by(fx.batches[1501]).max() > 256                    # three query groups and more on one list
    assert fx.probed_by(fx.batches[300]).max() > GQ
    assert 1501 > 1024 and 1501 % 1024 != 0 and 1501 % 4 != 0            # the query scan: a whole tile and a partial one


@pytest.mark.parametrize("segb", [None, 1])
@pytest.mark.parametrize("nq", SIZES)
def test_two_launch_grouping_matches_the_oracle(fx, nq, segb, monkeypatch):
    if segb:
        monkeypatch.setenv("VI_FILTER_SEGB", str(segb))    # ten and more segments in the long lists
    fx.check(fx.gpu, fx.batches[nq], 10, segb=segb or 32)


@pytest.mark.parametrize("nq", SIZES)
def test_three_chains_return_the_same_bits(fx, nq, monkeypatch):
    Q = fx.batches[nq]
    D1, I1 = fx.check(fx.gpu, Q, 10)
    monkeypatch.setenv("VI_SCAN_IN_TOTALS", "0")           # list_totals, group_prepare, item_push
    D0, I0 = fx.check(fx.gpu, Q, 10)
    monkeypatch.delenv("VI_SCAN_IN_TOTALS")
    monkeypatch.setenv("VI_ITEM_PUSH", "0")                # ... and the work items by kernels of their own
    D2, I2 = fx.check(fx.gpu, Q, 10)
    monkeypatch.delenv("VI_ITEM_PUSH")
    D3, I3 = fx.check(fx.gpu, Q, 10)                       # (and back, on buffers the other chains have written)
    for Dx, Ix in ((D0, I0), (D2, I2), (D3, I3)):
        assert (Ix == I1).all() and (bits(Dx) == bits(D1)).all()


def test_bf16_batch_through_the_same_grouping(fx):
    """a 255 in the batch: the bf16 streaming kernel, the same work items"""
    Q = fx.batches[300].copy()
    Q[17, 33] = 255.0
    fx.check(fx.gpu, Q, 10, int8=0)
    fx.check(fx.gpu, fx.batches[300], 10, int8=1)


def test_buffers_grow_and_the_offsets_change_length(fx):
    """a fresh handle: the first batch finds no room, the second needs more than the first left, the third has another
    number of queries (qoff of another length, other sums)"""
    gpu = fx.load()
    fx.check(gpu, fx.batches[256], 1)
    fx.check(gpu, fx.batches[1501], 10)
    fx.check(gpu, fx.batches[300], 10)
    fx.check(gpu, fx.batches[1501][:1027], 10)   # (the last lane of the query scan holds three words, then two)
    fx.check(gpu, fx.batches[1501][:258], 10)
    fx.check(gpu, fx.batches[1501], 64)


def test_more_query_tiles_than_one_round(fx):
    """70 001 queries, the batch of 300 repeated: 69 tiles of record totals over 14 query workgroups, two rounds each; the
    oracle's answer is that of the 300, repeated, and every list is probed 233 times as often and by 101 queries more"""
    nq, Q300 = 70001, fx.batches[300]
    Q = np.resize(Q300, (nq, D))
    Do, Io = fx.expected(Q300, 10)
    fx._expected[(Q.tobytes(), 10)] = (np.resize(Do, (nq, 10)), np.resize(Io, (nq, 10)))
    fx._probes[Q.tobytes()] = (nq // 300) * fx.probed_by(Q300) + fx.probed_by(Q300[:nq % 300])
    fx.check(fx.gpu, Q, 10)
