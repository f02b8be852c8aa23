"""GPU parity of the coarse step on large centroid tables: 5 121 to 16 388 lists, where the MFMA coarse path with the
direct select (coarse_select_direct_kernel, up to 256 blocks of 64 centroids) runs for batches of >= 256 queries.

A lane of the direct select owns 16 records, i.e. up to 32 sub-blocks of 8 centroids; the list counts below sit on the
boundaries of its per-lane flag words (sub-block 10 from 5 121 lists, sub-block 16 from 8 193 lists) and of the direct
table itself (256 blocks).  The 1 027-list table at D = 256 takes the VALU coarse step, in search and probe export
alike.  Every check is exact:

  probe lists   vi_indexer_probe_device against the oracle's (distance, centroid index) order, and each order row a
                permutation of 0 .. found-1 — the coarse kernel alone, before the list scan can mask a wrong probe;
  search        ids and distance bits of search_sync against the oracle's search_batch;
  control       the same queries in a batch of 100 (below the MFMA coarse threshold);
  knobs         the coarse step's alternative forms on the 8 193- and 16 384-list tables;
  split step    three in-process ranks: probe_device on query slices, search_probed_device, vi_merge_partials_device.

The indexes are built by the product (GPU k-means at these list counts; build parity is pinned by C1) and the oracle
loads the very same files."""
import os

import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from hiprt import Hip
from vector_indexer_py import _native as N

pytestmark = pytest.mark.gpu

NO_POS = 0xFFFFFFFF
P_MAX = 64

# name = list count -> (data seed, D, data, nq, nlist requested).  The build drops the lists k-means leaves empty (2-4 %
# of them at 12 vectors per list): each request was found by building until the table had exactly that many lists (the
# build is deterministic).  D % 16 == 0 stages the exact rows through LDS with the whole wave, D = 20 fetches one row
# per lane; "grid" is small-integer data (tied centroid distances: the (distance, centroid index) rule decides).
TABLES = {
    "5121": (5121, 20, "grid", 513, 5128),        # 81 blocks: first count with sub-block 10; last block holds one list
    "8191": (8192, 128, "gauss", 256, 8545),      # 128 blocks: sub-blocks 0-15 only
    "8193": (8193, 48, "gauss", 1000, 8348),      # 129 blocks: first with sub-blocks 16 and 17; last block holds one list
    "12652": (12652, 96, "gauss", 1000, 13211),   # the reference's default nlist = 4 * ceil(sqrt(N)) at N = 1e7
    "16383": (16384, 20, "gauss", 513, 16777),    # 256 blocks at D = 20
    "16384": (16385, 128, "gauss", 513, 17126),   # the last direct table: 256 full blocks
    "16388": (16385, 128, "gauss", 256, 17110),   # 257 blocks: the non-direct select
    "1027": (1040, 256, "gauss", 256, 1070),      # D = 256: the VALU coarse step (filter_kernel keeps D <= 128)
}

KNOBS = {
    "f32 MFMA coarse": {"VI_FILTER_BF16": "0"},
    "non-direct select": {"VI_COARSE_DIRECT": "0"},
}
# (VI_SELECT_XMODE_COARSE=16 is an ablation with wrong results: it skips the row listing altogether, the ballot loop too)

SEARCHES = [(1, 1), (10, 8), (64, 32), (100, 64)]   # (k, n_probe)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_data(name, rng):
    """12 vectors per list (of the seed's count): N(0, 1), or integers 0..3 for the grid table"""
    seed, d, kind, _, _ = TABLES[name]
    n = 12 * seed
    X = rng.integers(0, 4, size=(n, d)) if kind == "grid" else rng.standard_normal((n, d))
    return X.astype(np.float32)


class Table:
    def __init__(self, name, work):
        seed, d, kind, nq, request = TABLES[name]
        nlist = int(name)
        rng = np.random.default_rng(seed)
        self.X = make_data(name, rng)
        n = self.X.shape[0]
        self.gpu = vip.build(self.X, work, nlist=request, now_secs=1_700_000_000)
        self.work = work
        self.orc = O.OracleIndex.load(os.path.join(work, "index"), os.path.join(work, "shards"))
        assert self.gpu.num_centroids == nlist == self.orc.num_centroids
        # half stored vectors, half perturbed ones, the last few far from the data
        half = nq // 2
        far = 8
        Q = np.concatenate([self.X[rng.integers(0, n, size=half)],
                            self.X[rng.integers(0, n, size=nq - half)] * (1 + 0.05 * rng.standard_normal((nq - half, d)))])
        Q[-far:] = 40.0 + 10.0 * rng.standard_normal((far, d))
        self.Q = np.ascontiguousarray(Q, dtype=np.float32)
        self.name = name
        self._probes, self._results = {}, {}

    def oracle_probes(self, Q):
        """the oracle's probe rows for 64 probes; it sorts every centroid, so the first P equal orc.probe(q, P)"""
        key = Q.shape[0]
        if key not in self._probes:
            rows = []
            for q in Q:
                rc, p = self.orc.probe(q, P_MAX)
                assert rc == O.ORC_OK and p.size == P_MAX
                rows.append(p)
            self._probes[key] = np.array(rows, dtype=np.int64)
        return self._probes[key]

    def oracle_search(self, Q, k, n_probe):
        key = (Q.shape[0], k, n_probe)
        if key not in self._results:
            rc, Do, Io = self.orc.search_batch(Q, k, n_probe, O.usable_cpus())
            assert rc == O.ORC_OK
            self._results[key] = (Do, Io)
        return self._results[key]


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """every table built once, on first use, for the whole module (tests of several tables interleave)"""
    built = {}

    def get(name):
        if name not in built:
            built[name] = Table(name, str(tmp_path_factory.mktemp("coarse" + name)))
        return built[name]
    yield get
    import shutil
    for t in built.values():
        shutil.rmtree(t.work, ignore_errors=True)


@pytest.fixture
def table(request, tables):
    return tables(request.param)


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.close()


def check_probes(t, hip, Q, n_probe, what):
    nq = Q.shape[0]
    xq = hip.upload(Q)
    probes, order = hip.alloc(nq * n_probe * 4), hip.alloc(nq * n_probe * 4)
    assert t.gpu.probe_device(xq, nq, n_probe, probes, order) == n_probe
    got = hip.download(probes, (nq, n_probe), np.uint32).astype(np.int64)
    go = hip.download(order, (nq, n_probe), np.uint32).astype(np.int64)
    want = t.oracle_probes(Q)[:, :n_probe]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (f"{t.name} lists, {what}, n_probe {n_probe}: {bad.size} of {nq} probe rows differ, first "
                           f"{bad[0]}: gpu {got[bad[0]].tolist()} oracle {want[bad[0]].tolist()}")
    check_orders(got, go, f"{t.name} lists, {what}, n_probe {n_probe}")


def check_orders(probes, order, what):
    """the real probes come first and their orders are a permutation of 0 .. found-1"""
    for r in range(probes.shape[0]):
        found = int((probes[r] != NO_POS).sum())
        assert (probes[r, :found] != NO_POS).all(), (what, r)
        assert sorted(order[r, :found].tolist()) == list(range(found)), (what, r, order[r].tolist())


def check_search(t, Q, k, n_probe, what):
    Do, Io = t.oracle_search(Q, k, n_probe)
    Dg, Ig = t.gpu.search_sync(Q, k, n_probe)
    bad = np.nonzero((Ig != Io).any(axis=1) | (bits(Dg) != bits(Do)).any(axis=1))[0]
    assert bad.size == 0, (f"{t.name} lists, {what}, k {k}, n_probe {n_probe}: {bad.size} of {Q.shape[0]} queries "
                           f"differ, first {bad[0]}: gpu {Ig[bad[0]]} {Dg[bad[0]]} oracle {Io[bad[0]]} {Do[bad[0]]}")


@pytest.mark.parametrize("table", list(TABLES), indirect=True)
def test_probe_lists_match_the_oracle(table, hip):
    for n_probe in (1, 8, 32, 64):
        check_probes(table, hip, table.Q, n_probe, f"{table.Q.shape[0]} queries")


@pytest.mark.parametrize("table", list(TABLES), indirect=True)
def test_search_matches_the_oracle(table):
    for k, n_probe in SEARCHES:
        check_search(table, table.Q, k, n_probe, f"{table.Q.shape[0]} queries")


@pytest.mark.parametrize("table", list(TABLES), indirect=True)
def test_small_batch_takes_the_other_coarse_step_to_the_same_result(table, hip):
    Q = np.ascontiguousarray(table.Q[-100:])   # (the far queries included)
    for n_probe in (8, 64):
        check_probes(table, hip, Q, n_probe, "100 queries")
    for k, n_probe in [(10, 8), (100, 64)]:
        check_search(table, Q, k, n_probe, "100 queries")


@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("table", ["8193", "16384"], indirect=True)
def test_coarse_knobs_match_the_oracle(table, knob, hip, monkeypatch):
    for key, value in KNOBS[knob].items():
        monkeypatch.setenv(key, value)
    for n_probe in (8, 64):
        check_probes(table, hip, table.Q, n_probe, knob)
    for k, n_probe in [(10, 8), (100, 64)]:
        check_search(table, table.Q, k, n_probe, knob)


@pytest.mark.parametrize("table", ["12652"], indirect=True)
def test_split_coarse_step_over_three_ranks(table, hip):
    """the coarse step split by query over three ranks (each slice >= 256 queries: the MFMA coarse path), the list
    scan on every rank's stripes with the gathered probe lists, the partial results merged: the oracle's search"""
    world, Q = 3, table.Q
    nq, d = Q.shape
    parts = [vip.load(os.path.join(table.work, "index"), os.path.join(table.work, "shards"), d, rank=r, world_size=world)
             for r in range(world)]
    xq = hip.upload(Q)
    per = (nq + world - 1) // world
    assert nq - (world - 1) * per >= 256
    for k, n_probe in [(10, 32), (100, 64)]:
        probes, order = hip.alloc(nq * n_probe * 4), hip.alloc(nq * n_probe * 4)
        for r, p in enumerate(parts):
            q0, q1 = r * per, min(nq, (r + 1) * per)
            assert p.probe_device(xq + q0 * d * 4, q1 - q0, n_probe, probes + q0 * n_probe * 4,
                                  order + q0 * n_probe * 4) == n_probe
        got = hip.download(probes, (nq, n_probe), np.uint32).astype(np.int64)
        want = table.oracle_probes(Q)[:, :n_probe]
        assert (got == want).all(), f"split coarse step: {(got != want).any(axis=1).sum()} probe rows differ"
        check_orders(got, hip.download(order, (nq, n_probe), np.uint32).astype(np.int64), "split coarse step")
        Dg, Ig, Tg = hip.alloc(world * nq * k * 4), hip.alloc(world * nq * k * 8), hip.alloc(world * nq * k * 8)
        for r, p in enumerate(parts):
            p.search_probed_device(xq, nq, k, n_probe, probes, order, Dg + r * nq * k * 4, Ig + r * nq * k * 8,
                                   Tg + r * nq * k * 8)
        Dm, Im = hip.alloc(nq * k * 4), hip.alloc(nq * k * 8)
        N.check(N.lib().vi_merge_partials_device(0, nq, k, world, Dg, Ig, Tg, Dm, Im))
        Do, Io = table.oracle_search(Q, k, n_probe)
        Dh, Ih = hip.download(Dm, (nq, k), np.float32), hip.download(Im, (nq, k), np.int64)
        bad = np.nonzero((Ih != Io).any(axis=1) | (bits(Dh) != bits(Do)).any(axis=1))[0]
        assert bad.size == 0, f"split coarse step, k {k}, n_probe {n_probe}: {bad.size} of {nq} queries differ"
