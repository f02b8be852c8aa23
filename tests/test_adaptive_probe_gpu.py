"""GPU: adaptive probing (vi_indexer_search_adaptive*, vi_indexer_prune_probes_device) on all three engines.

The contract: the pruned search of query q is, bit for bit, the reference's search of q with n_probe = p_q, and p_q follows
from the rule (include/vi_amd.h) and the query's coarse row.  Everything expected comes from the oracle alone: probe(q, P)
gives the row, l2sq_scalar against centroids() the coarse distances d_r, list_len the budget, numpy f32 the threshold
t = fl32(ratio2 * d_0), and search(q, k, p_q) the answer; n_probed is compared with p_q exactly.  The ratio and the budget
are chosen from the data (medians over the queries) so that the rule bites on about half of them, and one query is a
stored centroid (d_0 == 0)."""
import numpy as np
import pytest

import oracle_lib as O
import vector_indexer_py as vip
from vector_indexer_py import _native as N

from test_filtered_search_gpu import Fixture, TENTH, base, bits, bytes8, long_lists, queries, valu, wide  # noqa: F401

pytestmark = pytest.mark.gpu
U64_MAX = (1 << 64) - 1
MARK = 0xFFFFFFFF


class Case:
    """a fixture under the first nq of its queries, one of them replaced by a stored centroid; the oracle's coarse rows per
    n_probe are computed once and shared"""

    def __init__(self, fx, nq=None, centroid_query=True):
        self.fx = Fixture.__new__(Fixture)
        self.fx.__dict__.update(fx.__dict__)
        self.cent, _ = fx.orc.centroids()
        Q = fx.Q[:nq].copy()
        self.zero_q = min(7, Q.shape[0] - 1)
        if centroid_query:
            Q[self.zero_q] = self.cent[min(3, self.cent.shape[0] - 1)]
        self.fx.Q, self.fx._full = Q, {}
        self.Q, self.nq, self.gpu, self.orc, self.nlists = Q, Q.shape[0], fx.gpu, fx.orc, fx.nlists
        self.lens = np.array([fx.orc.list_len(c) for c in range(self.nlists)], dtype=np.uint64)
        self._rows = {}

    def rows(self, n_probe):
        """(P, probes i64[nq, P] (-1: none), d f32[nq, P] (inf: none), found[nq]) from the oracle"""
        P = min(n_probe, self.nlists)
        if P not in self._rows:
            probes, d = np.full((self.nq, P), -1, dtype=np.int64), np.full((self.nq, P), np.inf, dtype=np.float32)
            for q in range(self.nq):
                rc, row = self.orc.probe(self.Q[q], P)
                assert rc == O.ORC_OK
                probes[q, :row.size] = row
                d[q, :row.size] = [O.l2sq_scalar(self.Q[q], self.cent[int(l)]) for l in row]
            found = (probes >= 0).sum(axis=1)
            for a in (probes, d, found):
                a.setflags(write=False)
            self._rows[P] = (P, probes, d, found)
        return self._rows[P]

    def lens_of(self, n_probe):
        P, probes, _, _ = self.rows(n_probe)
        return np.where(probes >= 0, self.lens[np.maximum(probes, 0)], np.uint64(0))

    def ratio_from_data(self, n_probe):
        """the f32 median over the queries of d_{P/2} / d_0"""
        P, _, d, found = self.rows(n_probe)
        ok = d[:, 0] > 0
        r = (d[ok, min(P // 2, int(found.min()) - 1)] / d[ok, 0]).astype(np.float32)
        return float(np.float32(np.median(r)))

    def budget_from_data(self, n_probe):
        P = self.rows(n_probe)[0]
        return int(np.median(np.cumsum(self.lens_of(n_probe), axis=1)[:, P // 2]))

    def p_q(self, n_probe, rule):
        """the rule, from the oracle's rows alone"""
        P, probes, d, found = self.rows(n_probe)
        real = probes >= 0
        p = found.copy()
        if rule.ratio2 != 0.0:
            t = np.float32(rule.ratio2) * d[:, 0]          # one f32 multiply
            assert t.dtype == np.float32
            p = np.minimum(p, ((d <= t[:, None]) & real).sum(axis=1))
        if rule.max_codes != 0:
            met = (np.cumsum(self.lens_of(n_probe), axis=1) >= np.uint64(rule.max_codes)) & real
            p = np.minimum(p, np.where(met.any(axis=1), met.argmax(axis=1) + 1, found))
        if rule.n_probe_q is not None:
            p = np.minimum(p, np.asarray(rule.n_probe_q, dtype=np.int64))
        lo = np.minimum(max(rule.min_probe, 1), found)
        return np.minimum(np.maximum(p, lo), found).astype(np.int64)

    def expected(self, k, p, window=None):
        """(D, I) per query from orc.search at that query's own p; with a window: the oracle's whole sorted candidate
        sequence at that p with the records outside the window deleted, first k (as test_filtered_search_gpu)"""
        De, Ie = np.full((self.nq, k), np.inf, dtype=np.float32), np.full((self.nq, k), -1, dtype=np.int64)
        for v in np.unique(p):
            idx = np.nonzero(p == v)[0]
            if window is None:
                rc, D, I = self.orc.search_batch(self.Q[idx], k, int(v))
                assert rc == O.ORC_OK
                De[idx], Ie[idx] = D, I
                continue
            rc, D, I = self.orc.search_batch(self.Q[idx], self.fx.n, int(v))
            assert rc == O.ORC_OK
            s = self.fx.stored[np.where(I >= 0, (I - 1_000_003) // 7, 0)]
            keep = (I >= 0) & (s >= np.uint64(window[0])) & (s <= np.uint64(window[1]))
            rank = np.cumsum(keep, axis=1) - 1
            r, c = np.nonzero(keep & (rank < k))
            De[idx[r], rank[r, c]], Ie[idx[r], rank[r, c]] = D[r, c], I[r, c]
        return De, Ie

    def rules(self, n_probe, seed=0):
        """each rule alone and all three together, for this n_probe"""
        P = self.rows(n_probe)[0]
        ratio2, budget = self.ratio_from_data(n_probe), self.budget_from_data(n_probe)
        explicit = np.random.default_rng(seed).integers(0, P + 4, self.nq).astype(np.uint32)
        return {"ratio": vip.ProbeRule(ratio2=ratio2), "codes": vip.ProbeRule(max_codes=budget),
                "explicit": vip.ProbeRule(n_probe_q=explicit), "min_probe": vip.ProbeRule(min_probe=3, ratio2=1.0),
                "all": vip.ProbeRule(min_probe=2, ratio2=ratio2, max_codes=budget, n_probe_q=explicit)}

    def check(self, k, n_probe, rule, window=None, what=""):
        p = self.p_q(n_probe, rule)
        De, Ie = self.expected(k, p, window)
        flt = self.fx.filter(window) if window is not None else None
        Dg, Ig, probed = self.gpu.search_adaptive_sync(self.Q, k, n_probe, rule, filter=flt, return_probed=True)
        assert np.array_equal(probed.astype(np.int64), p), (what, k, n_probe, np.nonzero(probed != p)[0][:8], probed[:12], p[:12])
        bad = np.nonzero((Ig != Ie).any(axis=1) | (bits(Dg) != bits(De)).any(axis=1))[0]
        assert bad.size == 0, (f"{what} k {k} n_probe {n_probe}: {bad.size} queries differ, first {bad[0]} (p {p[bad[0]]}): "
                               f"gpu {Ig[bad[0]][:8]} {Dg[bad[0]][:8]} expected {Ie[bad[0]][:8]} {De[bad[0]][:8]}")
        return p

    def sweep(self, n_probe, ks=(10,), names=None):
        for name, rule in self.rules(n_probe).items():
            if names is None or name in names:
                for k in ks:
                    self.check(k, n_probe, rule, what=name)


@pytest.fixture(scope="module")
def case(base):  # noqa: F811
    return Case(base)


@pytest.fixture(scope="module")
def hip():
    from hiprt import Hip
    h = Hip()
    yield h
    h.close()


def device_adaptive(hip, index, xq, nq, k, n_probe, rule, flt=None):
    """the device entry -> (D, I, tie, n_probed) on the host; rule.n_probe_q (host array) is uploaded for the call"""
    D, I, T, Pq = hip.alloc(nq * k * 4), hip.alloc(nq * k * 8), hip.alloc(nq * k * 8), hip.alloc(nq * 4)
    dev = vip.ProbeRule(rule.min_probe, rule.ratio2, rule.max_codes,
                        None if rule.n_probe_q is None else hip.upload(np.asarray(rule.n_probe_q, dtype=np.uint32)))
    index.search_adaptive_device(xq, nq, k, n_probe, dev, D, I, T, Pq, filter=flt)
    return (hip.download(D, (nq, k), np.float32), hip.download(I, (nq, k), np.int64), hip.download(T, (nq, k), np.uint64),
            hip.download(Pq, (nq,), np.uint32))


def device_search(hip, index, xq, nq, k, n_probe, flt=None):
    D, I, T = hip.alloc(nq * k * 4), hip.alloc(nq * k * 8), hip.alloc(nq * k * 8)
    index.search_device(xq, nq, k, n_probe, D, I, T, filter=flt)
    return hip.download(D, (nq, k), np.float32), hip.download(I, (nq, k), np.int64), hip.download(T, (nq, k), np.uint64)


# ---- the rule bites, as the oracle alone sees it ----
@pytest.mark.parametrize("n_probe", [8, 24])
def test_the_rules_from_the_data_spread_the_probe_counts(case, n_probe):
    P, _, d, found = case.rows(n_probe)
    rule = case.rules(n_probe)["ratio"]
    assert rule.ratio2 >= 1.0
    p = case.p_q(n_probe, rule)
    assert np.unique(p).size >= 4, np.unique(p)
    assert (p == P).sum() < case.nq / 2 and (p == 1).sum() < case.nq / 2, np.bincount(p)
    assert d[case.zero_q, 0] == 0.0 and p[case.zero_q] == 1       # the stored centroid: t == 0 keeps the one at distance 0
    pc = case.p_q(n_probe, case.rules(n_probe)["codes"])
    assert np.unique(pc).size >= 2 and (pc == P).sum() < case.nq / 2, np.bincount(pc)


# ---- base: each rule alone and all three together ----
@pytest.mark.parametrize("n_probe", [8, 24])
@pytest.mark.parametrize("k", [1, 10, 100])
def test_each_rule_and_all_three(case, k, n_probe):
    case.sweep(n_probe, ks=(k,))
    assert case.gpu.last_stats()["rank_mode"] >= 1


def test_a_timestamp_filter_composed_with_a_rule(base):  # noqa: F811
    c = Case(base, 64)
    for name in ("ratio", "all"):
        for k, n_probe in [(10, 8), (100, 24)]:
            c.check(k, n_probe, c.rules(n_probe)[name], window=TENTH, what="filtered " + name)


# ---- the engines ----
def test_valu_engine(valu):  # noqa: F811
    Case(valu, 64).sweep(8)
    assert valu.gpu.last_stats()["rank_mode"] == 0


def test_wide_vectors(wide):  # noqa: F811
    Case(wide, 64).sweep(8)
    assert wide.gpu.last_stats()["rank_mode"] == 2


def test_byte_lists(bytes8):  # noqa: F811
    Case(bytes8, 64, centroid_query=False).sweep(8)      # (a batch of integer queries: the int8 rank kernel)
    st = bytes8.gpu.last_stats()
    assert st["rank_mode"] == 3 and st["rank_int8"] == 1, st
    Case(bytes8, 64).sweep(8, names=("ratio", "all"))     # ... and with the centroid, which is no integer vector: bf16
    assert bytes8.gpu.last_stats()["rank_int8"] == 0


def test_lists_longer_than_a_segment(long_lists):  # noqa: F811
    c = Case(long_lists, 64)
    c.sweep(2, names=("ratio", "explicit", "all"))
    p = c.p_q(2, c.rules(2)["ratio"])
    assert 0 < (p == 1).sum() < c.nq


def test_generic_engine_forced(case, monkeypatch):
    monkeypatch.setenv("VI_FORCE_GENERIC", "1")
    case.sweep(8)
    assert case.gpu.last_stats()["rank_mode"] == 0


def test_rows_longer_than_a_wave(tmp_path_factory):
    """n_probe = 80 > 64 on an index of 96 lists: the sort-everything engine, and prune rows of two chunks"""
    rng = np.random.default_rng(6)
    X = rng.standard_normal((6000, 32)).astype(np.float32)
    c = Case(Fixture(tmp_path_factory.mktemp("many"), X, 96, queries(rng, X, 64)))
    assert c.nlists >= 80
    c.sweep(80)
    p = c.p_q(80, c.rules(80)["explicit"])
    assert (p > 64).any() and (p < 64).any() and np.unique(c.p_q(80, c.rules(80)["ratio"])).size >= 4   # both chunks end rows


def test_coarse_step_on_the_matrix_cores(tmp_path_factory, hip):
    """nq >= 256 against >= 1024 lists: the shape coarse_on_matrix_cores takes"""
    rng = np.random.default_rng(7)
    X = rng.standard_normal((20000, 32)).astype(np.float32)
    c = Case(Fixture(tmp_path_factory.mktemp("mfma"), X, 1100, queries(rng, X, 300)))
    assert c.nlists >= 1024 and c.nq >= 256
    c.sweep(32, names=("ratio", "codes", "all"))
    assert c.gpu.last_stats()["rank_mode"] >= 1
    xq = hip.upload(c.Q)
    rule = c.rules(32)["all"]
    p = c.p_q(32, rule)
    De, Ie = c.expected(10, p)
    Dd, Id, Td, Pd = device_adaptive(hip, c.gpu, xq, c.nq, 10, 32, rule)
    assert np.array_equal(Pd, p) and np.array_equal(Id, Ie) and np.array_equal(bits(Dd), bits(De))


@pytest.mark.parametrize("nq", [1, 33])
def test_small_batches(base, nq):  # noqa: F811
    Case(base, nq, centroid_query=nq > 1).sweep(8, ks=(10,))     # (the ratio comes from queries with d_0 > 0)


# ---- a rule of zeros is the plain search; host and device entries agree; tie keys ----
def test_zero_rule_equals_the_plain_search_bit_for_bit(case, hip):
    xq = hip.upload(case.Q)
    zero = vip.ProbeRule(min_probe=0)
    for k, n_probe in [(10, 8), (100, 24), (200, 8), (10, 10_000)]:
        Du, Iu, Tu = device_search(hip, case.gpu, xq, case.nq, k, n_probe)
        Da, Ia, Ta, Pa = device_adaptive(hip, case.gpu, xq, case.nq, k, n_probe, zero)
        assert np.array_equal(bits(Du), bits(Da)) and np.array_equal(Iu, Ia) and np.array_equal(Tu, Ta), (k, n_probe)
        assert (Pa == min(n_probe, case.nlists)).all()
        Dh, Ih, Vh = case.gpu.search_sync(case.Q, k, n_probe, include_vectors=True)
        Dg, Ig, Vg = case.gpu.search_adaptive_sync(case.Q, k, n_probe, vip.ProbeRule(), include_vectors=True)
        assert np.array_equal(bits(Dh), bits(Dg)) and np.array_equal(Ih, Ig) and np.array_equal(Vh, Vg), (k, n_probe)
    flt = case.fx.filter(TENTH)
    Du, Iu, Tu = device_search(hip, case.gpu, xq, case.nq, 10, 8, flt)
    Da, Ia, Ta, _ = device_adaptive(hip, case.gpu, xq, case.nq, 10, 8, zero, flt)
    assert np.array_equal(bits(Du), bits(Da)) and np.array_equal(Iu, Ia) and np.array_equal(Tu, Ta)


def test_device_entry_equals_host_entry_and_its_tie_keys_are_those_of_the_shorter_search(case, hip):
    xq = hip.upload(case.Q)
    for name, rule in case.rules(24).items():
        p = case.p_q(24, rule)
        Dh, Ih = case.gpu.search_adaptive_sync(case.Q, 10, 24, rule)
        Dd, Id, Td, Pd = device_adaptive(hip, case.gpu, xq, case.nq, 10, 24, rule)
        assert np.array_equal(Pd, p), name
        assert np.array_equal(bits(Dd), bits(Dh)) and np.array_equal(Id, Ih), name
        assert ((Td == U64_MAX) == (Id == -1)).all()
        # the oracle's tie keys (shard visiting rank << 32 | position) of the search at n_probe = p_q, query by query
        for q in list(range(12)) + [case.zero_q]:
            _, _, To = case.orc.search_partial_batch(case.Q[q:q + 1], 10, int(p[q]), 0, 1)
            assert np.array_equal(Td[q], To[0]), (name, q, p[q])
    # ... and for every query: the plain device search of the queries that share a count
    rule = case.rules(24)["all"]
    p = case.p_q(24, rule)
    Dd, Id, Td, _ = device_adaptive(hip, case.gpu, xq, case.nq, 100, 24, rule)
    for v in np.unique(p):
        idx = np.nonzero(p == v)[0]
        Du, Iu, Tu = device_search(hip, case.gpu, hip.upload(case.Q[idx]), idx.size, 100, int(v))
        assert np.array_equal(bits(Dd[idx]), bits(Du)) and np.array_equal(Id[idx], Iu) and np.array_equal(Td[idx], Tu), v


# ---- the prune alone, on rows of probe_device ----
def test_prune_probes_device_on_rows_of_probe_device(case, hip):
    xq = hip.upload(case.Q)
    nq = case.nq
    for n_probe in (8, 24):
        P, probes_o, _, _ = case.rows(n_probe)
        for name, rule in case.rules(n_probe).items():
            p = case.p_q(n_probe, rule)
            probes, order, kept = hip.alloc(nq * P * 4), hip.alloc(nq * P * 4), hip.alloc(nq * 4)
            assert case.gpu.probe_device(xq, nq, n_probe, probes, order) == P
            o0 = hip.download(order, (nq, P), np.uint32).astype(np.int64)
            dev = vip.ProbeRule(rule.min_probe, rule.ratio2, rule.max_codes,
                                None if rule.n_probe_q is None else hip.upload(np.asarray(rule.n_probe_q, dtype=np.uint32)))
            case.gpu.prune_probes_device(xq, nq, P, probes, order, dev, kept)
            assert case.gpu.prune_stats()["probes_in"] == nq * P and case.gpu.prune_stats()["probes_kept"] == int(p.sum())
            r1, o1 = hip.download(probes, (nq, P), np.uint32).astype(np.int64), hip.download(order, (nq, P), np.uint32).astype(np.int64)
            assert np.array_equal(hip.download(kept, (nq,), np.uint32), p), name
            inside = np.arange(P)[None, :] < p[:, None]
            assert np.array_equal(r1, np.where(inside, probes_o, MARK)), name       # the oracle's prefix, then markers
            assert (o1[~inside] == MARK).all(), name
            for q in range(nq):     # a permutation of 0 .. p-1 that keeps the relative order of the old ranks
                assert np.array_equal(np.sort(o1[q, :p[q]]), np.arange(p[q])), (name, q)
                assert np.array_equal(np.argsort(o1[q, :p[q]]), np.argsort(o0[q, :p[q]])), (name, q)
            # pruning twice is pruning once
            case.gpu.prune_probes_device(xq, nq, P, probes, order, dev, kept)
            assert np.array_equal(hip.download(probes, (nq, P), np.uint32), r1) and np.array_equal(hip.download(order, (nq, P), np.uint32), o1)
            assert np.array_equal(hip.download(kept, (nq,), np.uint32), p), name
            assert case.gpu.prune_stats()["probes_in"] == int(p.sum())
            # the list phase over the pruned rows is the one-call entry
            D, I, T = hip.alloc(nq * 10 * 4), hip.alloc(nq * 10 * 8), hip.alloc(nq * 10 * 8)
            case.gpu.search_probed_device(xq, nq, 10, P, probes, order, D, I, T)
            Da, Ia, Ta, _ = device_adaptive(hip, case.gpu, xq, nq, 10, n_probe, rule)
            assert np.array_equal(bits(hip.download(D, (nq, 10), np.float32)), bits(Da)), name
            assert np.array_equal(hip.download(I, (nq, 10), np.int64), Ia) and np.array_equal(hip.download(T, (nq, 10), np.uint64), Ta), name


def test_prune_rejects_rows_a_list_phase_would_reject(case, hip):
    xq = hip.upload(case.Q[:4])
    bad = np.array([[0, 1, case.nlists, 2]] * 4, dtype=np.uint32)        # a list id out of range
    order = np.array([[0, 1, 2, 3]] * 4, dtype=np.uint32)
    with pytest.raises(vip.ViError) as e:
        case.gpu.prune_probes_device(xq, 4, 4, hip.upload(bad), hip.upload(order), vip.ProbeRule(ratio2=2.0))
    assert e.value.kind == "InvalidInput"
    with pytest.raises(vip.ViError) as e:     # n_probe_eff is the index's own
        case.gpu.prune_probes_device(xq, 4, case.nlists + 1, hip.upload(bad), hip.upload(order), vip.ProbeRule())
    assert e.value.kind == "InvalidInput"


# ---- two in-process ranks ----
@pytest.mark.parametrize("placement", [0, 1])
def test_two_ranks_merge_to_the_unpartitioned_adaptive_result(case, hip, placement):
    fx, world, nq, k, n_probe = case.fx, 2, case.nq, 10, 24
    parts = [vip.load(fx.idx, fx.sh, fx.dim, rank=r, world_size=world, placement=placement) for r in range(world)]
    assert sum(p.num_vectors for p in parts) == fx.n
    xq = hip.upload(case.Q)
    rule = case.rules(n_probe)["ratio"]
    p = case.p_q(n_probe, rule)
    De, Ie = case.expected(k, p)
    S = int(N.lib().vi_packed_result_bytes(nq, k))
    off_i = (nq * k * 4 + 7) // 8 * 8
    packed, Dm, Im, Pq = hip.alloc(world * S), hip.alloc(nq * k * 4), hip.alloc(nq * k * 8), hip.alloc(nq * 4)
    for r, part in enumerate(parts):
        b = packed + r * S
        part.search_adaptive_device(xq, nq, k, n_probe, rule, b, b + off_i, b + off_i + nq * k * 8, Pq)
        assert np.array_equal(hip.download(Pq, (nq,), np.uint32), p), r       # the coarse table is replicated
    N.check(N.lib().vi_merge_partials_packed_device(0, nq, k, world, packed, Dm, Im))
    assert np.array_equal(hip.download(Im, (nq, k), np.int64), Ie)
    assert np.array_equal(bits(hip.download(Dm, (nq, k), np.float32)), bits(De))
    # the seam: the coarse step split by query, the prune on every rank, the list phase over the pruned rows
    P = min(n_probe, case.nlists)
    probes, order = hip.alloc(nq * P * 4), hip.alloc(nq * P * 4)
    per = nq // world
    for r, part in enumerate(parts):
        assert part.probe_device(xq + r * per * fx.dim * 4, per, n_probe, probes + r * per * P * 4, order + r * per * P * 4) == P
    for r, part in enumerate(parts):
        pr, od = hip.upload(hip.download(probes, (nq, P), np.uint32)), hip.upload(hip.download(order, (nq, P), np.uint32))
        part.prune_probes_device(xq, nq, P, pr, od, rule)
        b = packed + r * S
        part.search_probed_device(xq, nq, k, P, pr, od, b, b + off_i, b + off_i + nq * k * 8)
    N.check(N.lib().vi_merge_partials_packed_device(0, nq, k, world, packed, Dm, Im))
    assert np.array_equal(hip.download(Im, (nq, k), np.int64), Ie)
    assert np.array_equal(bits(hip.download(Dm, (nq, k), np.float32)), bits(De))
    # a rank knows the resident lengths of its lists only
    for call in (lambda: parts[0].search_adaptive_sync(case.Q[:3], k, n_probe, vip.ProbeRule(max_codes=500)),
                 lambda: parts[1].search_adaptive_device(xq, nq, k, n_probe, vip.ProbeRule(max_codes=500), Dm, Im),
                 lambda: parts[1].prune_probes_device(xq, nq, P, probes, order, vip.ProbeRule(max_codes=500))):
        with pytest.raises(vip.ViError) as e:
            call()
        assert e.value.kind == "InvalidInput" and "max_codes" in str(e.value)


def test_gpu_searcher_with_a_rule(case, tmp_path):
    """distributed.gpu_searcher(...).search(rule=): the probe step, the prune and the list phase over the pruned rows behind
    one call.  torch has to initialise its HIP runtime before the library does, which a pytest process cannot arrange: the
    searcher runs in a child (adaptive_searcher_child.py); here its results are compared with the oracle's"""
    import os
    import subprocess
    import sys
    k, n_probe = 10, 24
    rule = case.rules(n_probe)["ratio"]
    np.savez(tmp_path / "in.npz", Q=case.Q)
    out = tmp_path / "out.npz"
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "adaptive_searcher_child.py")
    subprocess.run([sys.executable, child, case.fx.idx, case.fx.sh, str(case.fx.dim), str(k), str(n_probe), repr(rule.ratio2),
                    str(tmp_path / "in.npz"), str(out)], check=True, timeout=300)
    got = np.load(out)
    De, Ie = case.expected(k, case.p_q(n_probe, rule))
    for name in ("", "_ranks"):
        assert np.array_equal(got["I" + name], Ie) and np.array_equal(bits(got["D" + name]), bits(De)), name
    Dp, Ip = case.gpu.search_sync(case.Q, k, n_probe)
    assert np.array_equal(got["I_plain"], Ip) and np.array_equal(bits(got["D_plain"]), bits(Dp))
    assert not np.array_equal(Ip, Ie)       # (the rule changed some row)


# ---- what the saving shows in ----
def test_scanned_vectors_and_prune_stats(case):
    for n_probe in (8, 24):
        P = case.rows(n_probe)[0]
        lens = case.lens_of(n_probe)
        for name, rule in case.rules(n_probe).items():
            p = case.p_q(n_probe, rule)
            case.gpu.search_adaptive_sync(case.Q, 10, n_probe, rule)
            want = int(lens[np.arange(P)[None, :] < p[:, None]].sum())
            st = case.gpu.last_stats()
            assert st["scanned_vectors"] == want and st["n_probe_eff"] == P and st["nq"] == case.nq, (name, st, want)
            ps = case.gpu.prune_stats()
            assert (ps["probes_in"], ps["probes_kept"]) == (case.nq * P, int(p.sum())), (name, ps)
            assert ps["ms_prune"] == 0.0       # (taken under VI_PRUNE_TIMING only)
        case.gpu.search_sync(case.Q, 10, n_probe)
        assert case.gpu.last_stats()["scanned_vectors"] == int(lens.sum())


def test_prune_timing_is_opt_in(case, monkeypatch):
    monkeypatch.setenv("VI_PRUNE_TIMING", "1")
    case.gpu.search_adaptive_sync(case.Q, 10, 8, case.rules(8)["ratio"])
    assert case.gpu.prune_stats()["ms_prune"] > 0.0


# ---- errors that need an index ----
def test_errors(case, valu, hip):  # noqa: F811
    rule = vip.ProbeRule(ratio2=2.0)
    other = vip.load(case.fx.idx, case.fx.sh, case.fx.dim)
    for idx, Q in ((other, case.Q[:3]), (valu.gpu, valu.Q[:3])):    # a filter of another handle, of another index
        with pytest.raises(vip.ViError) as e:
            idx.search_adaptive_sync(Q, 5, 4, rule, filter=case.fx.filter(TENTH))
        assert e.value.kind == "InvalidInput"
    for bad in (float("nan"), float("inf"), -2.0, 0.5):
        case.gpu.search_adaptive_sync(case.Q[:3], 5, 4, rule)
        assert case.gpu.prune_stats()["probes_in"] == 12
        with pytest.raises(vip.ViError) as e:
            case.gpu.search_adaptive_sync(case.Q[:3], 5, 4, vip.ProbeRule(ratio2=bad))
        assert e.value.kind == "InvalidInput" and "ratio2" in str(e.value)
        assert case.gpu.prune_stats() == {"probes_in": 0, "probes_kept": 0, "ms_prune": 0.0}     # zeros after a failed call
    for k, n_probe in ((0, 4), (5, 0)):
        with pytest.raises(vip.ViError) as e:
            case.gpu.search_adaptive_sync(case.Q[:3], k, n_probe, rule)
        assert e.value.kind == "InvalidInput"
    with pytest.raises(RuntimeError):
        case.gpu.search_adaptive_sync(case.Q[:3, :5], 5, 4, rule)
    with pytest.raises(RuntimeError):
        case.gpu.search_adaptive_sync(case.Q[:3], 5, 4, vip.ProbeRule(n_probe_q=[1, 2]))      # one count per query


# ---- the other layers ----
def test_request_and_adapter_layers(case):
    from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig
    from vector_indexer_py.harness import FaissStyleAdapter
    ratio2, budget = case.ratio_from_data(24), case.budget_from_data(24)
    rule = vip.ProbeRule(ratio2=ratio2, max_codes=budget)
    De, Ie = case.expected(10, case.p_q(24, rule))
    ad = FaissStyleAdapter(case.gpu)
    ad.nprobe, ad.probe_ratio2, ad.max_codes = 24, ratio2, budget
    D, I = ad.search(case.Q, 10)
    assert np.array_equal(I, Ie) and np.array_equal(bits(D), bits(De))
    ad.probe_ratio2, ad.max_codes = 0.0, 0
    assert np.array_equal(ad.search(case.Q, 10)[1], case.gpu.search_sync(case.Q, 10, 24)[1])
    vi = VectorIndexer.load(VectorIndexerConfig.new(case.fx.dim).with_index_dir(case.fx.idx).with_shards_dir(case.fx.sh))
    for q in (0, case.zero_q, 50):
        req = vi.search_request(case.Q[q]).with_k(10).with_n_probe(24).with_probe_ratio(ratio2).with_max_codes(budget)
        got = vi.search(req)
        n = int((Ie[q] >= 0).sum())
        assert [r.external_id for r in got] == Ie[q, :n].tolist()
        assert np.array_equal(bits(np.array([r.distance for r in got], dtype=np.float32)), bits(De[q, :n]))
