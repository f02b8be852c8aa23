"""GPU: clustering the stored records by radius — vi_indexer_cluster_radius (host and device form).

The contract (include/vi_amd.h): participants are the records the filter admits; row R(j) is row j of the radius graph
with the record itself excluded, read as a set; a ~ b iff either row holds the other; core = degree + 1 >= min_pts;
clusters = components of the core records, labelled by their lowest list-order ordinal; a border record takes the cluster
of its lowest adjacent core; the rest is noise (-1).  The expected values come from the untouched oracle:
Fixture.sequences(X_e[chunk], p) is the full sorted candidate sequence of EVERY record in export order; the entries with
I >= 0, D <= float32(radius2), not the row's own entry and admitted by the filter are the row, ids mapped to ordinals
through export(); cluster_cases applies the definition.  Everything is exact: no tolerance appears."""
import ctypes as C
import threading

import numpy as np
import pytest

import vector_indexer_py as vip
from cluster_cases import EPS2, NCOPIES, NLIST, NOISE, cluster_reference, cluster_reference_csr, planted
from test_id_filter_gpu import HALF, bits, u64
from test_range_similar_gpu import radii_of
from test_similar_search_gpu import ORACLE_CHUNK, Fixture, own_entries
from vector_indexer_py import _native as N

pytestmark = pytest.mark.gpu

INF = float("inf")
MIN_PTS = [0, 1, 2, 5, 10_000]
COUNTS = ("n_core", "n_border", "n_noise")


class Case:
    """a Fixture with unique ids, its export order, and the oracle's rows in that order as CSR of ordinals — made once
    per (n_probe, radius, filter) and shared by the tests, never changed"""

    def __init__(self, fx):
        self.fx, self.n, self.gpu = fx, fx.n, fx.gpu
        self.ext_e, self.X_e, self.ts_e, self.where_e = fx.gpu.export()
        assert np.unique(self.ext_e).size == self.n and np.array_equal(np.sort(self.ext_e), np.sort(fx.ext))
        assert (np.diff(self.where_e.astype(np.int64)) > 0).all()        # list order: `where` ascends
        self._order = np.argsort(self.ext_e)
        self._sorted = self.ext_e[self._order]
        self.ord_of_row = self.ordinals(fx.ext.astype(np.int64))         # data row of fx.X -> list-order ordinal
        self.list_of = (self.where_e >> np.uint64(32)).astype(np.int64)  # ordinal -> list
        self._csr = {}

    def ordinals(self, I):
        return self._order[np.searchsorted(self._sorted, np.asarray(I).astype(np.uint64))]

    def csr(self, n_probe, radii, part=None, key=None):
        """{radius: (lims, cols)} of every record's row in export order; part: bool[n] by ordinal, the filter's participants"""
        p = min(n_probe, self.fx.nlists)
        todo = [r for r in radii if (p, float(r), key) not in self._csr]
        if todo:
            out = {r: ([], []) for r in todo}
            for at in range(0, self.n, ORACLE_CHUNK):
                D, I = self.fx.sequences(self.X_e[at:at + ORACLE_CHUNK], p)
                valid = I >= 0
                keep = valid & ~own_entries(D, I, self.ext_e[at:at + ORACLE_CHUNK])
                if part is not None:
                    adm = np.zeros_like(valid)
                    adm[valid] = part[self.ordinals(I[valid])]
                    keep &= adm
                for r in todo:
                    k = keep & (D <= np.float32(r))
                    out[r][0].append(k.sum(axis=1))
                    out[r][1].append(self.ordinals(I[k]))
            for r in todo:
                lims = np.concatenate([[0], np.cumsum(np.concatenate(out[r][0]))]).astype(np.int64)
                cols = np.concatenate(out[r][1]).astype(np.int64)
                lims.setflags(write=False), cols.setflags(write=False)
                self._csr[(p, float(r), key)] = (lims, cols)
        return {r: self._csr[(p, float(r), key)] for r in radii}

    def expected(self, n_probe, r, min_pts, part=None, key=None):
        lims, cols = self.csr(n_probe, [r], part, key)[r]
        return cluster_reference_csr(lims, cols, self.n, min_pts, part)

    def one_directional(self, n_probe, r):
        lims, cols = self.csr(n_probe, [r])[r]
        a = np.repeat(np.arange(self.n), np.diff(lims))
        fwd = set((a * self.n + cols).tolist())
        return sum(1 for x, y in zip(a.tolist(), cols.tolist()) if y * self.n + x not in fwd)


def check(case, n_probe, r, min_pts, flt=None, part=None, key=None, what=""):
    """one call against the oracle: labels, degree, n_clusters and the counts of cluster_stats, exactly"""
    want_l, want_d, want_nc, want_c = case.expected(n_probe, r, min_pts, part, key)
    labels, degree = case.gpu.cluster_radius(r, n_probe, min_pts, filter=flt, with_degree=True)
    st = case.gpu.cluster_stats()
    what = f"{what} n_probe {n_probe} radius {r} min_pts {min_pts}"
    assert labels.dtype == np.int64 and degree.dtype == np.uint32 and labels.shape == degree.shape == (case.n,)
    bad = np.nonzero(labels != want_l)[0]
    assert bad.size == 0, (what, "labels", bad.size, bad[:8], labels[bad[:8]], want_l[bad[:8]])
    assert np.array_equal(degree, want_d), (what, "degree", np.nonzero(degree != want_d)[0][:8])
    assert st["n_clusters"] == want_nc, (what, st, want_nc)
    assert {k: st[k] for k in COUNTS} == {k: want_c[k] for k in COUNTS}, (what, st, want_c)
    assert st["hits"] == want_c["hits"] and st["rows"] == case.n, (what, st, want_c)
    assert st["passes"] == (2 if min_pts >= 2 else 1), (what, st)
    return labels, degree, st


def sizes_of(labels):
    return np.bincount(labels[labels >= 0], minlength=labels.size)


def parts_by_ordinal(case, parts):
    """the planted shapes by list-order ordinal: arrays ascending, the two hubs single ordinals"""
    return {k: int(case.ord_of_row[v]) if np.ndim(v) == 0 else np.sort(case.ord_of_row[v]) for k, v in parts.items()}


# ---- fixtures ----
@pytest.fixture(scope="module")
def plant(tmp_path_factory):        # D = 32, 24 lists of about 145 records that end in a ragged block: the MFMA engine
    X, parts = planted()
    case = Case(Fixture(tmp_path_factory.mktemp("cplant"), X, NLIST))
    case.parts = parts_by_ordinal(case, parts)
    return case


@pytest.fixture(scope="module")
def plant104(tmp_path_factory):     # the same records in 104 requested lists: rows that are one-directional; n_probe 100 > 64
    X, parts = planted()
    case = Case(Fixture(tmp_path_factory.mktemp("cplant104"), X, 104))
    case.parts = parts_by_ordinal(case, parts)
    return case


@pytest.fixture(scope="module")
def valu(tmp_path_factory):         # D % 4 != 0: the generic engine's radius form
    rng = np.random.default_rng(3)
    return Case(Fixture(tmp_path_factory.mktemp("cvalu"), rng.standard_normal((6000, 10)).astype(np.float32), 24))


@pytest.fixture(scope="module")
def bytes8(tmp_path_factory):       # 8-bit descriptors: the int8 rank kernel
    rng = np.random.default_rng(5)
    centers = rng.integers(40, 216, size=(24, 128))
    X = np.clip(centers[rng.integers(0, 24, 6000)] + rng.integers(-40, 41, size=(6000, 128)), 0, 254).astype(np.float32)
    return Case(Fixture(tmp_path_factory.mktemp("cbytes"), X, 24))


@pytest.fixture(scope="module")
def hip():
    from hiprt import Hip
    h = Hip()
    yield h
    h.close()


# ---- 1. against the oracle on the planted set ----
@pytest.mark.parametrize("n_probe", [1, 8, 10_000])
def test_against_the_oracle_on_the_planted_set(plant, n_probe):
    case = plant
    radii = [0.0, EPS2, -1.0, INF]
    case.csr(n_probe, radii)
    for r in radii:
        g = case.gpu.radius_graph(r, n_probe, exclude_self=True)
        graph_total = g.total
        g.free()
        for min_pts in MIN_PTS:
            labels, degree, st = check(case, n_probe, r, min_pts, what="planted")
            assert st["hits"] == graph_total, (n_probe, r, min_pts, st, graph_total)
        if r != INF:    # the plain-Python statement of the definition itself, where its loop is affordable
            lims, cols = case.csr(n_probe, [r])[r]
            rows = [cols[lims[j]:lims[j + 1]] for j in range(case.n)]
            for min_pts in (1, 5):
                a, b = cluster_reference(rows, case.n, min_pts), case.expected(n_probe, r, min_pts)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    # what the cases rely on, from the oracle's rows
    P = case.parts
    l1, d1, nc1, c1 = case.expected(n_probe, EPS2, 1)
    big = np.nonzero(sizes_of(l1) > 1)[0]
    l0 = case.expected(n_probe, 0.0, 1)[0]
    assert sorted(sizes_of(l0)[sizes_of(l0) > 1].tolist()) == [NCOPIES] and (d1[P["copies"]] >= NCOPIES - 1).all()
    assert (case.expected(n_probe, -1.0, 1)[0] == np.arange(case.n)).all() and (case.expected(n_probe, -1.0, 2)[0] == NOISE).all()
    assert (case.expected(n_probe, INF, 10_000)[0] == NOISE).all()
    if n_probe == 1:
        assert big.size > 4, "the chain and the walk do not fall apart where they cross lists"
    else:
        assert sorted(sizes_of(l1)[big].tolist()) == [2 * 31 + 1, NCOPIES, 200, 200]
        assert np.unique(l1[P["chain"]]).size == 1 and np.unique(l1[P["walk"]]).size == 1
        assert np.unique(case.list_of[P["chain"]]).size >= 3, "no cluster touches three lists"
        assert l1[P["hub1"]] == l1[P["hub2"]] == l1[P["bridge"][0]]      # the two stars joined through the bridge
        l5, d5, nc5, c5 = case.expected(n_probe, EPS2, 5)
        assert nc5 == 3 and c5["n_border"] == 61 and c5["n_core"] == NCOPIES + 2
        assert (l5[P["chain"]] == NOISE).all() and (l5[P["walk"]] == NOISE).all()
        hubs = sorted([int(P["hub1"]), int(P["hub2"])])
        assert l5[hubs[0]] != l5[hubs[1]] and d5[P["bridge"][0]] == 2        # a border with cores of two clusters ...
        assert l5[P["bridge"][0]] == l5[hubs[0]] == hubs[0]                  # ... is labelled with the lower-ordinal hub
        assert (d5[P["copies"]] == NCOPIES - 1).all()                         # rows of 69 entries: across a wave's 64 lanes
    if n_probe == 10_000:
        assert case.expected(n_probe, INF, 5)[2] == 1 and (case.expected(n_probe, INF, 5)[1] == case.n - 1).all()


# ---- 2. the three engines ----
@pytest.mark.parametrize("name", ["valu", "bytes8"])
def test_generic_and_int8_engines(name, request):
    case = request.getfixturevalue(name)
    radii, _ = radii_of(case.fx)
    r = float(radii["r1"])
    want = case.expected(8, r, 1)
    assert 1 < want[2] < case.n and (sizes_of(want[0]) > 2).any(), (want[2], case.n)
    for min_pts in (1, 3):
        check(case, 8, r, min_pts, what=name)
    want3 = case.expected(8, r, 3)
    assert want3[3]["n_core"] > 0 and want3[3]["n_border"] > 0 and want3[3]["n_noise"] > 0, want3[3]


@pytest.mark.parametrize("n_probe", [1, 2, 100])
def test_104_lists_one_directional_rows_and_n_probe_100(plant104, n_probe):
    case = plant104
    assert case.fx.nlists > 100
    want = case.expected(n_probe, EPS2, 1)
    assert 1 < want[2] < case.n
    if n_probe in (1, 2):
        assert case.one_directional(n_probe, EPS2) >= 1, "every edge is present in both rows"
    for min_pts in (1, 5):
        check(case, n_probe, EPS2, min_pts, what="104 lists")
    if n_probe == 100:
        st = case.gpu.last_stats()
        assert st["n_probe_eff"] == 100 and st["rank_mode"] == 0, st
        assert sorted(sizes_of(want[0])[sizes_of(want[0]) > 1].tolist()) == [2 * 31 + 1, NCOPIES, 200, 200]


# ---- 3. chunking ----
@pytest.mark.parametrize("chunk", ["7", "64", "1000", None])
def test_chunks_give_identical_arrays(plant, chunk, monkeypatch):
    case = plant
    if chunk is None:
        monkeypatch.delenv("VI_GRAPH_CHUNK", raising=False)
    else:
        monkeypatch.setenv("VI_GRAPH_CHUNK", chunk)
    C_ = int(chunk or 65536)
    for min_pts in (1, 5):
        labels, degree, st = check(case, 8, EPS2, min_pts, what=f"chunk {chunk}")
        assert st["chunk_rows"] == C_, st       # the knob reached the call
    if chunk is not None:
        l1 = case.expected(8, EPS2, 1)[0]
        members = np.nonzero(l1 == l1[case.parts["chain"][0]])[0]
        assert np.unique(members // C_).size > 1, "no cluster spans a chunk border"
        a = np.repeat(np.arange(case.n), np.diff(case.csr(8, [EPS2])[EPS2][0]))
        b = case.csr(8, [EPS2])[EPS2][1]
        assert (a // C_ != b // C_).any()        # an edge whose two records are searched in different chunks


def test_timing_report_counts_the_consumer_kernels_bytes(plant, monkeypatch):
    """link_bytes is what cluster_degree_kernel / cluster_link_kernel read and write per pass: 32 bytes per row (its
    bounds, slot, allow word and degree) and the 8-byte slot of every searched entry — the entries of the radius graph
    with the record itself kept.  It is counted with or without VI_SIMILAR_TIMING; the four spans only with it."""
    case = plant
    g = case.gpu.radius_graph(EPS2, 8, exclude_self=False)
    T = g.total
    g.free()
    monkeypatch.setenv("VI_GRAPH_CHUNK", "4")
    monkeypatch.setenv("VI_SIMILAR_TIMING", "1")
    for min_pts, passes in ((1, 1), (2, 2)):
        case.gpu.cluster_radius(EPS2, 8, min_pts)
        st = case.gpu.cluster_stats()
        print("cluster_stats", min_pts, T, st)
        assert st["passes"] == passes and st["chunk_rows"] == 4, st
        assert st["link_bytes"] == passes * (case.n * 32 + T * 8), (st, T)
        assert st["ms_resolve"] > 0 and st["ms_search"] > 0 and st["ms_link"] > 0 and st["ms_label"] > 0, st
    monkeypatch.delenv("VI_SIMILAR_TIMING")
    case.gpu.cluster_radius(EPS2, 8, 1)
    st = case.gpu.cluster_stats()
    assert st["link_bytes"] == case.n * 32 + T * 8, (st, T)
    assert st["ms_resolve"] == st["ms_search"] == st["ms_link"] == st["ms_label"] == 0.0, st


# ---- 4. composition: the reference applied to the library's own radius graph ----
@pytest.mark.parametrize("name", ["plant", "plant104", "valu", "bytes8"])
def test_labels_are_the_reference_applied_to_the_librarys_own_radius_graph(name, request):
    case = request.getfixturevalue(name)
    r = EPS2 if name.startswith("plant") else float(radii_of(case.fx)[0]["r1"])
    for n_probe, min_pts in ((2, 1), (8, 4)):
        g = case.gpu.radius_graph(r, n_probe, exclude_self=True)
        lims, _, I = g.copy()
        g.free()
        want = cluster_reference_csr(lims.astype(np.int64), case.ordinals(I), case.n, min_pts)
        labels, degree = case.gpu.cluster_radius(r, n_probe, min_pts, with_degree=True)
        assert np.array_equal(labels, want[0]) and np.array_equal(degree, want[1]), (name, n_probe, min_pts)
        assert np.array_equal(degree, np.diff(lims.astype(np.int64)).astype(np.uint32))
        assert case.gpu.cluster_stats()["n_clusters"] == want[2]


# ---- 5. with a filter ----
def test_with_a_filter_and_a_cluster_that_loses_its_representative(plant):
    case, P = plant, plant.parts
    free = case.expected(8, EPS2, 1)[0]
    reps = [int(P["copies"].min()), int(P["chain"].min()), int(min(P["hub1"], P["hub2"]))]
    assert all(free[r] == r or r == reps[2] for r in reps)
    deny_ord = np.concatenate([reps, np.arange(0, case.n, 9)])
    deny = case.ext_e[deny_ord]
    flt = case.gpu.filter_timestamps(*HALF) & case.gpu.filter_ids(deny, exclude=True)
    part = (case.ts_e >= np.uint64(HALF[0])) & (case.ts_e <= np.uint64(HALF[1])) & ~np.isin(case.ext_e, deny)
    assert flt.num_allowed == int(part.sum()) and 0 < part.sum() < case.n
    for r in (EPS2, 0.0):
        for min_pts in (1, 2, 5):
            labels, degree, st = check(case, 8, r, min_pts, flt=flt, part=part, key="half", what="filtered")
            assert (labels[~part] == NOISE).all() and (degree[~part] == 0).all()
            assert st["n_core"] + st["n_border"] + st["n_noise"] == int(part.sum())
    labels = case.gpu.cluster_radius(0.0, 8, 1, filter=flt)
    left = P["copies"][part[P["copies"]]]
    assert 1 < left.size < NCOPIES and not part[reps[0]]
    assert (labels[left] == left.min()).all() and left.min() != reps[0]      # the copies that take part have a new representative
    assert (labels[part] >= 0).all() and (labels[labels >= 0] <= np.nonzero(labels >= 0)[0]).all()


# ---- 6. duplicate ids: slot, not id; bits, not id ----
def test_duplicate_ids_at_radius_zero(tmp_path_factory):
    rng = np.random.default_rng(23)
    n = 1500
    X = rng.standard_normal((n, 32)).astype(np.float32)
    ext = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    ext[900] = ext[100]                   # one id, two vectors
    X[1000] = X[200]                      # one vector, two ids
    ext[1100], X[1100] = ext[300], X[300]   # both shared
    fx = Fixture(tmp_path_factory.mktemp("cdups"), X, 8, ext=ext)
    ext_e, X_e, _, where_e = fx.gpu.export()

    def ordinal(where):     # ordinals come from `where`, which names a record whatever ids repeat
        o = np.searchsorted(where_e, where)
        assert (where_e[o] == where).all()
        return o

    cnt, _, _, w = fx.gpu.get([ext[200], ext[1000]])
    assert cnt.tolist() == [1, 1]
    o200, o1000 = ordinal(w).tolist()
    shared = np.nonzero(ext_e == ext[100])[0]          # the two carriers of one id: different vectors
    both = np.nonzero(ext_e == ext[300])[0]            # id and vector shared
    assert shared.size == 2 and both.size == 2 and not np.array_equal(X_e[shared[0]], X_e[shared[1]])
    assert np.array_equal(X_e[both[0]], X_e[both[1]]) and np.array_equal(X_e[o200], X_e[o1000])
    cnt, _, _, w = fx.gpu.get([ext[100]])
    assert cnt[0] == 2 and ordinal(w)[0] == shared[0]  # get() names the first carrier in list order
    for n_probe in (8, 10_000):
        labels, degree = fx.gpu.cluster_radius(0.0, n_probe, 1, with_degree=True)
        assert labels[o200] == labels[o1000] == min(o200, o1000) and degree[o200] == degree[o1000] == 1
        assert labels[shared[0]] == shared[0] and labels[shared[1]] == shared[1]      # one id, two vectors: not joined
        assert labels[both[0]] == labels[both[1]] == both[0]
        twins = np.array([o200, o1000, both[0], both[1]])
        rest = np.setdiff1d(np.arange(n), twins)
        assert (labels[rest] == rest).all() and (degree[rest] == 0).all()
        assert fx.gpu.cluster_stats()["n_clusters"] == n - 2
        l2 = fx.gpu.cluster_radius(0.0, n_probe, 2)
        assert (l2[twins] == labels[twins]).all() and (l2[rest] == NOISE).all()


# ---- 7. the dedup workflow, and the errors that need an update ----
def test_dedup_workflow_retain_then_add(tmp_path_factory):
    X, parts = planted()
    fx = Fixture(tmp_path_factory.mktemp("cdedup"), X, NLIST)
    gpu, n = fx.gpu, fx.n
    labels = gpu.cluster_radius(0.0, 8)
    keep = labels == np.arange(n)
    assert int((~keep).sum()) == NCOPIES - 1
    flt = gpu.filter_mask(keep)
    assert gpu.retain(flt) == NCOPIES - 1
    assert gpu.num_vectors == n - (NCOPIES - 1)
    # the filter was made before the update: rejected, nothing written
    out = np.full(gpu.num_vectors, 7, dtype=np.int64)
    assert N.lib().vi_indexer_cluster_radius(gpu._h, flt._h, 0.0, 8, 1, N.ptr(out), None, None) == N.VI_ERR_INVALID_INPUT
    assert N.lib().vi_last_error() and (out == 7).all()
    labels = gpu.cluster_radius(0.0, 8)
    assert np.array_equal(labels, np.arange(n - (NCOPIES - 1)))      # no cluster of more than one record is left
    assert gpu.cluster_stats()["n_clusters"] == n - (NCOPIES - 1)
    # three copies of a stored vector under new ids: the four share the old record's ordinal
    ext_e, X_e, _, _ = gpu.export()
    own_first = ~np.isin(ext_e, fx.ext[fx.unprobed])        # records whose own list is the first their vector probes
    old = int(np.nonzero(own_first)[0][1234])
    new_ids = u64([1 << 50, (1 << 50) + 1, (1 << 50) + 2])
    gpu.add(np.repeat(X_e[old:old + 1], 3, axis=0), ext_ids=new_ids)
    ext_2, X_2, _, _ = gpu.export()
    o_old = int(np.nonzero(ext_2 == ext_e[old])[0][0])
    o_new = np.nonzero(np.isin(ext_2, new_ids))[0]
    assert o_new.size == 3 and (o_new > o_old).all() and all(np.array_equal(X_2[o], X_2[o_old]) for o in o_new)
    labels, degree = gpu.cluster_radius(0.0, 8, with_degree=True)
    assert labels[o_old] == o_old and (labels[o_new] == o_old).all() and degree[o_old] == 3 and (degree[o_new] == 3).all()
    assert gpu.cluster_stats()["n_clusters"] == gpu.num_vectors - 3


# ---- 8. the device form ----
def test_device_form_equals_host_form_and_errors_leave_the_buffers_alone(plant, hip):
    case, n = plant, plant.n
    L = N.lib()
    for min_pts in (1, 5):
        labels, degree = case.gpu.cluster_radius(EPS2, 8, min_pts, with_degree=True)
        nc_host = C.c_uint64(7)
        N.check(L.vi_indexer_cluster_radius(case.gpu._h, None, EPS2, 8, min_pts, None, None, C.byref(nc_host)))
        pl, pd = hip.upload(np.full(n, 7, dtype=np.int64)), hip.upload(np.full(n, 7, dtype=np.uint32))
        nc = case.gpu.cluster_radius_device(pl, pd, EPS2, 8, min_pts)
        assert nc == nc_host.value == case.expected(8, EPS2, min_pts)[2]
        assert np.array_equal(hip.download(pl, (n,), np.int64), labels) and np.array_equal(hip.download(pd, (n,), np.uint32), degree)
        # either output alone
        pl2 = hip.upload(np.full(n, 7, dtype=np.int64))
        assert case.gpu.cluster_radius_device(pl2, 0, EPS2, 8, min_pts) == nc
        assert np.array_equal(hip.download(pl2, (n,), np.int64), labels)
        pd2 = hip.upload(np.full(n, 7, dtype=np.uint32))
        N.check(L.vi_indexer_cluster_radius_device(case.gpu._h, None, EPS2, 8, min_pts, None, pd2, None))    # only degrees: one pass
        assert np.array_equal(hip.download(pd2, (n,), np.uint32), degree)
        st = case.gpu.cluster_stats()
        assert st["passes"] == 1 and st["hits"] == int(degree.sum()) and st["n_clusters"] == 0, st
    pl, pd = hip.upload(np.full(n, 7, dtype=np.int64)), hip.upload(np.full(n, 7, dtype=np.uint32))
    nc = C.c_uint64(7)
    for r, p in ((float("nan"), 8), (1.0, 0)):
        assert L.vi_indexer_cluster_radius_device(case.gpu._h, None, r, p, 1, pl, pd, C.byref(nc)) == N.VI_ERR_INVALID_INPUT
        assert nc.value == 7 and (hip.download(pl, (n,), np.int64) == 7).all() and (hip.download(pd, (n,), np.uint32) == 7).all()


# ---- 9. errors ----
def test_errors_write_nothing(plant):
    case, n = plant, plant.n
    L = N.lib()
    labels, degree, nc = np.full(n, 7, dtype=np.int64), np.full(n, 7, dtype=np.uint32), C.c_uint64(7)

    def call(h, r, p, flt=None, outputs=True):
        if not outputs:
            return L.vi_indexer_cluster_radius(h, flt, r, p, 1, None, None, None)
        return L.vi_indexer_cluster_radius(h, flt, r, p, 1, N.ptr(labels), N.ptr(degree), C.byref(nc))

    other = case.fx.open()
    part = case.fx.open(rank=0, world_size=2)
    foreign = other.filter_timestamps(*HALF)
    cases = {"NaN": lambda: call(case.gpu._h, float("nan"), 8), "n_probe 0": lambda: call(case.gpu._h, 1.0, 0),
             "all outputs NULL": lambda: call(case.gpu._h, 1.0, 8, outputs=False),
             "a filter of another handle": lambda: call(case.gpu._h, 1.0, 8, foreign._h),
             "a partitioned handle": lambda: call(part._h, 1.0, 8)}
    for what, c in cases.items():
        assert c() == N.VI_ERR_INVALID_INPUT, what
        assert L.vi_last_error(), what
        assert (labels == 7).all() and (degree == 7).all() and nc.value == 7, what
    assert call(part._h, 1.0, 8) == N.VI_ERR_INVALID_INPUT and b"partitioned" in L.vi_last_error()
    with pytest.raises(vip.ViError) as e:
        case.gpu.cluster_radius(float("nan"), 8)
    assert e.value.kind == "InvalidInput"
    # the handle stays usable
    check(case, 8, EPS2, 5, what="after the errors")


# ---- 10. threads ----
def test_four_threads_cluster_beside_searches_on_one_handle(plant):
    case = plant
    want = [case.gpu.cluster_radius(EPS2, 8, m, with_degree=True) for m in (1, 5)]
    Q = case.X_e[:64]
    want_s = case.gpu.search_sync(Q, 10, 8)
    errors = []

    def worker(t):
        try:
            for _ in range(3):
                labels, degree = case.gpu.cluster_radius(EPS2, 8, (1, 5)[t % 2], with_degree=True)
                assert np.array_equal(labels, want[t % 2][0]) and np.array_equal(degree, want[t % 2][1])
                assert case.gpu.cluster_stats()["passes"] == 1 + t % 2      # the figures are the calling thread's own
                D, I = case.gpu.search_sync(Q, 10, 8)
                assert np.array_equal(I, want_s[1]) and np.array_equal(bits(D), bits(want_s[0]))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(t,), daemon=True) for t in range(4)]
    [t.start() for t in threads]
    [t.join(timeout=60) for t in threads]
    assert not any(t.is_alive() for t in threads), "a thread is still waiting"
    assert not errors, errors
    assert np.array_equal(want[1][0], case.expected(8, EPS2, 5)[0])


# ---- 11. the Python surface ----
def test_python_surface(plant):
    from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig
    case, P = plant, plant.parts
    ix = VectorIndexer.load(VectorIndexerConfig.new(case.fx.dim).with_index_dir(case.fx.idx).with_shards_dir(case.fx.sh))
    groups = ix.duplicate_groups()
    assert groups == [[int(e) for e in case.ext_e[P["copies"]]]]        # exactly the 70 copies, in list order
    groups = ix.duplicate_groups(1.0, n_probe=8)
    l1 = case.expected(8, EPS2, 1)[0]
    reps = np.nonzero(sizes_of(l1) > 1)[0]
    assert len(groups) == 4 and [len(g) for g in groups] == sizes_of(l1)[reps].tolist()
    assert groups == [[int(e) for e in case.ext_e[l1 == r]] for r in reps]     # members in list order, groups by representative
    assert ix.duplicate_groups(1.0, n_probe=8, min_size=100) == [g for g in groups if len(g) >= 100] and len(groups[0]) > 0
    assert ix.duplicate_groups(-1.0) == []
    labels = case.gpu.cluster_radius(EPS2, 8)
    assert isinstance(labels, np.ndarray) and np.array_equal(labels, l1)
    st = case.gpu.cluster_stats()
    assert set(st) == {f for f, _ in N.ClusterStats._fields_} and st["link_bytes"] > 0
