"""GPU: lists at and past 64 segments of 32 blocks (131 072 vectors), probed three at a time — two fixed capacities of the
MFMA engine that no smaller fixture reaches, on every rank kernel, the top-k and the radius select, and the engines
that share the segmentation rule.

  * list_segments (scan.hpp) cuts a list into at most 64 segments.  Up to 64 x 32 blocks the segment is the configured
    32 blocks (a shift); past that it is ceil(blocks / 64) — 33 blocks for 131 073 vectors, 35 for 140 000: odd, no
    multiple of 8, a tile count that is no multiple of 16 — and a segment holds more than 16 pair records (20 here), so
    the record loops of both selects run more than once.
  * both selects keep the first kCacheG = 256 group records of a query in LDS and read the rest from global memory.  A
    query has 2 x (segments of its probed lists) records: 128 + 126 + 126 = 380 at n_probe 3.  n_probe 1 stays within 128
    and isolates the first limit from the second.

Three well separated clusters of exactly 131 072, 131 073 and 140 000 points make the oracle's k-means (nlist 3) build
exactly these lists; the test asserts it.  A query on a stored vector has all its near neighbours in the list probed
first — inside the cached records — so half the queries sit at the circumcentre of the three cluster centres, where the
neighbours come from all three lists alike; that too is asserted from the oracle's result.  Everything is compared with
the untouched oracle as in test_filtered_search_gpu.py and test_range_search_gpu.py: ids, distance bits, lims — exact."""
import contextlib

import numpy as np
import pytest

from test_filtered_search_gpu import EVERYTHING, NOTHING, ONLY_NOW, TENTH, Fixture, bits
from test_range_search_gpu import INF, check, expected, median_radius

pytestmark = pytest.mark.gpu

SIZES = (131072, 131073, 140000)
N = sum(SIZES)
NEAR, CENTRE = slice(0, 24), slice(24, 48)      # 8 stored vectors + 16 next to stored vectors; 24 at the circumcentre
TOPK = [(1, 1), (10, 2), (10, 3), (100, 3), (128, 3)]


class Part(Fixture):
    """some of a fixture's queries as a batch of their own (a radius is per call), sharing index, filters and the
    oracle's sequences"""

    def __init__(self, whole, rows):
        self.__dict__.update(whole.__dict__)
        self.whole, self.rows, self.Q = whole, rows, np.ascontiguousarray(whole.Q[rows])

    def full(self, n_probe):
        return tuple(x[self.rows] for x in self.whole.full(n_probe))


def make(root, dim, integer):
    """three clusters around 0, 60 e0 and 60 e1 (8-bit: 60 everywhere, 190 in dimension 0 or 1), rows shuffled"""
    rng = np.random.default_rng(2)
    centres = np.full((3, dim), 60.0 if integer else 0.0)
    centres[1, 0] = centres[2, 1] = 190.0 if integer else 60.0
    if integer:
        X = np.concatenate([np.clip(c + rng.integers(-40, 41, size=(s, dim)), 0, 255) for c, s in zip(centres, SIZES)])
    else:
        X = np.concatenate([c + rng.standard_normal((s, dim)) for c, s in zip(centres, SIZES)])
    perm = rng.permutation(N)
    X, label = X.astype(np.float32)[perm], np.repeat(np.arange(3), SIZES)[perm]
    near = X[rng.integers(0, N, 16)]
    near = near + (rng.integers(-3, 4, size=near.shape) if integer else 0.3 * rng.standard_normal(near.shape))
    cc = (centres[1] + centres[2]) / 2.0      # (the right angle is at centre 0) equidistant from the three: (30, 30, 0, ...) / (125, 125, 60, ...)
    cc = cc + (rng.integers(-1, 2, size=(24, dim)) if integer else 0.02 * rng.standard_normal((24, dim)))
    Q = np.concatenate([X[:8], near, cc]).astype(np.float32)
    fx = Fixture(root, X, 3, np.clip(Q, 0, 254) if integer else Q)
    fx.label, fx.want = label, {}
    # the lists are the clusters — on the oracle's side, and on the GPU's: a query on a centroid probes that list alone
    assert fx.nlists == 3 and sorted(int(fx.orc.list_len(c)) for c in range(3)) == list(SIZES)
    cent, _ = fx.orc.centroids()
    for c in range(3):
        fx.gpu.search_sync(cent[c:c + 1], 1, 1)
        assert fx.gpu.last_stats()["scanned_vectors"] == fx.orc.list_len(c)
    return fx


@pytest.fixture(scope="module")
def real8(tmp_path_factory):
    return make(tmp_path_factory.mktemp("real8"), 8, False)


@pytest.fixture(scope="module")
def wide132(tmp_path_factory):      # D > 128: the wide rank kernel
    return make(tmp_path_factory.mktemp("wide132"), 132, False)


@pytest.fixture(scope="module")
def bytes16(tmp_path_factory):      # 8-bit descriptors, integer queries: hi planes, the streaming kernel, int8
    return make(tmp_path_factory.mktemp("bytes16"), 16, True)


@contextlib.contextmanager
def environment(env):
    with pytest.MonkeyPatch.context() as mp:
        for name, value in env.items():
            mp.setenv(name, value)
        yield


def topk(fx, k, n_probe, window=None):
    """all 48 queries against the oracle's first k (inside the window); the expectation is shared between the settings"""
    key = (window, k, n_probe)
    if key not in fx.want:
        fx.want[key] = fx.expected(window or EVERYTHING, 48, k, n_probe)
    De, Ie, cnt = fx.want[key]
    Dg, Ig = fx.gpu.search_sync(fx.Q, k, n_probe, filter=fx.filter(window) if window else None)
    bad = np.nonzero((Ig != Ie).any(axis=1) | (bits(Dg) != bits(De)).any(axis=1))[0]
    assert bad.size == 0, (f"window {window} k {k} n_probe {n_probe}: {bad.size} queries differ, first {bad[0]}: "
                           f"gpu {Ig[bad[0]][:12]} {Dg[bad[0]][:12]} expected {Ie[bad[0]][:12]} {De[bad[0]][:12]}")
    assert ((Ig >= 0).sum(axis=1) == cnt).all()
    return Ie


def lists_of(fx, I):
    """how many of the ids come from each of the three lists"""
    return np.bincount(fx.label[(I[I >= 0] - 1_000_003) // 7], minlength=3)


def topk_sweep(fx):
    for k, p in TOPK:
        Ie = topk(fx, k, p)
        if (k, p) == (100, 3):      # a circumcentre query's first 100 come from all three lists: past the cached group records
            assert max(lists_of(fx, Ie[q]).min() for q in range(24, 48)) > 0
    return fx.gpu.last_stats()


def radius_sweep(fx, cases, window=EVERYTHING):
    """cases: (batch, radius2, nq, n_probe); the expectation is shared between the settings"""
    for part, r, nq, p in cases:
        key = (part.rows.start, float(r), nq, p, window)
        if key not in fx.want:
            fx.want[key] = expected(part, r, nq, p, window)
        check(part, r, nq, p, window=window, want=fx.want[key])
    return fx.want[key]


def median_radii(fx):
    """the circumcentre batch at its median 10th, 100th and 1000th neighbour, three lists; and one list (group records
    within the cache: the long segments alone)"""
    centre = Part(fx, CENTRE)
    cases = [(centre, median_radius(centre, 3, kth), 24, 3) for kth in (10, 100, 1000)]
    lims, _, Ie, _ = expected(centre, cases[-1][1], 24, 3)
    per_list = [lists_of(fx, Ie[int(lims[q]):int(lims[q + 1])]).min() for q in range(24)]
    assert max(per_list) >= 200, per_list      # some query has 200 hits and more in every one of the three lists
    return centre, cases + [(centre, median_radius(centre, 1, 100), 24, 1)]


def everything(centre):
    """radius inf on 4 queries, three lists: 402 145 hits each, rows of 2^19 keys, every sub-block through the pick queue"""
    return [(centre, INF, 4, 3)]


# --------------------------------------------------------------------------------------------------------------
# top-k
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,modes", [({}, (2, 4, 5, 6)), ({"VI_FILTER_BF16": "0"}, (1,)), ({"VI_FILTER_HI_ONLY": "0"}, (2, 5)),
                                       ({"VI_FILTER_GQ": "32"}, (2, 4, 5, 6)), ({"VI_RANK_APPROX": "0"}, (2, 5)),
                                       ({"VI_RANK_APPROX": "1"}, (4, 6)), ({"VI_RANK_APPROX": "2"}, (4, 6)),
                                       ({"VI_FILTER": "0"}, (0,)), ({"VI_FORCE_GENERIC": "1"}, (0,))],
                         ids=lambda v: ("-".join(f"{a}={b}" for a, b in v.items()) or "default") if isinstance(v, dict) else None)
def test_top_k_real_valued(real8, env, modes):
    """f32 MFMA, bf16 x 3, hi planes of real-valued lists with and without the queries' lo plane, groups of 32 — and the
    exact-order VALU engine and the sort-everything engine, which share the segmentation rule"""
    with environment(env):
        st = topk_sweep(real8)
    assert st["rank_mode"] in modes, st
    assert st["group_queries"] == 32 or "VI_FILTER_GQ" not in env, st


@pytest.mark.parametrize("env,int8", [({}, 0), ({"VI_RANK_STREAM": "1", "VI_RANK_I8": "1"}, 1), ({"VI_RANK_STREAM": "1", "VI_RANK_I8": "0"}, 0),
                                      ({"VI_RANK_STREAM": "0"}, 0)],
                         ids=lambda v: ("-".join(f"{a}={b}" for a, b in v.items()) or "default") if isinstance(v, dict) else None)
def test_top_k_bytes(bytes16, env, int8):
    """hi planes of bf16-exact lists on the block-synchronous kernel (D = 16 streams only when told to), the streaming
    kernel with bf16 and with int8 products"""
    with environment(env):
        st = topk_sweep(bytes16)
    assert st["rank_mode"] == 3 and st["rank_int8"] == int8, st


def test_top_k_bytes_in_groups_of_256(bytes16):
    """groups of 256 are formed once the handle has seen a batch of this shape with bf16-exact queries: the second sweep"""
    with environment({"VI_RANK_STREAM": "1", "VI_STREAM_GQ": "256"}):
        topk_sweep(bytes16)
        st = topk_sweep(bytes16)
    assert st["rank_mode"] == 3 and st["rank_int8"] == 1 and st["group_queries"] == 256, st


def test_top_k_wide(wide132):
    st = topk_sweep(wide132)
    assert st["rank_mode"] == 2, st


@pytest.mark.parametrize("which", ["real8", "bytes16"])
def test_top_k_with_a_timestamp_window(which, request):
    fx = request.getfixturevalue(which)
    for window in (TENTH, ONLY_NOW, NOTHING):
        for k, p in [(10, 3), (100, 3)]:
            Ie = topk(fx, k, p, window)
            assert (Ie[:, 0] >= 0).all() != (window == NOTHING)
    assert fx.gpu.last_stats()["rank_mode"] >= 1


# --------------------------------------------------------------------------------------------------------------
# radius search
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{}, {"VI_FILTER_BF16": "0"}, {"VI_FILTER_GQ": "32"}, {"VI_FORCE_GENERIC": "1"}],
                         ids=lambda v: "-".join(f"{a}={b}" for a, b in v.items()) or "default")
def test_radii_real_valued(real8, env):
    centre, cases = median_radii(real8)
    near = Part(real8, NEAR)
    D, I, _ = centre.full(3)
    edge = D[5, 999]      # the boundary pair on one circumcentre query's 1000th neighbour: d == radius2 is inside
    below = np.nextafter(edge, np.float32(-1.0))
    assert edge > 0 and int((D[5] <= edge).sum()) >= 1000 > int((D[5] <= below).sum())
    cases = cases + [(centre, 0.0, 24, 3), (centre, float(edge), 24, 3), (centre, float(below), 24, 3),
                     (near, 0.0, 24, 3), (near, median_radius(near, 3, 10), 24, 3), (near, median_radius(near, 1, 10), 24, 1)]
    with environment(env):
        radius_sweep(real8, cases)
        lims = radius_sweep(real8, everything(centre))[0]
        st = real8.gpu.last_stats()
    assert int(lims[-1]) == 4 * N
    assert (st["rank_mode"] == 0) == ("VI_FORCE_GENERIC" in env) and (st["rank_mode"] == 1) == ("VI_FILTER_BF16" in env), st
    assert st["group_queries"] == 32 or "VI_FILTER_GQ" not in env, st


@pytest.mark.parametrize("rank_i8", ["1", "0"])
def test_radii_bytes(bytes16, rank_i8):
    centre, cases = median_radii(bytes16)
    with environment({"VI_RANK_STREAM": "1", "VI_RANK_I8": rank_i8}):
        radius_sweep(bytes16, cases)
        lims = radius_sweep(bytes16, everything(centre))[0]
        st = bytes16.gpu.last_stats()
    assert int(lims[-1]) == 4 * N
    assert st["rank_mode"] == 3 and st["rank_int8"] == int(rank_i8), st


def test_radii_wide(wide132):
    centre, cases = median_radii(wide132)
    radius_sweep(wide132, cases)
    lims = radius_sweep(wide132, everything(centre))[0]
    assert int(lims[-1]) == 4 * N
    assert wide132.gpu.last_stats()["rank_mode"] == 2


@pytest.mark.parametrize("which", ["real8", "bytes16", "wide132"])
def test_radius_with_a_timestamp_window(which, request):
    fx = request.getfixturevalue(which)
    centre, cases = median_radii(fx)
    radius_sweep(fx, cases[3:], window=TENTH)      # one list: the long segments alone
    lims = radius_sweep(fx, cases[2:3], window=TENTH)[0]      # the 1000th-neighbour radius on three lists
    plain = expected(centre, cases[2][1], 24, 3)[0]
    assert 0 < int(lims[-1]) < int(plain[-1])      # the window does thin the result
    assert fx.gpu.last_stats()["rank_mode"] >= 1
