"""GPU parity of the Lloyd update pass: vi_kmeans_partial_sums_device / vi_kmeans_finish_update_device through the C ABI
against the CPU oracle, at the shapes where the two summing kernels and the radix grouping change what they do.

Every case (tests/update_cases.py, its preconditions proven in tests/test_update_cases_cpu.py) makes ONE call of
vi_kmeans_partial_sums_device and checks
  * the sums against O.cluster_sums as uint32 bits (any NaN equal to any NaN: the payload and sign of a NaN sum are not
    part of the reference's contract — x86 gives 0xFFC00000 for inf + -inf — every other value, +-inf, +-0 and subnormals
    included, by bits) and the counts exactly;
  * vi_kmeans_finish_update_device on those sums against O.update_centroids bit for bit: zero rows for empty clusters,
    the list of empty clusters, and the RMS movement against the oracle's sequential formula restated in np.float32;
  * without the oracle: every sum lies within gamma * sum|x| of the float64 sum of the same members, gamma =
    (m - 1) u / (1 - (m - 1) u), u = 2^-24, m members (the bound of a sequential sum, Higham 2002 eq. 4.4), plus
    m * 2^-52 * sum|x| for the float64 evaluation itself; non-finite columns by class.
A cluster's f32 chain depends on the order of its members (test_update_cases_cpu.py: reversing it or exchanging its
halves changes the bits of every big cluster's sum), so equal bits mean the same members in the same order.

Whole loops on top: Lloyd with clusters far above 2048 members (kSegMean in segment_big_kernel, the zero row and the
re-seed of an empty cluster) and the centroid hierarchy with a 2600-member group and empty groups (kSegMeanKeep)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import update_cases as U
import vector_indexer_py as vip
from hiprt import Hip
from vector_indexer_py import _native as N

pytestmark = pytest.mark.gpu

POISON_F32, POISON_U32 = 0x7FC0DEAD, 0xDEADBEEF  # what the outputs hold before the call: an unwritten entry shows


def same(a, b):
    """bit equality, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def first_diff(a, b):
    bad = np.argwhere(~same(a, b))
    return f"{bad.shape[0]} entries differ, first at {bad[0].tolist()}" if bad.size else ""


def delta_restated(Cn, Cp):
    """centroid_delta of the oracle (sequential over the columns of a cluster, then over the clusters), in np.float32"""
    k, d = Cn.shape
    local = np.zeros(k, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(d):
            diff = Cn[:, j] - Cp[:, j]
            local = local + diff * diff
        dsq = np.cumsum(local, dtype=np.float32)[-1]  # (a sequential f32 accumulation; 0.0 + local[0] = local[0] >= +0)
        return np.sqrt(np.float32(dsq) / np.float32(k * d))


def partial_sums(hip, X, lab, k, unaligned=False):
    n, d = X.shape
    if unaligned:  # one float past a 16-byte aligned address
        Xd = hip.alloc(X.nbytes + 16) + 4
        hip.upload_to(Xd, X)
    else:
        Xd = hip.upload(X)
    assert (Xd % 16 == 4) if unaligned else (Xd % 16 == 0)
    Ld = hip.upload(lab)
    Sd = hip.upload(np.full(k * d, POISON_F32, dtype=np.uint32))
    Nd = hip.upload(np.full(k, POISON_U32, dtype=np.uint32))
    N.check(N.lib().vi_kmeans_partial_sums_device(0, Xd, n, d, Ld, k, Sd, Nd))
    return Sd, Nd, hip.download(Sd, (k, d), np.float32), hip.download(Nd, (k,), np.uint32)


def check_update(name, unaligned=False):
    X, lab, k = U.make(name)
    n, d = X.shape
    hip = Hip()
    try:
        Sd, Nd, S, cnt = partial_sums(hip, X, lab, k, unaligned)
        # -- against the oracle, bit for bit
        So, co = O.cluster_sums(X, lab, k)
        assert (cnt == co).all(), name
        assert same(S, So).all(), (name, first_diff(S, So))
        # -- the finishing step on the GPU's own sums
        Cp = np.random.default_rng(k + d).standard_normal((k, d)).astype(np.float32)
        Cpd, Cnd = hip.upload(Cp), hip.upload(np.full(k * d, POISON_F32, dtype=np.uint32))
        delta, ne = C.c_float(-1.0), C.c_uint64(1 << 40)
        empties = np.full(k, POISON_U32, dtype=np.uint32)
        N.check(N.lib().vi_kmeans_finish_update_device(0, Sd, Nd, k, d, Cpd, Cnd, C.byref(delta), empties.ctypes.data,
                                                       C.byref(ne)))
        Cg = hip.download(Cnd, (k, d), np.float32)
        Co, co2 = O.update_centroids(X, lab, k)
        assert (co2 == co).all()
        assert same(Cg, Co).all(), (name, first_diff(Cg, Co))
        empty = np.flatnonzero(co == 0)
        assert (Cg[empty].view(np.uint32) == 0).all(), name                      # rows of +0.0
        assert ne.value == empty.size and (empties[:empty.size] == empty).all(), name
        assert (empties[empty.size:] == POISON_U32).all(), name
        exp_delta = delta_restated(Co, Cp)
        print(f"{name}: n={n} d={d} k={k} largest={int(co.max())} empty={empty.size} delta={delta.value!r}")
        assert same(np.float32(delta.value), exp_delta).all(), (name, delta.value, exp_delta)
        # -- without the oracle: the sequential-sum bound against float64
        ids, S64, A, m = U.f64_reference(X, lab, k)
        rest = np.ones(k, dtype=bool)
        rest[ids] = False
        assert (S[rest].view(np.uint32) == 0).all() and (cnt[ids] == m).all() and (cnt[rest] == 0).all(), name
        u = 2.0 ** -24
        gamma = ((m - 1) * u / (1.0 - (m - 1) * u))[:, None]
        Sg = S[ids].astype(np.float64)
        fin = np.isfinite(A)
        with np.errstate(invalid="ignore"):
            err, bound = np.abs(Sg - S64), gamma * A + (m[:, None] * 2.0 ** -52) * A
        assert (err[fin] <= bound[fin]).all(), (name, float((err[fin] / np.maximum(bound[fin], 1e-300)).max()))
        assert (np.isnan(Sg[~fin]) == np.isnan(S64[~fin])).all(), name          # NaN, or inf and -inf met: NaN
        inf = ~fin & ~np.isnan(S64)
        assert (Sg[inf] == S64[inf]).all(), name                                  # +inf or -inf alone
    finally:
        hip.close()


@pytest.mark.parametrize("d", U.GEOMETRY_DIMS)
def test_chunk_geometry_of_the_big_kernel(d):
    """H = 16384 // d rows per chunk, three chunks per trip: member counts of 2049, H, H+-1, 2H+1, 3H, 3H+-1, 6H+5 and
    one chain of 60013 (d = 20, 24, 100, 500 leave a partial row in the chunk; H = 32 at d = 512).  From d = 24 on most
    of these are <= 2048 and test the hand-over to segment_kernel; what the big kernel sees at every d are the counts
    jH, jH+-1 at four multiples above 2048: an end on a chunk edge, one row past it and one row short of it for every
    number of chunks mod 3 (update_cases.geometry_counts, asserted in test_update_cases_cpu.py)"""
    check_update(f"big_geometry_d{d}")


def test_the_2048_boundary():
    check_update("big_boundary")


def test_more_big_clusters_than_workgroups():
    """1100 big clusters on a grid of 1024 (the stride loop); 2.3 M points = 559 radix tiles (the tile-count scan runs its
    256-tile step three times)"""
    check_update("big_many")


@pytest.mark.parametrize("name", ["big_fallback_residues_d8", "big_fallback_d18", "big_fallback_d516", "big_fallback_d1024"])
def test_long_chains_where_the_split_must_not_happen(name):
    check_update(name)


def test_long_chains_on_points_aligned_to_four_bytes_only():
    assert "big_fallback_unaligned_d32" in U.UNALIGNED
    check_update("big_fallback_unaligned_d32", unaligned=True)
    check_update("big_fallback_unaligned_d32")   # the same input, aligned: through the big kernel


@pytest.mark.parametrize("name", ["big_layout_sorted", "big_layout_reverse", "big_layout_round_robin", "big_layout_random",
                                  "big_layout_ends", "big_one_cluster_k1", "big_one_cluster_k7"]
                         + [f"tile_n{n}" for n in U.TILE_NS])
def test_label_layouts(name):
    check_update(name)


@pytest.mark.parametrize("name,k,passes", [("radix_k256", 256, 1), ("radix_k257", 257, 2), ("radix_k65536", 65536, 2),
                                           ("radix_k65537", 65537, 3), ("radix_k16777217", 2 ** 24 + 1, 4)])
def test_radix_pass_counts(name, k, passes):
    """1 to 4 passes of 8 bits by the bits of k - 1 (k = 2^24 + 1: d = 1, 64 MB of sums)"""
    assert U.radix_passes(k) == passes
    check_update(name)


@pytest.mark.parametrize("kind", U.KINDS)
def test_data_kinds(kind):
    check_update(f"big_kind_{kind}")


def test_argument_errors_touch_no_memory():
    lib = N.lib()
    hip = Hip()
    try:
        n, d, k = 5000, 16, 3
        X = np.ones((n, d), dtype=np.float32)
        lab = (np.arange(n) % k).astype(np.uint32)
        lab[n - 1] = k
        Xd, Ld = hip.upload(X), hip.upload(lab)
        Sd, Nd = hip.upload(np.full(k * d, POISON_F32, dtype=np.uint32)), hip.upload(np.full(k, POISON_U32, dtype=np.uint32))

        def untouched():
            return (hip.download(Sd, (k * d,), np.uint32) == POISON_F32).all() and \
                (hip.download(Nd, (k,), np.uint32) == POISON_U32).all()
        # a label equal to k
        assert lib.vi_kmeans_partial_sums_device(0, Xd, n, d, Ld, k, Sd, Nd) == N.VI_ERR_INVALID_INPUT
        assert b"a label is not below k" in lib.vi_last_error() and untouched()
        assert lib.vi_kmeans_partial_sums_device(0, Xd, n, d, Ld, k + 1, hip.alloc((k + 1) * d * 4), hip.alloc((k + 1) * 4)) == N.VI_OK
        # n = 2^32 - 1: refused by the size check before a pointer is followed (the buffers hold 5000 rows)
        assert lib.vi_kmeans_partial_sums_device(0, Xd, 2 ** 32 - 1, d, Ld, k, Sd, Nd) == N.VI_ERR_INVALID_INPUT
        assert b"2^32 - 2 points" in lib.vi_last_error() and untouched()
        # null outputs, null inputs with n > 0, d = 0, k = 0
        for args in ((Xd, n, d, Ld, k, None, Nd), (Xd, n, d, Ld, k, Sd, None), (None, n, d, Ld, k, Sd, Nd),
                     (Xd, n, d, None, k, Sd, Nd), (Xd, n, 0, Ld, k, Sd, Nd), (Xd, n, d, Ld, 0, Sd, Nd)):
            assert lib.vi_kmeans_partial_sums_device(0, *args) == N.VI_ERR_INVALID_INPUT, args
            assert b"bad arguments" in lib.vi_last_error() and untouched()
        Cd = hip.alloc(k * d * 4)
        for args in ((None, Nd, k, d, Cd, Cd), (Sd, None, k, d, Cd, Cd), (Sd, Nd, k, d, None, Cd), (Sd, Nd, k, d, Cd, None),
                     (Sd, Nd, 0, d, Cd, Cd), (Sd, Nd, k, 0, Cd, Cd)):
            assert lib.vi_kmeans_finish_update_device(0, *args, None, None, None) == N.VI_ERR_INVALID_INPUT, args
        # n = 0 is a rank without points: zero sums and counts
        assert lib.vi_kmeans_partial_sums_device(0, None, 0, d, None, k, Sd, Nd) == N.VI_OK
        assert (hip.download(Sd, (k * d,), np.uint32) == 0).all() and (hip.download(Nd, (k,), np.uint32) == 0).all()
    finally:
        hip.close()


@pytest.mark.parametrize("name", U.LLOYD_CASES)
def test_lloyd_with_big_clusters(name):
    """60 000 points in 4..6 clusters: every update runs kSegMean in segment_big_kernel; 'few_distinct' has fewer
    distinct points than k, so clusters run empty: the zero row, then the re-seed from the replayed stream"""
    X, k = U.lloyd_case(name)
    for max_iters in (1, 5):
        rc, Co, lo, ito = O.kmeans_parallel(X, k, max_iters, seed=42)
        Cg, lg, itg = vip.kmeans_parallel(X, k, max_iters, seed=42)
        assert rc == 0 and itg == ito
        assert np.bincount(lo.astype(np.int64), minlength=k).max() > U.BIG
        assert (lg == lo).all(), int((lg != lo).sum())
        assert (Cg.view(np.uint32) == Co.view(np.uint32)).all(), first_diff(Cg, Co)


@pytest.mark.parametrize("seed", U.HIER_SEEDS)
def test_hierarchy_with_a_big_group_and_empty_groups(seed):
    """6000 centroids of which 2600 are copies of one row: build_centroid_hierarchy gets a group above 2048 members
    (kSegMeanKeep in segment_big_kernel) and empty groups, which keep their row.  What this checks is that the mode runs
    in the big kernel and that a kept row stays: labels only, and the mean of 2600 equal rows hardly depends on their
    order.  The order of the adds in the big kernel is checked by the kSegSums cases above; the modes differ in
    segment_store alone."""
    X, Cn = U.hierarchy_case()
    sizes = np.bincount(O.build_centroid_hierarchy(Cn, U.HIER_META_K, seed * 17 + 42)[1].astype(np.int64), minlength=U.HIER_META_K)
    assert sizes.max() > U.BIG and (sizes == 0).any()
    lab_o = O.assign(X, Cn, seed=seed, mode="hier")
    lab_g = vip.assign(X, Cn, seed=seed, mode=vip.VI_ASSIGN_REFERENCE)
    assert (lab_g == lab_o).all(), int((lab_g != lab_o).sum())
