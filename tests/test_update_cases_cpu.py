"""CPU: the inputs of tests/update_cases.py do what they claim, shown with the oracle and numpy alone (no library).

These are the preconditions of tests/test_kmeans_update_gpu.py: without them a GPU test could pass for the wrong reason
(no cluster large enough to reach segment_big_kernel, sums that do not depend on the order of the adds, a hierarchy
without a large or an empty group)."""
import numpy as np
import pytest

import oracle_lib as O
import update_cases as U

BIG_NAMES = [n for n in U.CASES if "big" in n]


def same(a, b):
    """bit equality, any NaN equal to any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def test_every_case_is_well_formed_and_documented():
    for name, (_, doc) in U.CASES.items():
        X, lab, k = U.make(name)
        assert doc and X.dtype == np.float32 and X.ndim == 2 and X.flags.c_contiguous, name
        assert lab.dtype == np.uint32 and lab.shape == (X.shape[0],) and lab.size and int(lab.max()) < k, name
        X2, lab2, _ = U.make(name)  # deterministic
        assert (X.view(np.uint32) == X2.view(np.uint32)).all() and (lab == lab2).all(), name


@pytest.mark.parametrize("name", BIG_NAMES)
def test_big_cases_hold_a_cluster_above_the_threshold(name):
    X, lab, k = U.make(name)
    assert np.bincount(lab, minlength=k).max() > U.BIG


def test_cases_named_in_the_plan_exist():
    assert U.BIG == 2048 and U.CHUNK_FLOATS == 16384 and U.RADIX_TILE == 4096
    for d in (16, 20, 24, 32, 96, 100, 128, 500, 512):
        H = 16384 // d
        X, lab, k = U.make(f"big_geometry_d{d}")
        assert X.shape[1] == d
        c = np.bincount(lab, minlength=k).tolist()
        assert c[:9] == [2049, H, H - 1, H + 1, 2 * H + 1, 3 * H, 3 * H - 1, 3 * H + 1, 6 * H + 5] and c[9] >= 60000
        # what segment_big_kernel itself sees at this d: clusters that end on a chunk edge, one row past it and one row
        # short of it, each for every number of chunks mod 3 (three chunks per trip of its loop)
        big = [m for m in c if m > U.BIG]
        for rem in (0, 1, H - 1):
            assert {(-(-m // H)) % 3 for m in big if m % H == rem} == {0, 1, 2}, (d, rem)
    for d in (20, 24, 100, 500):
        assert 16384 % d != 0  # a partial row is staged
    assert 16384 // 512 == 32
    X, lab, k = U.make("big_boundary")
    assert np.bincount(lab, minlength=k).tolist() == [2047, 2048, 2049, 2050]
    X, lab, k = U.make("big_many")
    c = np.bincount(lab, minlength=k)
    assert X.shape[1] == 16 and (c > U.BIG).sum() > 1024 and lab.size > 256 * U.RADIX_TILE
    for name in ("big_fallback_residues_d8", "big_fallback_unaligned_d32"):
        X, lab, k = U.make(name)
        c = np.bincount(lab, minlength=k)
        assert (c > U.BIG).all() and sorted(set((c % 32).tolist())) == list(range(32))
    for d in (8, 18, 516, 1024):  # no split: d < 16, d % 4 != 0 or d > 512
        assert d < 16 or d % 4 or d > 512
    assert set(U.UNALIGNED) == {"big_fallback_unaligned_d32"}
    for name, n, k, empty in (("big_one_cluster_k1", 300000, 1, 0), ("big_one_cluster_k7", 300000, 7, 6)):
        X, lab, kk = U.make(name)
        c = np.bincount(lab, minlength=kk)
        assert kk == k and lab.size == n and c.max() == n and (c == 0).sum() == empty
    X, lab, k = U.make("big_layout_sorted")
    assert (np.diff(lab.astype(np.int64)) >= 0).all()
    X, lab, k = U.make("big_layout_reverse")
    assert (np.diff(lab.astype(np.int64)) <= 0).all()
    X, lab, k = U.make("big_layout_round_robin")
    assert (lab == np.arange(lab.size) % k).all()
    X, lab, k = U.make("big_layout_ends")
    assert set(np.unique(lab).tolist()) == {0, k - 1}
    assert [U.make(f"tile_n{n}")[1].size for n in U.TILE_NS] == [1, 63, 64, 65, 4095, 4096, 4097, 8193]
    passes = {"radix_k256": 1, "radix_k257": 2, "radix_k65536": 2, "radix_k65537": 3, "radix_k16777217": 4}
    for name, p in passes.items():
        X, lab, k = U.make(name)
        assert U.radix_passes(k) == p, name
        assert {0, 1, k - 2, k - 1} <= set(lab.tolist())
        assert int(lab.max()) >> (8 * (p - 1)) != 0 or k == 256  # the top digit is not all zero
        assert np.unique(lab, return_counts=True)[1].max() >= 16   # repeated members: their order is observable
    X, lab, k = U.make("radix_k16777217")
    assert k == 2 ** 24 + 1 and X.shape == (lab.size, 1) and 2000 <= lab.size <= 10000
    assert (lab == 0).sum() >= 16 and (lab == 2 ** 24).sum() >= 16   # labels that differ in the top byte only
    assert len(set((lab[lab < 2 ** 24] >> 16).tolist())) > 200       # spread over the whole range


def test_data_kinds_hold_what_they_name():
    kinds = {}
    for kind in U.KINDS:
        X, lab, k = U.make(f"big_kind_{kind}")
        assert np.bincount(lab, minlength=k).tolist() == U.KIND_COUNTS
        kinds[kind] = X
    assert abs(float(kinds["offset"].mean()) - 100.0) < 1.0
    norms = np.abs(kinds["scaled"]).max(axis=1)
    assert norms.max() / norms.min() > 1e5
    Xi = kinds["ints"]
    assert (Xi == np.round(Xi)).all() and np.abs(Xi).max() <= 8
    nz = kinds["negzero"].view(np.uint32) == 0x80000000
    assert nz.all(axis=1).sum() > 1000 and not nz.all()
    Xs = kinds["special"]
    sub = (Xs != 0) & (np.abs(Xs) < np.finfo(np.float32).tiny)
    assert np.isposinf(Xs).any() and np.isneginf(Xs).any() and np.isnan(Xs).any() and sub.sum() >= 8
    # the -0.0 cluster and the single -0.0 member sum to +0.0
    X, lab, k = U.make("big_kind_negzero")
    S, _ = O.cluster_sums(X, lab, k)
    assert (S[[U.NEGZERO_CLUSTER, U.NEGZERO_SINGLE]].view(np.uint32) == 0).all()
    assert (X[lab == U.NEGZERO_CLUSTER].view(np.uint32) == 0x80000000).all()


@pytest.mark.parametrize("name", [n for n in BIG_NAMES if U.kind_of(n) not in U.ORDER_INSENSITIVE_KINDS])
def test_big_cluster_sums_depend_on_member_order(name):
    """the argument that a GPU sum equal to the oracle's bit for bit was added in the oracle's order: for every big
    cluster, reversing its members and exchanging the two halves of its member list each change the bits of the oracle's
    sum in at least one column (so a reordered chunk cannot go unseen)"""
    X, lab, k = U.make(name)
    S0, counts = O.cluster_sums(X, lab, k)
    big = np.flatnonzero(counts > U.BIG)
    assert big.size
    order = np.argsort(lab, kind="stable")
    off = np.r_[0, np.cumsum(counts.astype(np.int64))]
    Xr, Xh = X.copy(), X.copy()
    for c in big:
        m = order[off[c]:off[c + 1]]
        Xr[m] = X[m[::-1]]
        Xh[m] = X[np.r_[m[m.size // 2:], m[:m.size // 2]]]
    for what, Xp in (("reversed", Xr), ("halves exchanged", Xh)):
        S1, _ = O.cluster_sums(Xp, lab, k)
        changed = (~same(S0[big], S1[big])).any(axis=1)
        assert changed.all(), (name, what, big[~changed].tolist())
        small = np.setdiff1d(np.arange(k), big)
        assert same(S0[small], S1[small]).all()


def test_integer_sums_do_not_depend_on_order():
    """... which is why the integer kind never stands alone: it checks membership only"""
    X, lab, k = U.make("big_kind_ints")
    S0, _ = O.cluster_sums(X, lab, k)
    p = np.random.default_rng(0).permutation(lab.size)
    S1, _ = O.cluster_sums(X[p], lab[p], k)
    assert (S0.view(np.uint32) == S1.view(np.uint32)).all()


@pytest.mark.parametrize("name", ["big_boundary", "big_kind_special", "big_kind_negzero", "big_kind_scaled", "big_layout_random",
                                  "big_geometry_d100", "big_many", "radix_k65537", "tile_n4097"])
def test_oracle_sums_equal_an_unbuffered_numpy_accumulation(name):
    """np.add.at adds the rows one by one in index order in f32: the same chains, written without the oracle"""
    X, lab, k = U.make(name)
    S, counts = O.cluster_sums(X, lab, k)
    ref = np.zeros((k, X.shape[1]), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        np.add.at(ref, lab.astype(np.int64), X)
    assert same(S, ref).all()
    assert (counts == np.bincount(lab, minlength=k)).all()


def test_f64_reference_matches_a_plain_loop():
    X, lab, k = U.make("big_kind_scaled")
    ids, S, A, m = U.f64_reference(X, lab, k)
    assert ids.tolist() == [c for c in range(k) if U.KIND_COUNTS[c]] and m.tolist() == [c for c in U.KIND_COUNTS if c]
    for i, c in enumerate(ids):
        rows = X[lab == c].astype(np.float64)
        assert np.allclose(S[i], rows.sum(axis=0), rtol=1e-12, atol=0) or np.allclose(S[i], rows.sum(axis=0), rtol=0, atol=1e-9)
        assert np.allclose(A[i], np.abs(rows).sum(axis=0), rtol=1e-12)


def test_hierarchy_case_has_a_big_group_and_empty_groups():
    X, Cn = U.hierarchy_case()
    assert Cn.shape == (6000, 16) and O.lib().orc_meta_k(6000) == U.HIER_META_K == 77
    row, n_copies = np.unique(Cn.view(np.uint32), axis=0, return_counts=True)
    assert n_copies.max() == U.HIER_COPIES == 2600 and (n_copies > 1).sum() == 1   # exact copies of one row, no others
    dup = row[n_copies.argmax()].view(np.float32)
    on = (X.view(np.uint32) == dup.view(np.uint32)).all(axis=1)
    near = ~on & (np.linalg.norm(X - dup, axis=1) < 0.5)
    assert 4500 <= X.shape[0] <= 5500 and on.sum() >= 100 and near.sum() >= 500
    for seed in U.HIER_SEEDS:
        meta, c2m = O.build_centroid_hierarchy(Cn, U.HIER_META_K, seed * 17 + 42)
        sizes = np.bincount(c2m.astype(np.int64), minlength=U.HIER_META_K)
        assert sizes.max() > U.BIG and (sizes == 0).sum() >= 1, (seed, sizes.max())


@pytest.mark.parametrize("name", U.LLOYD_CASES)
def test_lloyd_cases_keep_clusters_above_the_threshold(name):
    X, k = U.lloyd_case(name)
    assert X.shape[0] >= 50000 and X.shape[1] in (32, 100)
    rc, Cn, lab, it = O.kmeans_parallel(X, k, 5, seed=42)
    assert rc == 0 and np.bincount(lab.astype(np.int64), minlength=k).max() > U.BIG
    if name == "few_distinct":
        assert np.unique(X.view(np.uint32), axis=0).shape[0] < k
        assert (np.bincount(lab.astype(np.int64), minlength=k) == 0).any()
