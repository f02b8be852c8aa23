"""GPU: compound filters — a | b, ~a, a - b, id ranges, masks in list order, and vi_indexer_filter_compose (one launch for
the AND / OR of up to eight terms, optionally written over an existing filter) — on all three engines, the radius search,
retain and the per-rank merge.

Expected results come from the untouched oracle (filter_compose_cases.py): a per-record boolean admit[row], computed in
numpy from ids and timestamps, masks OracleIndex.search_batch(Q, N, p), the full stable-sorted candidate sequence; the first
k survivors are the answer.  Ids, distance bits, counts and padding must match exactly; num_allowed must equal admit.sum()."""
import ctypes as C

import numpy as np
import pytest

import filter_compose_cases as F
import vector_indexer_py as vip
from filter_compose_cases import EVERYTHING, HALF, MID, NOW, SHAPES, U64_MAX, bits, u64
from vector_indexer_py import _native as N
from vector_indexer_py.harness import FaissStyleAdapter

pytestmark = pytest.mark.gpu

Term = vip.Term


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return F.make_base(tmp_path_factory.mktemp("base"))


@pytest.fixture(scope="module")
def valu(tmp_path_factory):
    return F.make_valu(tmp_path_factory.mktemp("valu"))


@pytest.fixture(scope="module")
def bytes8(tmp_path_factory):
    return F.make_bytes8(tmp_path_factory.mktemp("bytes"))


@pytest.fixture(scope="module")
def case(base):
    return F.AndCase(base)


def invalid(fn):
    with pytest.raises(vip.ViError) as e:
        fn()
    assert e.value.kind == "InvalidInput" and str(e.value)


# ---- 1. union ----
def test_union_of_two_id_sets_and_of_a_window_with_an_id_set(base):
    A, B = base.sets["tenth"], base.sets["n65"]
    fa, fb = base.gpu.filter_ids(A), base.gpu.filter_ids(B)
    both = fa | fb
    assert isinstance(both, vip.ComposedFilter)
    F.check_all(base, both, F.in_set(base, "tenth") | F.in_set(base, "n65"), what="ids | ids")
    F.same_results(base, both, base.gpu.filter_ids(np.concatenate([A, B])))
    win = base.gpu.filter_timestamps(*HALF)
    F.check_all(base, win | fa, F.in_window(base, HALF) | F.in_set(base, "tenth"), what="window | ids")
    F.same_results(base, win | fa, fa | win, shapes=[MID])


# ---- 2. complement ----
def test_complement(base):
    S = base.sets["tenth"]
    fs, deny = base.gpu.filter_ids(S), base.gpu.filter_ids(S, exclude=True)
    comp = ~fs
    F.check_all(base, comp, ~F.in_set(base, "tenth"), what="~ids")
    assert comp.num_allowed == deny.num_allowed
    F.same_results(base, comp, deny)
    win = base.gpu.filter_timestamps(*HALF)
    F.check_all(base, ~win, ~F.in_window(base, HALF), what="~window")
    F.nothing_found(base, ~base.gpu.filter_timestamps(*EVERYTHING))
    everything = ~base.gpu.filter_ids([])
    assert everything.num_allowed == base.n          # no pad slot is admitted
    F.same_results(base, everything, None, shapes=SHAPES + [(300, 200, 8)])
    for a in (fs, deny, win, comp, base.gpu.filter_ids(base.sets["odd"])):
        assert a.num_allowed + (~a).num_allowed == base.gpu.num_vectors


# ---- 3. difference and De Morgan ----
def test_difference_and_de_morgan(base):
    a, b = base.gpu.filter_ids(base.sets["half"]), base.gpu.filter_timestamps(*HALF)
    ra, rb = F.in_set(base, "half"), F.in_window(base, HALF)
    diff = a - b
    F.check_all(base, diff, ra & ~rb, what="a - b")
    chained = a & ~b
    assert diff.num_allowed == chained.num_allowed
    F.same_results(base, diff, chained)
    lhs, rhs = ~(a | b), ~a & ~b
    F.check_all(base, lhs, ~(ra | rb), what="~(a | b)")
    assert lhs.num_allowed == rhs.num_allowed
    F.same_results(base, lhs, rhs)


# ---- 4. id range ----
def test_id_range(base):
    s = np.sort(base.ext)
    j = int(np.nonzero(np.diff(s) > np.uint64(1))[0][100])        # s[j] + 1 .. s[j + 1] - 1 holds no stored id
    one = base.gpu.filter_id_range(int(s[j]), int(s[j + 1]) - 1)
    F.check_all(base, one, base.ext == s[j], what="one id")
    assert one.num_allowed == 1
    zero = base.gpu.filter_id_range(0, 0)
    F.check_all(base, zero, base.ext == np.uint64(0), what="[0, 0]")
    assert zero.num_allowed == 1
    everything = base.gpu.filter_id_range(0, U64_MAX)
    assert everything.num_allowed == base.n
    F.same_results(base, everything, None, shapes=SHAPES + [(300, 200, 8)])
    F.nothing_found(base, base.gpu.filter_id_range(int(s[j]) + 1, int(s[j + 1]) - 1))
    F.nothing_found(base, base.gpu.filter_id_range(int(s[-1]) + 1, U64_MAX), shapes=[MID])
    lo, hi = 2 << 40, (3 << 40) - 1                               # the fifth of the records whose bits 40.. hold 2
    wide = base.gpu.filter_id_range(lo, hi)
    assert 1000 < wide.num_allowed < 1400
    F.check_all(base, wide, F.in_range(base, lo, hi), what="a fifth")
    F.check_all(base, base.gpu.filter_id_range(int(s[1000]), int(s[4000])), F.in_range(base, s[1000], s[4000]), shapes=[MID])
    invalid(lambda: base.gpu.filter_id_range(5, 4))
    invalid(lambda: base.gpu.filter_compose([Term.timestamps(5, 4)]))


def test_id_range_on_an_index_that_stores_uint64_max(tmp_path):
    rng = np.random.default_rng(11)
    X = rng.standard_normal((200, 8)).astype(np.float32)
    ext = np.arange(200, dtype=np.uint64) * np.uint64(3) + np.uint64(1)
    ext[77] = U64_MAX
    ix = vip.build(X, str(tmp_path), ext_ids=ext, now_secs=NOW)
    top = ix.filter_id_range(U64_MAX, U64_MAX)
    assert top.num_allowed == 1 and (~top).num_allowed == 199 and ix.filter_id_range(0, U64_MAX).num_allowed == 200
    assert ix.filter_id_range(U64_MAX - 1, U64_MAX).num_allowed == 1 and ix.filter_id_range(0, U64_MAX - 1).num_allowed == 199
    D, I = ix.search_sync(X[77:78], 5, 10_000, filter=top)
    assert D[0, 0] == 0.0 and np.isinf(D[0, 1:]).all() and I[0, 0] == -1   # (the id as an i64; the distance shows the hit)
    D, I = ix.search_sync(X[77:78], 5, 10_000, filter=~top)
    assert D[0, 0] > 0.0 and (I[0] >= 0).all()
    assert ix.filter_compose([Term.ids([U64_MAX]), Term.id_range(U64_MAX, U64_MAX)]).num_allowed == 1


# ---- 5. mask ----
def test_masks_in_list_order(base):
    rows, where = F.list_rows(base)
    assert np.array_equal(np.sort(rows), np.arange(base.n))
    rng = np.random.default_rng(21)
    for ones in (63, 64, 65):
        admit = np.zeros(base.n, dtype=bool)
        admit[rng.choice(base.n, ones, replace=False)] = True
        F.check_all(base, base.gpu.filter_mask(admit[rows]), admit, what=f"{ones} ones")
    F.nothing_found(base, base.gpu.filter_mask(np.zeros(base.n, dtype=bool)))
    everything = base.gpu.filter_mask(np.ones(base.n, dtype=np.uint8))
    assert everything.num_allowed == base.n
    F.same_results(base, everything, None, shapes=SHAPES + [(300, 200, 8)])
    # the last record of every list: the ragged block's last live lane
    lists = (where >> np.uint64(32)).astype(np.int64)
    last = np.concatenate([lists[1:] != lists[:-1], [True]])
    assert last.sum() == base.nlists and ((where[last] & np.uint64(0xFFFFFFFF)) % np.uint64(64) != np.uint64(63)).any()
    admit = np.zeros(base.n, dtype=bool)
    admit[rows[last]] = True
    F.check_all(base, base.gpu.filter_mask(last), admit, what="last of every list")
    first = np.concatenate([[True], lists[1:] != lists[:-1]])
    admit = np.zeros(base.n, dtype=bool)
    admit[rows[first]] = True
    F.check_all(base, base.gpu.filter_mask(first), admit, shapes=[MID], what="first of every list")
    # any non-zero byte admits
    admit = rng.random(base.n) < 0.3
    m = np.where(admit[rows], np.where(np.arange(base.n) % 2 == 0, 0x80, 2), 0).astype(np.uint8)
    assert set(np.unique(m)) == {0, 2, 0x80}
    f_bytes = base.gpu.filter_mask(m)
    F.check_all(base, f_bytes, admit, what="bytes 0x80 and 2")
    invalid(lambda: base.gpu.filter_mask(np.ones(base.n - 1, dtype=np.uint8)))
    invalid(lambda: base.gpu.filter_mask(np.ones(base.n + 1, dtype=np.uint8)))
    invalid(lambda: base.gpu.filter_mask(np.zeros(0, dtype=np.uint8)))
    from hiprt import Hip
    hip = Hip()
    try:
        dev = hip.upload(m)
        f_dev = base.gpu.filter_mask_device(dev, m.size)
        assert f_dev.num_allowed == f_bytes.num_allowed
        F.check_all(base, f_dev, admit, shapes=[MID], what="device mask")
        F.same_results(base, f_dev, f_bytes)
        invalid(lambda: base.gpu.filter_mask_device(dev, m.size - 1))
        invalid(lambda: base.gpu.filter_mask_device(0, m.size))
        assert base.gpu.filter_compose([Term.mask_device(dev, m.size), ~Term.mask(m)]).num_allowed == 0
    finally:
        hip.close()


# ---- 6. compose ----
def test_compose_equals_the_chain_of_single_filters(base, case):
    terms = case.terms(vip)
    one = base.gpu.filter_compose(terms)
    assert isinstance(one, vip.ComposedFilter)
    F.check_all(base, one, case.admit_and, what="AND of four")
    w, a, nb, m = case.chain()
    chain = w & a & nb & m
    assert chain.num_allowed == one.num_allowed
    F.same_results(base, one, chain)
    any_of = base.gpu.filter_compose(terms, any=True)
    F.check_all(base, any_of, case.admit_or, what="OR of four")
    F.same_results(base, any_of, w | a | nb | m, shapes=[MID])
    # nesting: a filter as a term, negated
    nested = base.gpu.filter_compose([Term.filter(w), ~Term.filter(any_of)], any=True)
    F.check_all(base, nested, F.in_window(base, HALF) | ~case.admit_or, shapes=[MID], what="nested")


def test_compose_with_several_id_tables_and_a_negated_empty_set(base):
    ra, rb = F.in_set(base, "half"), F.in_set(base, "mostly_absent")
    two = base.gpu.filter_compose([Term.ids(base.sets["half"]), Term.ids(base.sets["mostly_absent"])])
    F.check_all(base, two, ra & rb, what="ids AND ids")
    two_or = base.gpu.filter_compose([Term.ids(base.sets["n63"]), Term.ids(base.sets["odd"]), Term.ids(base.sets["repeated"])], any=True)
    F.check_all(base, two_or, F.in_set(base, "n63") | F.in_set(base, "odd") | F.in_set(base, "repeated"), what="ids OR ids OR ids")
    everything = base.gpu.filter_compose([~Term.ids([])])
    assert everything.num_allowed == base.n
    F.same_results(base, everything, None)
    F.nothing_found(base, base.gpu.filter_compose([Term.ids([])]), shapes=[MID])
    F.check_all(base, base.gpu.filter_compose([~Term.ids([]), Term.ids(base.sets["tenth"])]), F.in_set(base, "tenth"), shapes=[MID])
    from hiprt import Hip
    hip = Hip()
    try:
        ids = np.concatenate([base.sets["tenth"], base.sets["tenth"][:100]])
        dev = hip.upload(ids)
        f = base.gpu.filter_compose([Term.ids_device(dev, ids.size), ~Term.ids(base.sets["half"])])
        F.check_all(base, f, F.in_set(base, "tenth") & ~ra, shapes=[MID], what="device ids")
    finally:
        hip.close()


def test_compose_term_counts_and_operands(base, case):
    w = base.gpu.filter_timestamps(*HALF)
    eight = case.terms(vip) + [Term.id_range(0, (4 << 40) - 1), ~Term.id_range(1 << 40, (2 << 40) - 1), Term.filter(w),
                               ~Term.timestamps(1100, 1199)]
    admit = (case.admit_and & F.in_range(base, 0, (4 << 40) - 1) & ~F.in_range(base, 1 << 40, (2 << 40) - 1)
             & ~F.in_window(base, (1100, 1199)))
    assert admit.sum() > 100
    F.check_all(base, base.gpu.filter_compose(eight), admit, what="eight terms")
    invalid(lambda: base.gpu.filter_compose(eight + [Term.id_range(0, 1)]))
    invalid(lambda: base.gpu.filter_compose([]))
    other = base.open()
    invalid(lambda: base.gpu.filter_compose([Term.timestamps(*HALF), Term.filter(other.filter_timestamps(*HALF))]))
    invalid(lambda: other.filter_compose([Term.filter(w)]))
    invalid(lambda: w | other.filter_timestamps(*HALF))
    invalid(lambda: other.filter_timestamps(*HALF) - w)


def test_compose_rejects_bad_arguments_through_the_raw_entry(base):
    L, h = N.lib(), base.gpu._h
    out = C.c_void_p(0x5A5A)
    ok = N.FilterTerm(kind=N.VI_TERM_ID_RANGE, lo=0, hi=9)
    ids = u64([1, 2, 3])

    def refused(join, terms, n, reuse=None):
        arr = (N.FilterTerm * max(len(terms), 1))(*terms)
        st = L.vi_indexer_filter_compose(h, join, arr, n, reuse, C.byref(out))
        return st == N.VI_ERR_INVALID_INPUT and bool(L.vi_last_error()) and out.value == 0x5A5A

    assert L.vi_indexer_filter_compose(h, N.VI_JOIN_AND, None, 1, None, C.byref(out)) == N.VI_ERR_INVALID_INPUT
    assert L.vi_indexer_filter_compose(h, N.VI_JOIN_AND, C.byref(ok), 1, None, None) == N.VI_ERR_INVALID_INPUT
    assert refused(2, [ok], 1) and refused(-1, [ok], 1)                                     # join
    assert refused(N.VI_JOIN_AND, [ok], 0) and refused(N.VI_JOIN_AND, [ok] * 9, 9)          # term count
    assert refused(N.VI_JOIN_AND, [N.FilterTerm(kind=7)], 1)                                # kind
    assert refused(N.VI_JOIN_AND, [N.FilterTerm(kind=N.VI_TERM_ID_RANGE, negate=2, lo=0, hi=9)], 1)
    for kind in (N.VI_TERM_IDS, N.VI_TERM_IDS_DEVICE, N.VI_TERM_MASK, N.VI_TERM_MASK_DEVICE):
        assert refused(N.VI_JOIN_AND, [N.FilterTerm(kind=kind, n=3)], 1)                    # null data with n > 0
    assert refused(N.VI_JOIN_AND, [N.FilterTerm(kind=N.VI_TERM_FILTER)], 1)                 # null operand
    assert refused(N.VI_JOIN_AND, [N.FilterTerm(kind=N.VI_TERM_IDS, data=ids.ctypes.data, n=(1 << 40) + 1)], 1)
    assert refused(N.VI_JOIN_OR, [ok, N.FilterTerm(kind=N.VI_TERM_TIMESTAMPS, lo=2, hi=1)], 2)
    assert out.value == 0x5A5A
    # fields a kind does not use are ignored
    noisy = N.FilterTerm(kind=N.VI_TERM_ID_RANGE, lo=0, hi=U64_MAX, data=0x10, n=5, filter=0x20)
    out = C.c_void_p()
    N.check(L.vi_indexer_filter_compose(h, N.VI_JOIN_AND, C.byref(noisy), 1, None, C.byref(out)))
    assert L.vi_filter_num_allowed(out) == base.n
    L.vi_filter_free(out)


# ---- 7. reuse ----
def test_reuse_overwrites_one_filter_in_place(base, case):
    exprs = [(case.terms(vip), False, case.admit_and),
             ([Term.ids(base.sets["tenth"]), ~Term.timestamps(*HALF)], True, F.in_set(base, "tenth") | ~F.in_window(base, HALF))]
    target = base.gpu.filter_ids(base.sets["n64"])
    handle = target._h.value
    for rnd in range(3):
        for terms, any_, admit in exprs:
            got = base.gpu.filter_compose(terms, any=any_, reuse=target)
            assert got is target and target._h.value == handle
            fresh = base.gpu.filter_compose(terms, any=any_)
            assert target.num_allowed == fresh.num_allowed == int(admit.sum())
            F.same_results(base, target, fresh, shapes=[MID, SHAPES[2]] if rnd else SHAPES)
            F.check(base, target, admit, *MID, what=f"reuse round {rnd}")
    # an operand may not be the filter to overwrite; the filter is left as it was
    _, _, admit = exprs[1]
    invalid(lambda: base.gpu.filter_compose([Term.timestamps(*HALF), Term.filter(target)], reuse=target))
    invalid(lambda: base.gpu.filter_compose([~Term.filter(target)], reuse=target))
    F.check_all(base, target, admit, what="after the refused calls")
    # ... another filter of the index as an operand is fine, and a reused filter of another handle is not
    w = base.gpu.filter_timestamps(*HALF)
    assert base.gpu.filter_compose([Term.filter(w)], reuse=target) is target
    F.check_all(base, target, F.in_window(base, HALF), shapes=[MID], what="reuse with an operand")
    invalid(lambda: base.gpu.filter_compose([Term.timestamps(*HALF)], reuse=base.open().filter_timestamps(*HALF)))


# ---- 8. engines and entries ----
def test_valu_engine(valu):
    c = F.AndCase(valu)
    F.check_all(valu, valu.gpu.filter_compose(c.terms(vip)), c.admit_and, what="valu")
    assert valu.gpu.last_stats()["rank_mode"] == 0


@pytest.mark.parametrize("rank_i8", ["1", "0"])
def test_byte_lists(bytes8, rank_i8, monkeypatch):
    monkeypatch.setenv("VI_RANK_I8", rank_i8)
    c = F.AndCase(bytes8)
    F.check_all(bytes8, bytes8.gpu.filter_compose(c.terms(vip)), c.admit_and, what=f"rank_i8 {rank_i8}")
    st = bytes8.gpu.last_stats()
    assert st["rank_mode"] == 3 and st["rank_int8"] == int(rank_i8), st


def test_forced_generic_engine(base, case, monkeypatch):
    monkeypatch.setenv("VI_FORCE_GENERIC", "1")
    F.check_all(base, base.gpu.filter_compose(case.terms(vip)), case.admit_and, what="generic")
    assert base.gpu.last_stats()["rank_mode"] == 0


def test_generic_engine_beyond_the_select_limits(base, case):
    """k = 200 > 128 takes the sort-everything engine"""
    flt = base.gpu.filter_compose(case.terms(vip))
    for nq in (1, 33):
        F.check(base, flt, case.admit_and, nq, 200, 8, what="k 200")


def test_radius_search(base, case):
    nq, p = 300, 8
    D, I = base.full(p)
    keep = (I >= 0) & case.admit_and[base.rows_of(I)]
    radius2 = float(np.median(np.sort(np.where(keep, D, np.inf), axis=1)[:, 19]))   # a 20th admitted candidate's distance
    assert np.isfinite(radius2)
    hit = keep & (D <= np.float32(radius2))
    per = hit.sum(axis=1)
    assert (per < 20).any() and (per >= 20).any()
    lims_e = np.concatenate([[0], np.cumsum(per)]).astype(np.uint64)
    lims, Dg, Ig = base.gpu.range_search_sync(base.Q[:nq], radius2, p, filter=base.gpu.filter_compose(case.terms(vip)))
    assert np.array_equal(lims, lims_e) and np.array_equal(Ig, I[hit]) and np.array_equal(bits(Dg), bits(D[hit]))


def test_faiss_style_adapter_takes_a_filter(base, case):
    flt = base.gpu.filter_compose(case.terms(vip))
    adapter = FaissStyleAdapter(base.gpu)
    adapter.nprobe = 8
    De, Ie, _ = F.expected(base, case.admit_and, 33, 10, 8)
    Da, Ia = adapter.search(base.Q[:33], 10, filter=flt)
    assert np.array_equal(Ia, Ie) and np.array_equal(bits(Da), bits(De))
    D, I = base.full(8)
    keep = (I[:1] >= 0) & case.admit_and[base.rows_of(I[:1])]
    radius2 = float(D[0][keep[0]][4])
    hit = keep[0] & (D[0] <= np.float32(radius2))
    lims, Dr, Ir = adapter.range_search(base.Q[:1], radius2, filter=flt)
    assert Ir.tolist() == I[0][hit].tolist() and lims.tolist() == [0, int(hit.sum())]
    for kw in ({"allowed_ids": [1]}, {"excluded_ids": [1]}):
        with pytest.raises(ValueError):
            adapter.search(base.Q[:3], 10, filter=flt, **kw)
        with pytest.raises(ValueError):
            adapter.range_search(base.Q[:3], 1.0, filter=flt, **kw)


# ---- 9. retain ----
def test_retain_a_union(tmp_path):
    rng = np.random.default_rng(31)
    n = 1500
    X = rng.standard_normal((n, 16)).astype(np.float32)
    ext, ts = F.ext_ids_for(n), F.timestamps_for(n)
    ix = vip.build(X, str(tmp_path), ext_ids=ext, timestamps=ts, now_secs=NOW, nlist=6)
    before = ix.export()[0]
    ids = ext[rng.choice(n, 200, replace=False)]
    admit = np.isin(ext, ids) | ((ts >= 1000) & (ts <= 1249))
    assert 200 < admit.sum() < n
    removed = ix.retain(ix.filter_ids(ids) | ix.filter_timestamps(1000, 1249))
    assert removed == n - admit.sum() and ix.num_vectors == admit.sum()
    assert np.array_equal(ix.export()[0], before[np.isin(before, ext[admit])])   # the admitted ids in their old list order


# ---- 10. two in-process ranks ----
@pytest.mark.parametrize("placement", [0, 1])
def test_two_ranks_each_with_its_own_mask_merge_to_the_single_gpu_result(base, placement):
    from hiprt import Hip
    world, nq = 2, 300
    parts = [base.open(rank=r, world_size=world, placement=placement) for r in range(world)]
    assert sum(p.num_vectors for p in parts) == base.n
    mask_rows = np.random.default_rng(41).random(base.n) < 0.6
    admit = F.in_window(base, HALF) & mask_rows
    filters = [p.filter_compose([Term.timestamps(*HALF), Term.mask(F.mask_for(base, mask_rows, p))]) for p in parts]
    assert sum(f.num_allowed for f in filters) == int(admit.sum())
    hip = Hip()
    try:
        xq = hip.upload(base.Q)
        for k, n_probe in [(10, 8), (200, 8)]:
            De, Ie, _ = F.expected(base, admit, nq, k, n_probe)
            S = int(N.lib().vi_packed_result_bytes(nq, k))
            off_i = (nq * k * 4 + 7) // 8 * 8
            packed, Dm, Im = hip.alloc(world * S), hip.alloc(nq * k * 4), hip.alloc(nq * k * 8)
            for r, p in enumerate(parts):
                b = packed + r * S
                p.search_device(xq, nq, k, n_probe, b, b + off_i, b + off_i + nq * k * 8, filter=filters[r])
            N.check(N.lib().vi_merge_partials_packed_device(0, nq, k, world, packed, Dm, Im))
            assert np.array_equal(hip.download(Im, (nq, k), np.int64), Ie), (k, n_probe)
            assert np.array_equal(bits(hip.download(Dm, (nq, k), np.float32)), bits(De)), (k, n_probe)
    finally:
        hip.close()
