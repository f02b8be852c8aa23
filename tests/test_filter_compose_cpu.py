"""No GPU: the compound-filter entries of the C ABI (vi_indexer_filter_compose and the five thin calls into it) exist, are
declared to ctypes, and reject bad arguments before any device work; the Term objects of the Python mirror normalise what
they carry."""
import ctypes as C

import numpy as np
import pytest

import vector_indexer_py as vip
from vector_indexer_py import _native as N

ENTRIES = ["vi_indexer_filter_compose", "vi_filter_union", "vi_filter_complement", "vi_indexer_filter_id_range",
           "vi_indexer_filter_mask", "vi_indexer_filter_mask_device"]
SENTINEL = 0x5A5A5A5A


def last_error():
    return (N.lib().vi_last_error() or b"").decode()


def rejected(status, out):
    """INVALID_INPUT with a message, and *out as it was"""
    return status == N.VI_ERR_INVALID_INPUT and bool(last_error()) and out.value == SENTINEL


def test_the_entries_resolve_in_the_library_and_in_the_prototype_table():
    raw = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert getattr(raw, name) is not None
        assert name in N.SIGNATURES and getattr(N.lib(), name).restype is C.c_int
    assert N.lib().vi_abi_version() == 2   # (purely additive)


def test_the_enum_values_and_the_term_structure():
    assert (N.VI_TERM_TIMESTAMPS, N.VI_TERM_ID_RANGE, N.VI_TERM_IDS, N.VI_TERM_IDS_DEVICE, N.VI_TERM_MASK,
            N.VI_TERM_MASK_DEVICE, N.VI_TERM_FILTER) == (0, 1, 2, 3, 4, 5, 6)
    assert (N.VI_JOIN_AND, N.VI_JOIN_OR) == (0, 1) and N.VI_FILTER_MAX_TERMS == 8
    T = N.FilterTerm
    assert [f for f, _ in T._fields_] == ["kind", "negate", "lo", "hi", "data", "n", "filter"]
    assert C.sizeof(T) == 48 and (T.lo.offset, T.hi.offset, T.data.offset, T.n.offset, T.filter.offset) == (8, 16, 24, 32, 40)


def test_null_arguments_are_invalid_input_with_a_message_and_out_is_untouched():
    L = N.lib()
    term = N.FilterTerm(kind=N.VI_TERM_ID_RANGE, lo=1, hi=2)
    out = C.c_void_p(SENTINEL)
    for join in (N.VI_JOIN_AND, N.VI_JOIN_OR):
        assert rejected(L.vi_indexer_filter_compose(None, join, C.byref(term), 1, None, C.byref(out)), out)   # ix
    # (terms == NULL and out == NULL with a live handle are in the GPU tests; with a null handle each alone is refused too)
    assert rejected(L.vi_indexer_filter_compose(None, N.VI_JOIN_AND, None, 1, None, C.byref(out)), out)
    assert L.vi_indexer_filter_compose(None, N.VI_JOIN_AND, C.byref(term), 1, None, None) == N.VI_ERR_INVALID_INPUT
    assert last_error()
    mask = np.ones(3, dtype=np.uint8)
    assert rejected(L.vi_filter_union(None, None, None, C.byref(out)), out)
    assert rejected(L.vi_filter_complement(None, None, C.byref(out)), out)
    assert rejected(L.vi_indexer_filter_id_range(None, 0, 1, C.byref(out)), out)
    assert rejected(L.vi_indexer_filter_mask(None, N.ptr(mask), 3, C.byref(out)), out)
    assert rejected(L.vi_indexer_filter_mask_device(None, None, 0, C.byref(out)), out)
    for call in (lambda: L.vi_filter_union(None, None, None, None), lambda: L.vi_filter_complement(None, None, None),
                 lambda: L.vi_indexer_filter_id_range(None, 0, 1, None), lambda: L.vi_indexer_filter_mask(None, None, 0, None),
                 lambda: L.vi_indexer_filter_mask_device(None, None, 0, None)):
        assert call() == N.VI_ERR_INVALID_INPUT and last_error()


def test_terms_normalise_ids_to_u64_and_masks_to_uint8():
    t = vip.Term.ids([5, 3, 5, 2**64 - 1])
    assert t.kind == N.VI_TERM_IDS and t.data.dtype == np.uint64 and t.data.tolist() == [5, 3, 5, 2**64 - 1] and t.n == 4
    assert vip.Term.ids(np.array([[1, 2], [3, 4]], dtype=np.int32)).data.tolist() == [1, 2, 3, 4]
    assert vip.Term.ids([]).n == 0
    with pytest.raises(ValueError):
        vip.Term.ids([-1])
    with pytest.raises(TypeError):
        vip.Term.ids([1.5])
    m = vip.Term.mask(np.array([True, False, True]))
    assert m.kind == N.VI_TERM_MASK and m.data.dtype == np.uint8 and m.data.tolist() == [1, 0, 1] and m.n == 3
    m = vip.Term.mask(np.array([[0, 2], [0x80, 0]], dtype=np.uint8))
    assert m.data.tolist() == [0, 2, 0x80, 0] and m.data.flags.c_contiguous and m.n == 4
    assert vip.Term.mask([True, False]).data.tolist() == [1, 0]
    with pytest.raises(TypeError):
        vip.Term.mask(np.zeros(3, dtype=np.int64))
    with pytest.raises(TypeError):
        vip.Term.filter("not a filter")


def test_negation_is_carried_through_invert_and_into_the_native_term():
    t = vip.Term.timestamps(10, 20)
    assert (t.kind, t.lo, t.hi, t.negate) == (N.VI_TERM_TIMESTAMPS, 10, 20, False)
    n = ~t
    assert n.negate and not t.negate and (n.kind, n.lo, n.hi) == (t.kind, 10, 20) and not (~n).negate
    r = ~vip.Term.id_range(0, 2**64 - 1)
    c = r._native_term()
    assert (c.kind, c.negate, c.lo, c.hi, c.data, c.n, c.filter) == (N.VI_TERM_ID_RANGE, 1, 0, 2**64 - 1, None, 0, None)
    ids = ~vip.Term.ids([7, 9])
    c = ids._native_term()
    assert (c.kind, c.negate, c.n) == (N.VI_TERM_IDS, 1, 2) and c.data == ids.data.ctypes.data
    d = vip.Term.ids_device(0x1000, 5)._native_term()
    assert (d.kind, d.negate, d.data, d.n) == (N.VI_TERM_IDS_DEVICE, 0, 0x1000, 5)
    md = (~vip.Term.mask_device(0x2000, 6))._native_term()
    assert (md.kind, md.negate, md.data, md.n) == (N.VI_TERM_MASK_DEVICE, 1, 0x2000, 6)
    e = vip.Term.ids([])._native_term()
    assert e.data is None and e.n == 0
