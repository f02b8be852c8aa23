"""No GPU: the id-filter entries of the C ABI (vi_indexer_filter_ids, _device, vi_filter_intersect) exist, are declared to
ctypes, and reject bad arguments before any device work; the request side of the Python mirror normalises an id set."""
import ctypes as C

import numpy as np

from vector_indexer_py import _native as N
from vector_indexer_py.api import SearchRequest

ENTRIES = ["vi_indexer_filter_ids", "vi_indexer_filter_ids_device", "vi_filter_intersect"]


def last_error():
    return (N.lib().vi_last_error() or b"").decode()


def test_the_entries_resolve_in_the_library_and_in_the_prototype_table():
    raw = C.CDLL(N.LIB_PATH)
    for name in ENTRIES:
        assert getattr(raw, name) is not None
        assert name in N.SIGNATURES and getattr(N.lib(), name).restype is C.c_int
    assert (N.VI_IDS_ALLOW, N.VI_IDS_DENY) == (0, 1)
    assert N.lib().vi_abi_version() == 2   # (purely additive)


def test_null_arguments_are_invalid_input_with_a_message():
    L = N.lib()
    ids = np.array([1, 2, 3], dtype=np.uint64)
    out = C.c_void_p()
    for entry in (L.vi_indexer_filter_ids, L.vi_indexer_filter_ids_device):
        for mode in (N.VI_IDS_ALLOW, N.VI_IDS_DENY):
            assert entry(None, N.ptr(ids), 3, mode, C.byref(out)) == N.VI_ERR_INVALID_INPUT
            assert last_error()
            assert entry(None, None, 0, mode, None) == N.VI_ERR_INVALID_INPUT   # out == NULL
            assert last_error()
    assert L.vi_filter_intersect(None, None, None, C.byref(out)) == N.VI_ERR_INVALID_INPUT
    assert last_error()
    assert L.vi_filter_intersect(None, None, None, None) == N.VI_ERR_INVALID_INPUT
    assert not out.value
    assert L.vi_filter_num_allowed(None) == 0
    L.vi_filter_free(None)


def test_search_request_keeps_a_sorted_unique_u64_set_and_a_cache_key():
    req = SearchRequest([0.0, 1.0]).with_allowed_ids([5, 3, 5])
    sel = req.id_selector
    assert sel.ids.dtype == np.uint64 and sel.ids.tolist() == [3, 5] and not sel.exclude
    assert not sel.ids.flags.writeable
    again = SearchRequest([2.0, 3.0]).with_allowed_ids(np.array([3, 5, 3, 3], dtype=np.int32)).id_selector
    assert again.key == sel.key and hash(again.key) == hash(sel.key)
    denied = req.with_excluded_ids([3, 5]).id_selector
    assert denied.exclude and denied.key != sel.key and denied.digest == sel.digest
    assert SearchRequest([0.0]).with_allowed_ids([3, 6]).id_selector.key != sel.key
    assert SearchRequest([0.0]).with_allowed_ids([]).id_selector.ids.size == 0
    assert SearchRequest([0.0]).with_allowed_ids([0, 2**64 - 1]).id_selector.ids.tolist() == [0, 2**64 - 1]
    both = req.with_timestamp_range(10, 20)
    assert both.id_selector is sel and both.timestamp_range == (10, 20) and req.timestamp_range is None
    assert SearchRequest([0.0]).id_selector is None
