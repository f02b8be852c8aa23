"""CPU: the entries of the C ABI for a radius search by stored record (vi_indexer_range_search_by_ids, host and device
form, and vi_indexer_radius_graph) exist in libvi_amd.so with the prototypes include/vi_amd.h documents, and the errors
that need no device are errors with a message that leave *out NULL and found untouched, not crashes.  (Loading the
library needs no GPU.)"""
import ctypes as C
import os

from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64, u32, f32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_float

# name -> (return type, argument types), as declared in include/vi_amd.h
PROTOTYPES = {
    "vi_indexer_range_search_by_ids": (C.c_int, [vp, vp, vp, u64, f32, u64, u32, vp, C.POINTER(vp)]),
    "vi_indexer_range_search_by_ids_device": (C.c_int, [vp, vp, vp, u64, f32, u64, u32, vp, C.POINTER(vp)]),
    "vi_indexer_radius_graph": (C.c_int, [vp, vp, u64, u64, f32, u64, u32, C.POINTER(vp)]),
}
DECLARATIONS = [
    "vi_status vi_indexer_range_search_by_ids(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids, uint64_t nq, "
    "float radius2, uint64_t n_probe, uint32_t exclude_self, uint32_t *found, "
    "vi_range_result **out);",
    "vi_status vi_indexer_range_search_by_ids_device(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids_dev, uint64_t nq, "
    "float radius2, uint64_t n_probe, uint32_t exclude_self, uint32_t *found_dev, "
    "vi_range_result **out);",
    "vi_status vi_indexer_radius_graph(const vi_indexer *ix, const vi_filter *f, uint64_t first, uint64_t count, float radius2, "
    "uint64_t n_probe, uint32_t exclude_self, vi_range_result **out);",
]


def new_handle(dim=8):
    """a handle from vi_indexer_new: it holds no index"""
    cfg = N.Config()
    N.lib().vi_config_init(C.byref(cfg), dim)
    h = vp()
    N.check(N.lib().vi_indexer_new(C.byref(cfg), C.byref(h)))
    return h


class Out:
    """a result pointer that starts NULL and a found array with a pattern that shows any write"""

    def __init__(self):
        self.res, self.found = vp(), (u32 * 3)(7, 7, 7)

    def untouched(self):
        return self.res.value is None and list(self.found) == [7] * 3


def by_ids(L, h, ids, nq, r2, p, o, out=True, device=False):
    fn = L.vi_indexer_range_search_by_ids_device if device else L.vi_indexer_range_search_by_ids
    return fn(h, None, ids, nq, r2, p, 1, o.found, C.byref(o.res) if out else None)


def graph(L, h, first, count, r2, p, o, out=True):
    return L.vi_indexer_radius_graph(h, None, first, count, r2, p, 1, C.byref(o.res) if out else None)


def test_the_three_symbols_resolve_with_the_documented_prototypes():
    L = N.lib()
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)      # AttributeError: not exported
        assert fn.restype is res or fn.restype == res, name
        assert list(fn.argtypes) == args, name
        assert N.SIGNATURES[name] == (res, args), name


def test_abi_version_is_still_2_and_the_header_declares_the_entries_verbatim():
    assert N.lib().vi_abi_version() == 2
    flat = " ".join(open(os.path.join(ROOT, "include", "vi_amd.h")).read().split())
    assert "#define VI_AMD_ABI_VERSION 2" in flat
    for decl in DECLARATIONS:
        assert " ".join(decl.split()) in flat, decl


def test_null_indexer_is_an_error_with_a_message():
    L = N.lib()
    ids, o = (u64 * 3)(1, 2, 3), Out()
    for call in (lambda: by_ids(L, None, ids, 3, 1.0, 2, o),
                 lambda: by_ids(L, None, ids, 3, 1.0, 2, o, device=True),
                 lambda: by_ids(L, None, None, 0, 1.0, 2, o),
                 lambda: graph(L, None, 0, 3, 1.0, 2, o),
                 lambda: graph(L, None, 0, 0, 1.0, 2, o)):
        assert call() == N.VI_ERR_INVALID_INPUT
        assert L.vi_last_error()
        assert o.untouched()


def test_bad_arguments_are_errors_before_any_device_work_and_write_nothing():
    L = N.lib()
    h = new_handle()
    try:
        ids, o = (u64 * 3)(1, 2, 3), Out()
        nan, big = float("nan"), (1 << 40) + 1
        both = lambda *a, **k: [lambda: by_ids(L, h, *a, **k), lambda: by_ids(L, h, *a, device=True, **k)]  # noqa: E731
        calls = {
            "no index": both(ids, 3, 1.0, 2, o) + [lambda: graph(L, h, 0, 3, 1.0, 2, o), lambda: graph(L, h, 0, 0, 1.0, 2, o)],
            "null ids": both(None, 3, 1.0, 2, o),
            "null out": both(ids, 3, 1.0, 2, o, out=False) + [lambda: graph(L, h, 0, 3, 1.0, 2, o, out=False)],
            "n_probe == 0": both(ids, 3, 1.0, 0, o) + [lambda: graph(L, h, 0, 3, 1.0, 0, o)],
            "NaN radius2": both(ids, 3, nan, 2, o) + [lambda: graph(L, h, 0, 3, nan, 2, o)],
            "nq past 2^40": both(ids, big, 1.0, 2, o) + [lambda: graph(L, h, 0, big, 1.0, 2, o)],
        }
        for what, cs in calls.items():
            for i, call in enumerate(cs):
                assert call() == N.VI_ERR_INVALID_INPUT, (what, i)
                assert L.vi_last_error(), (what, i)
                assert o.untouched(), (what, i)
        assert by_ids(L, h, ids, 3, 1.0, 2, o) == N.VI_ERR_INVALID_INPUT and b"no index" in L.vi_last_error()
        assert by_ids(L, h, None, 3, 1.0, 2, o) == N.VI_ERR_INVALID_INPUT and b"null id" in L.vi_last_error()
        assert by_ids(L, h, ids, 3, nan, 2, o) == N.VI_ERR_INVALID_INPUT and b"NaN" in L.vi_last_error()
        assert by_ids(L, h, ids, 3, 1.0, 0, o) == N.VI_ERR_INVALID_INPUT and b"n_probe" in L.vi_last_error()
    finally:
        L.vi_indexer_free(h)


def test_an_error_resets_a_stale_result_pointer_to_null():
    """*out is NULL after a failed call whatever it held before (no result is ever half returned)"""
    L = N.lib()
    h = new_handle()
    try:
        ids, found = (u64 * 3)(1, 2, 3), (u32 * 3)(7, 7, 7)
        res = vp(0xDEAD0)
        assert L.vi_indexer_range_search_by_ids(h, None, ids, 3, 1.0, 2, 1, found, C.byref(res)) == N.VI_ERR_INVALID_INPUT
        assert res.value is None and list(found) == [7] * 3
        res = vp(0xDEAD0)
        assert L.vi_indexer_radius_graph(h, None, 0, 3, 1.0, 2, 1, C.byref(res)) == N.VI_ERR_INVALID_INPUT
        assert res.value is None
    finally:
        L.vi_indexer_free(h)
