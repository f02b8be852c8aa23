"""CPU: the radius-search entries of the C ABI exist in libvi_amd.so with the prototypes include/vi_amd.h documents, and
the two that take no index are safe on NULL.  (Loading the library needs no GPU.)"""
import ctypes as C
import os
import re

from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64, u32, f32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_float

# name -> (return type, argument types), as declared in include/vi_amd.h
PROTOTYPES = {
    "vi_indexer_range_search": (C.c_int, [vp, vp, vp, u64, u32, f32, u64, C.POINTER(vp)]),
    "vi_indexer_range_search_device": (C.c_int, [vp, vp, vp, u64, f32, u64, C.POINTER(vp)]),
    "vi_range_result_total": (u64, [vp]),
    "vi_range_result_copy": (C.c_int, [vp, vp, vp, vp, vp]),
    "vi_range_result_device": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
    "vi_range_result_free": (None, [vp]),
}


def test_the_six_symbols_resolve_with_the_documented_prototypes():
    L = N.lib()
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)      # AttributeError: not exported
        assert fn.restype is res or fn.restype == res, name
        assert list(fn.argtypes) == args, name
        assert N.SIGNATURES[name] == (res, args), name


def test_free_and_total_are_safe_on_null():
    L = N.lib()
    L.vi_range_result_free(None)
    assert L.vi_range_result_total(None) == 0


def test_null_result_and_null_indexer_are_errors_not_crashes():
    L = N.lib()
    out = vp()
    assert L.vi_range_result_copy(None, None, None, None, None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()
    assert L.vi_range_result_device(None, None, None, None, None) == N.VI_ERR_INVALID_INPUT
    assert L.vi_indexer_range_search(None, None, None, 0, 4, 1.0, 1, C.byref(out)) == N.VI_ERR_INVALID_INPUT
    assert L.vi_indexer_range_search_device(None, None, None, 0, 1.0, 1, C.byref(out)) == N.VI_ERR_INVALID_INPUT
    assert not out.value


def test_abi_version_is_still_2():
    assert N.lib().vi_abi_version() == 2


def test_the_header_declares_the_six_symbols():
    hdr = open(os.path.join(ROOT, "include", "vi_amd.h")).read()
    assert "typedef struct vi_range_result vi_range_result;" in hdr
    for name in PROTOTYPES:
        assert re.search(r"\b(vi_status|uint64_t|void)\s+%s\(" % name, hdr), name
    flat = " ".join(hdr.split())
    assert ("vi_status vi_indexer_range_search(const vi_indexer *ix, const vi_filter *f, const float *queries, uint64_t nq, "
            "uint32_t query_dim, float radius2, uint64_t n_probe, vi_range_result **out);") in flat
    assert ("vi_status vi_indexer_range_search_device(const vi_indexer *ix, const vi_filter *f, const float *queries_dev, uint64_t nq, "
            "float radius2, uint64_t n_probe, vi_range_result **out);") in flat
    assert "#define VI_AMD_ABI_VERSION 2" in flat
