"""CPU: the entries of the C ABI that read records back exist in libvi_amd.so with the prototypes include/vi_amd.h
documents, and the errors that need no device are errors, not crashes.  (Loading the library needs no GPU.)"""
import ctypes as C
import os
import re

from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64 = C.c_void_p, C.c_uint64

# name -> (return type, argument types), as declared in include/vi_amd.h
PROTOTYPES = {
    "vi_indexer_get_records": (C.c_int, [vp, vp, u64, vp, vp, vp, vp]),
    "vi_indexer_get_records_device": (C.c_int, [vp, vp, u64, vp, vp, vp, vp]),
    "vi_indexer_export_records": (C.c_int, [vp, u64, u64, vp, vp, vp, vp]),
    "vi_indexer_export_records_device": (C.c_int, [vp, u64, u64, vp, vp, vp, vp]),
    "vi_indexer_last_fetch_stats": (C.c_int, [vp, C.POINTER(N.FetchStats)]),
}


def new_handle(dim=8):
    """a handle from vi_indexer_new: it holds no index"""
    cfg = N.Config()
    N.lib().vi_config_init(C.byref(cfg), dim)
    h = vp()
    N.check(N.lib().vi_indexer_new(C.byref(cfg), C.byref(h)))
    return h


def test_the_five_symbols_resolve_with_the_documented_prototypes():
    L = N.lib()
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)      # AttributeError: not exported
        assert fn.restype is res or fn.restype == res, name
        assert list(fn.argtypes) == args, name
        assert N.SIGNATURES[name] == (res, args), name


def test_null_indexer_is_an_error_with_a_message():
    L = N.lib()
    ids = (u64 * 3)(1, 2, 3)
    for call in (lambda: L.vi_indexer_get_records(None, ids, 3, None, None, None, None),
                 lambda: L.vi_indexer_get_records_device(None, ids, 3, None, None, None, None),
                 lambda: L.vi_indexer_get_records(None, None, 0, None, None, None, None),
                 lambda: L.vi_indexer_export_records(None, 0, 0, None, None, None, None),
                 lambda: L.vi_indexer_export_records_device(None, 0, 1, None, None, None, None)):
        assert call() == N.VI_ERR_INVALID_INPUT
        assert L.vi_last_error()


def test_a_handle_without_an_index_is_an_error_before_any_device_work():
    L = N.lib()
    h = new_handle()
    try:
        ids = (u64 * 3)(1, 2, 3)
        cnt = (C.c_uint32 * 3)(7, 7, 7)
        assert L.vi_indexer_get_records(h, None, 3, cnt, None, None, None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()
        assert L.vi_indexer_get_records_device(h, None, 3, None, None, None, None) == N.VI_ERR_INVALID_INPUT
        assert L.vi_indexer_get_records(h, ids, 3, cnt, None, None, None) == N.VI_ERR_INVALID_INPUT
        assert b"no index" in L.vi_last_error()
        assert L.vi_indexer_get_records(h, ids, (1 << 40) + 1, cnt, None, None, None) == N.VI_ERR_INVALID_INPUT
        assert L.vi_indexer_export_records(h, 0, 1, None, None, None, None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()
        assert list(cnt) == [7, 7, 7]    # nothing was written
    finally:
        L.vi_indexer_free(h)


def test_fetch_stats_of_nothing_is_an_error():
    L = N.lib()
    st = N.FetchStats()
    assert L.vi_indexer_last_fetch_stats(None, C.byref(st)) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()
    h = new_handle()
    try:
        assert L.vi_indexer_last_fetch_stats(h, None) == N.VI_ERR_INVALID_INPUT
    finally:
        L.vi_indexer_free(h)


def test_abi_version_is_still_2_and_the_header_declares_the_entries():
    assert N.lib().vi_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "vi_amd.h")).read()
    flat = " ".join(hdr.split())
    assert "#define VI_AMD_ABI_VERSION 2" in flat and "#define VI_WHERE_NONE UINT64_MAX" in flat
    for name in PROTOTYPES:
        assert re.search(r"\bvi_status\s+%s\(" % name, hdr), name
    assert ("vi_status vi_indexer_get_records(const vi_indexer *ix, const uint64_t *ext_ids, uint64_t n, uint32_t *count_out, "
            "float *values_out, uint64_t *timestamps_out, uint64_t *where_out);") in flat
    assert ("vi_status vi_indexer_export_records_device(const vi_indexer *ix, uint64_t first, uint64_t count, "
            "uint64_t *ext_ids_dev, float *values_dev, uint64_t *timestamps_dev, uint64_t *where_dev);") in flat
    assert ("typedef struct vi_fetch_stats { uint64_t n;" in flat) and "float ms_gather;" in flat
    assert C.sizeof(N.FetchStats) == 48 and N.WHERE_NONE == (1 << 64) - 1
