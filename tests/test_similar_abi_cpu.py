"""CPU: the entries of the C ABI that search by stored record (vi_indexer_search_by_ids / vi_indexer_knn_graph, host and
device forms) exist in libvi_amd.so with the prototypes include/vi_amd.h documents, and the errors that need no device
are errors with a message that write no output, not crashes.  (Loading the library needs no GPU.)"""
import ctypes as C
import os

from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32

# name -> (return type, argument types), as declared in include/vi_amd.h
PROTOTYPES = {
    "vi_indexer_search_by_ids": (C.c_int, [vp, vp, vp, u64, u64, u64, u32, vp, vp, vp, vp, vp, C.POINTER(u64)]),
    "vi_indexer_search_by_ids_device": (C.c_int, [vp, vp, vp, u64, u64, u64, u32, vp, vp, vp, vp]),
    "vi_indexer_knn_graph": (C.c_int, [vp, vp, u64, u64, u64, u64, u32, vp, vp, vp, C.POINTER(u64)]),
    "vi_indexer_knn_graph_device": (C.c_int, [vp, vp, u64, u64, u64, u64, u32, vp, vp, vp]),
}
DECLARATIONS = [
    "vi_status vi_indexer_search_by_ids(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids, uint64_t nq, "
    "uint64_t k, uint64_t n_probe, uint32_t exclude_self, float *D, int64_t *I, float *V, "
    "uint64_t *counts, uint32_t *found, uint64_t *k_out);",
    "vi_status vi_indexer_search_by_ids_device(const vi_indexer *ix, const vi_filter *f, const uint64_t *ext_ids_dev, uint64_t nq, "
    "uint64_t k, uint64_t n_probe, uint32_t exclude_self, float *D_dev, int64_t *I_dev, "
    "uint64_t *tie_dev, uint32_t *found_dev);",
    "vi_status vi_indexer_knn_graph(const vi_indexer *ix, const vi_filter *f, uint64_t first, uint64_t count, uint64_t k, "
    "uint64_t n_probe, uint32_t exclude_self, float *D, int64_t *I, uint64_t *counts, uint64_t *k_out);",
    "vi_status vi_indexer_knn_graph_device(const vi_indexer *ix, const vi_filter *f, uint64_t first, uint64_t count, uint64_t k, "
    "uint64_t n_probe, uint32_t exclude_self, float *D_dev, int64_t *I_dev, uint64_t *tie_dev);",
]


def new_handle(dim=8):
    """a handle from vi_indexer_new: it holds no index"""
    cfg = N.Config()
    N.lib().vi_config_init(C.byref(cfg), dim)
    h = vp()
    N.check(N.lib().vi_indexer_new(C.byref(cfg), C.byref(h)))
    return h


class Out:
    """output arrays of three rows of k = 4 with a pattern that shows any write"""

    def __init__(self):
        self.D, self.I = (C.c_float * 12)(*[7.0] * 12), (C.c_int64 * 12)(*[7] * 12)
        self.counts, self.found, self.k_out = (u64 * 3)(7, 7, 7), (u32 * 3)(7, 7, 7), u64(7)

    def untouched(self):
        return (list(self.D) == [7.0] * 12 and list(self.I) == [7] * 12 and list(self.counts) == [7] * 3
                and list(self.found) == [7] * 3 and self.k_out.value == 7)


def by_ids(L, h, ids, nq, k, p, o, D="D", I="I"):
    return L.vi_indexer_search_by_ids(h, None, ids, nq, k, p, 1, o.D if D else None, o.I if I else None, None, o.counts, o.found,
                                      C.byref(o.k_out))


def graph(L, h, first, count, k, p, o, D="D", I="I"):
    return L.vi_indexer_knn_graph(h, None, first, count, k, p, 1, o.D if D else None, o.I if I else None, o.counts, C.byref(o.k_out))


def test_the_four_symbols_resolve_with_the_documented_prototypes():
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
    for call in (lambda: by_ids(L, None, ids, 3, 4, 2, o),
                 lambda: L.vi_indexer_search_by_ids_device(None, None, ids, 3, 4, 2, 1, o.D, o.I, None, None),
                 lambda: by_ids(L, None, None, 0, 4, 2, o),
                 lambda: graph(L, None, 0, 3, 4, 2, o),
                 lambda: L.vi_indexer_knn_graph_device(None, None, 0, 3, 4, 2, 0, o.D, o.I, None)):
        assert call() == N.VI_ERR_INVALID_INPUT
        assert L.vi_last_error()
    assert o.untouched()


def test_bad_arguments_are_errors_before_any_device_work_and_write_nothing():
    L = N.lib()
    h = new_handle()
    try:
        ids, o = (u64 * 3)(1, 2, 3), Out()
        dev = lambda *a: L.vi_indexer_search_by_ids_device(h, None, *a)          # noqa: E731
        gdev = lambda *a: L.vi_indexer_knn_graph_device(h, None, *a)             # noqa: E731
        calls = {
            "no index": [lambda: by_ids(L, h, ids, 3, 4, 2, o), lambda: dev(ids, 3, 4, 2, 1, o.D, o.I, None, None),
                         lambda: graph(L, h, 0, 3, 4, 2, o), lambda: gdev(0, 3, 4, 2, 1, o.D, o.I, None)],
            "null ids": [lambda: by_ids(L, h, None, 3, 4, 2, o), lambda: dev(None, 3, 4, 2, 1, o.D, o.I, None, None)],
            "null D": [lambda: by_ids(L, h, ids, 3, 4, 2, o, D=None), lambda: dev(ids, 3, 4, 2, 1, None, o.I, None, None),
                       lambda: graph(L, h, 0, 3, 4, 2, o, D=None), lambda: gdev(0, 3, 4, 2, 1, None, o.I, None)],
            "null I": [lambda: by_ids(L, h, ids, 3, 4, 2, o, I=None), lambda: dev(ids, 3, 4, 2, 1, o.D, None, None, None),
                       lambda: graph(L, h, 0, 3, 4, 2, o, I=None), lambda: gdev(0, 3, 4, 2, 1, o.D, None, None)],
            "k == 0": [lambda: by_ids(L, h, ids, 3, 0, 2, o), lambda: dev(ids, 3, 0, 2, 1, o.D, o.I, None, None),
                       lambda: graph(L, h, 0, 3, 0, 2, o), lambda: gdev(0, 3, 0, 2, 1, o.D, o.I, None)],
            "n_probe == 0": [lambda: by_ids(L, h, ids, 3, 4, 0, o), lambda: dev(ids, 3, 4, 0, 1, o.D, o.I, None, None),
                             lambda: graph(L, h, 0, 3, 4, 0, o), lambda: gdev(0, 3, 4, 0, 1, o.D, o.I, None)],
            "nq past 2^40": [lambda: by_ids(L, h, ids, (1 << 40) + 1, 4, 2, o),
                             lambda: dev(ids, (1 << 40) + 1, 4, 2, 1, o.D, o.I, None, None),
                             lambda: graph(L, h, 0, (1 << 40) + 1, 4, 2, o), lambda: gdev(0, (1 << 40) + 1, 4, 2, 1, o.D, o.I, None)],
        }
        for what, cs in calls.items():
            for i, call in enumerate(cs):
                assert call() == N.VI_ERR_INVALID_INPUT, (what, i)
                assert L.vi_last_error(), (what, i)
        assert by_ids(L, h, ids, 3, 4, 2, o) == N.VI_ERR_INVALID_INPUT and b"no index" in L.vi_last_error()
        assert by_ids(L, h, None, 3, 4, 2, o) == N.VI_ERR_INVALID_INPUT and b"null id" in L.vi_last_error()
        assert o.untouched()
    finally:
        L.vi_indexer_free(h)
