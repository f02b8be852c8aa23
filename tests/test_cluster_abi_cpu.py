"""CPU: the entries of the C ABI for clustering the stored records by radius (vi_indexer_cluster_radius, host and device
form, and vi_cluster_last_stats) exist in libvi_amd.so with the prototypes include/vi_amd.h documents, and the errors that
need no device are errors with a message that write none of the outputs, not crashes.  (Loading the library needs no
GPU.)"""
import ctypes as C
import os
import threading

from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64, u32, f32, i64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_int64

# name -> (return type, argument types), as declared in include/vi_amd.h
PROTOTYPES = {
    "vi_indexer_cluster_radius": (C.c_int, [vp, vp, f32, u64, u32, vp, vp, C.POINTER(u64)]),
    "vi_indexer_cluster_radius_device": (C.c_int, [vp, vp, f32, u64, u32, vp, vp, C.POINTER(u64)]),
    "vi_cluster_last_stats": (C.c_int, [C.POINTER(N.ClusterStats)]),
}
DECLARATIONS = [
    "#define VI_LABEL_NOISE (-1)",
    "vi_status vi_indexer_cluster_radius(const vi_indexer *ix, const vi_filter *f, float radius2, uint64_t n_probe, "
    "uint32_t min_pts, int64_t *labels_out, uint32_t *degree_out, uint64_t *n_clusters_out);",
    "vi_status vi_indexer_cluster_radius_device(const vi_indexer *ix, const vi_filter *f, float radius2, uint64_t n_probe, "
    "uint32_t min_pts, int64_t *labels_dev, uint32_t *degree_dev, uint64_t *n_clusters_out);",
    "typedef struct vi_cluster_stats { uint64_t rows, hits, passes; uint64_t n_core, n_border, n_noise, n_clusters; "
    "uint64_t chunk_rows, link_bytes; float ms_resolve, ms_search, ms_link, ms_label; } vi_cluster_stats;",
    "vi_status vi_cluster_last_stats(vi_cluster_stats *out);",
]


def new_handle(dim=8):
    """a handle from vi_indexer_new: it holds no index"""
    cfg = N.Config()
    N.lib().vi_config_init(C.byref(cfg), dim)
    h = vp()
    N.check(N.lib().vi_indexer_new(C.byref(cfg), C.byref(h)))
    return h


class Out:
    """the three outputs with a pattern that shows any write"""

    def __init__(self):
        self.labels, self.degree, self.n = (i64 * 3)(7, 7, 7), (u32 * 3)(7, 7, 7), u64(7)

    def untouched(self):
        return list(self.labels) == [7] * 3 and list(self.degree) == [7] * 3 and self.n.value == 7


def cluster(L, h, r2, p, min_pts, o, device=False, outputs=True):
    fn = L.vi_indexer_cluster_radius_device if device else L.vi_indexer_cluster_radius
    if not outputs:
        return fn(h, None, r2, p, min_pts, None, None, None)
    return fn(h, None, r2, p, min_pts, o.labels, o.degree, C.byref(o.n))


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


def test_the_stats_structure_is_the_headers():
    fields = [(n, t) for n, t in N.ClusterStats._fields_]
    names = ["rows", "hits", "passes", "n_core", "n_border", "n_noise", "n_clusters", "chunk_rows", "link_bytes",
             "ms_resolve", "ms_search", "ms_link", "ms_label"]
    assert [n for n, _ in fields] == names
    assert all(t is u64 for _, t in fields[:9]) and all(t is f32 for _, t in fields[9:])
    assert C.sizeof(N.ClusterStats) == 9 * 8 + 4 * 4
    L = N.lib()
    assert L.vi_cluster_last_stats(None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()
    st = N.ClusterStats()
    st.rows = st.passes = 99

    def fresh():        # a thread that has clustered nothing reads zeros: the figures are the calling thread's own
        assert L.vi_cluster_last_stats(C.byref(st)) == N.VI_OK

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert st.rows == 0 and st.passes == 0


def test_null_indexer_is_an_error_with_a_message():
    L = N.lib()
    o = Out()
    for device in (False, True):
        assert cluster(L, None, 1.0, 2, 1, o, device) == N.VI_ERR_INVALID_INPUT
        assert L.vi_last_error()
        assert o.untouched()


def test_bad_arguments_are_errors_before_any_device_work_and_write_nothing():
    L = N.lib()
    h = new_handle()
    try:
        o = Out()
        nan = float("nan")
        both = lambda *a, **k: [lambda: cluster(L, h, *a, device=False, **k), lambda: cluster(L, h, *a, device=True, **k)]  # noqa: E731
        calls = {
            "no index": both(1.0, 2, 1, o) + both(0.0, 2, 5, o) + both(-1.0, 2, 0, o),
            "n_probe == 0": both(1.0, 0, 1, o),
            "NaN radius2": both(nan, 2, 1, o),
            "all outputs NULL": both(1.0, 2, 1, o, outputs=False),
        }
        for what, cs in calls.items():
            for i, call in enumerate(cs):
                assert call() == N.VI_ERR_INVALID_INPUT, (what, i)
                assert L.vi_last_error(), (what, i)
                assert o.untouched(), (what, i)
        assert cluster(L, h, 1.0, 2, 1, o) == N.VI_ERR_INVALID_INPUT and b"no index" in L.vi_last_error()
        assert cluster(L, h, nan, 2, 1, o) == N.VI_ERR_INVALID_INPUT and b"NaN" in L.vi_last_error()
        assert cluster(L, h, 1.0, 0, 1, o) == N.VI_ERR_INVALID_INPUT and b"n_probe" in L.vi_last_error()
        assert cluster(L, h, 1.0, 2, 1, o, outputs=False) == N.VI_ERR_INVALID_INPUT and b"null pointer" in L.vi_last_error()
        # one output is enough to pass that check: the next one answers
        assert L.vi_indexer_cluster_radius(h, None, 1.0, 2, 1, None, None, C.byref(o.n)) == N.VI_ERR_INVALID_INPUT
        assert b"no index" in L.vi_last_error() and o.untouched()
    finally:
        L.vi_indexer_free(h)
