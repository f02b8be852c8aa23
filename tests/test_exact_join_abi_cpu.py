"""CPU: the entries of the C ABI for the exact radius self-join (vi_indexer_cluster_radius_exact, host and device form,
vi_indexer_radius_graph_exact, vi_exact_join_last_stats) exist in libvi_amd.so with the prototypes include/vi_amd.h
documents, and the errors that need no device are errors with a message that leave no result.  (Loading the library
needs no GPU.)"""
import ctypes as C
import os

import pytest

import vector_indexer_py as vip
from test_exact_abi_cpu import new_handle
from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64, u32, f32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_float

PROTOTYPES = {
    "vi_indexer_cluster_radius_exact": (C.c_int, [vp, vp, f32, u32, vp, vp, C.POINTER(u64)]),
    "vi_indexer_cluster_radius_exact_device": (C.c_int, [vp, vp, f32, u32, vp, vp, C.POINTER(u64)]),
    "vi_indexer_radius_graph_exact": (C.c_int, [vp, vp, f32, u32, C.POINTER(N.ExactJoinOpts), C.POINTER(vp)]),
    "vi_exact_join_last_stats": (C.c_int, [C.POINTER(N.ExactJoinStats)]),
}
DECLARATIONS = [
    "typedef struct vi_exact_join_opts { uint64_t pool_cap; } vi_exact_join_opts;",
    "vi_status vi_indexer_cluster_radius_exact(const vi_indexer *ix, const vi_filter *f, float radius2, uint32_t min_pts, "
    "int64_t *labels_out, uint32_t *degree_out, uint64_t *n_clusters_out);",
    "vi_status vi_indexer_cluster_radius_exact_device(const vi_indexer *ix, const vi_filter *f, float radius2, uint32_t min_pts, "
    "int64_t *labels_dev, uint32_t *degree_dev, uint64_t *n_clusters_out);",
    "vi_status vi_indexer_radius_graph_exact(const vi_indexer *ix, const vi_filter *f, float radius2, uint32_t exclude_self, "
    "const vi_exact_join_opts *opts, vi_range_result **out);",
    "typedef struct vi_exact_join_stats { uint64_t rows, tiles, segments, sweeps; uint64_t survivors, pairs, hits, pool_cap, chunk_rows; "
    "float ms_resolve, ms_prepare, ms_sweep, ms_finish; } vi_exact_join_stats;",
    "vi_status vi_exact_join_last_stats(vi_exact_join_stats *out);",
    "the adjacency is now symmetric by construction",
    "removes the row's own SLOT from its row",
]


def test_the_symbols_resolve_and_the_header_declares_them_verbatim():
    L = N.lib()
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)      # AttributeError: not exported
        assert (fn.restype is res or fn.restype == res) and list(fn.argtypes) == args, name
        assert N.SIGNATURES[name] == (res, args), name
    flat = " ".join(open(os.path.join(ROOT, "include", "vi_amd.h")).read().replace(" * ", " ").split())
    for decl in DECLARATIONS:
        assert " ".join(decl.split()) in flat, decl
    assert C.sizeof(N.ExactJoinOpts) == 8 and C.sizeof(N.ExactJoinStats) == 9 * 8 + 4 * 4
    assert L.vi_exact_join_last_stats(None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()


@pytest.mark.parametrize("entry", ["cluster", "cluster_device", "graph"])
def test_bad_arguments_are_errors_before_any_device_work_and_leave_no_result(entry):
    L = N.lib()
    h = new_handle()
    labels, n = (C.c_int64 * 4)(5, 5, 5, 5), u64(7)

    def call(ix, radius2=1.0, outputs=True):
        if entry == "graph":
            res = vp(7)
            return L.vi_indexer_radius_graph_exact(ix, None, radius2, 1, None, C.byref(res) if outputs else None), res.value
        fn = L.vi_indexer_cluster_radius_exact_device if entry == "cluster_device" else L.vi_indexer_cluster_radius_exact
        return fn(ix, None, radius2, 1, labels if outputs else None, None, C.byref(n) if outputs else None), None

    try:
        for message, kw in {"null indexer": dict(ix=None), "NaN": dict(ix=h, radius2=float("nan")), "no index": dict(ix=h),
                            "is required": dict(ix=h, outputs=False)}.items():
            status, res = call(**kw)
            assert status == N.VI_ERR_INVALID_INPUT, message
            assert message.encode() in L.vi_last_error(), (message, L.vi_last_error())
            assert res == (7 if entry == "graph" and not kw.get("outputs", True) else None)
            assert list(labels) == [5, 5, 5, 5] and n.value == 7
    finally:
        L.vi_indexer_free(h)


def test_the_python_wrapper_rejects_unknown_options():
    idx = vip.VectorIndex(new_handle(), 8)
    with pytest.raises(TypeError, match="unknown exact-join options"):
        idx.radius_graph_exact(1.0, opts={"pool": 1})
    with pytest.raises(N.ViError, match="radius2 is NaN") as e:
        idx.cluster_radius_exact(float("nan"))
    assert e.value.kind == "InvalidInput"
