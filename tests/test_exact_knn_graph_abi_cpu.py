"""CPU: the entries of the C ABI for the exact k-NN graph (vi_indexer_knn_graph_exact, host and device form,
vi_exact_knn_opts_init, vi_exact_knn_last_stats) exist in libvi_amd.so with the prototypes include/vi_amd.h documents, and
the errors that need no device are errors with a message that write none of the outputs.  (Loading the library needs no
GPU.)"""
import ctypes as C
import os

import pytest

import vector_indexer_py as vip
from test_exact_abi_cpu import new_handle
from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32

PROTOTYPES = {
    "vi_exact_knn_opts_init": (None, [C.POINTER(N.ExactKnnOpts)]),
    "vi_indexer_knn_graph_exact": (C.c_int, [vp, vp, C.POINTER(N.ExactKnnOpts), u64, u32, vp, vp, vp, vp]),
    "vi_indexer_knn_graph_exact_device": (C.c_int, [vp, vp, C.POINTER(N.ExactKnnOpts), u64, u32, vp, vp, vp, vp]),
    "vi_exact_knn_last_stats": (C.c_int, [C.POINTER(N.ExactKnnStats)]),
}
DECLARATIONS = [
    "typedef struct vi_exact_knn_opts { uint64_t seed_probe; uint64_t pool_cap; } vi_exact_knn_opts;",
    "void vi_exact_knn_opts_init(vi_exact_knn_opts *opts);",
    "vi_status vi_indexer_knn_graph_exact(const vi_indexer *ix, const vi_filter *f, const vi_exact_knn_opts *opts, uint64_t k, "
    "uint32_t exclude_self, float *D, int64_t *I, uint64_t *ord, uint64_t *counts);",
    "vi_status vi_indexer_knn_graph_exact_device(const vi_indexer *ix, const vi_filter *f, const vi_exact_knn_opts *opts, uint64_t k, "
    "uint32_t exclude_self, float *D_dev, int64_t *I_dev, uint64_t *ord_dev, uint64_t *counts_dev);",
    "typedef struct vi_exact_knn_stats { uint64_t rows, k, seed_probe, tiles, segments, sweeps; "
    "uint64_t survivors, candidates, unbounded_rows, pool_cap, chunk_rows; float ms_seed, ms_prepare, ms_sweep, ms_finish; } vi_exact_knn_stats;",
    "vi_status vi_exact_knn_last_stats(vi_exact_knn_stats *out);",
    "the row's own SLOT is no candidate",
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
    assert C.sizeof(N.ExactKnnOpts) == 16 and C.sizeof(N.ExactKnnStats) == 11 * 8 + 4 * 4 and vip.ExactKnnOpts is N.ExactKnnOpts
    o = N.ExactKnnOpts(7, 7)
    L.vi_exact_knn_opts_init(C.byref(o))
    assert (o.seed_probe, o.pool_cap) == (0, 0)
    L.vi_exact_knn_opts_init(None)
    assert L.vi_exact_knn_last_stats(None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()


@pytest.mark.parametrize("entry", ["vi_indexer_knn_graph_exact", "vi_indexer_knn_graph_exact_device"])
def test_bad_arguments_are_errors_before_any_device_work_and_write_nothing(entry):
    L = N.lib()
    fn, h = getattr(L, entry), new_handle()
    D, I = (C.c_float * 4)(5, 5, 5, 5), (C.c_int64 * 4)(5, 5, 5, 5)
    try:
        for message, (ix, k, outputs) in {"null indexer": (None, 1, True), "k must be in 1..128": (h, 0, True), "not 129": (h, 129, True),
                                          "D and I are required": (h, 1, False), "no index": (h, 1, True)}.items():
            assert fn(ix, None, None, k, 1, D if outputs else None, I if outputs else None, None, None) == N.VI_ERR_INVALID_INPUT, message
            assert message.encode() in L.vi_last_error(), (message, L.vi_last_error())
            assert list(D) == [5, 5, 5, 5] and list(I) == [5, 5, 5, 5]
        st = N.ExactKnnStats()
        assert L.vi_exact_knn_last_stats(C.byref(st)) == N.VI_OK and all(getattr(st, f) == 0 for f, _ in st._fields_)
    finally:
        L.vi_indexer_free(h)


def test_the_python_wrapper_rejects_unknown_options():
    idx = vip.VectorIndex(new_handle(), 8)
    with pytest.raises(TypeError, match="unknown exact-knn options"):
        idx.knn_graph_exact(1, opts={"pool": 1})
