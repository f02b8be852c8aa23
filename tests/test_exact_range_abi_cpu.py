"""CPU: the entries of the C ABI for the exact (flat) radius search (vi_indexer_range_search_exact, host and device form,
vi_exact_range_opts_init, vi_exact_range_last_stats) exist in libvi_amd.so with the prototypes include/vi_amd.h documents,
the errors that need no device are errors with a message that leave no result, and the Python wrappers check their
arguments before they call.  (Loading the library needs no GPU.)"""
import ctypes as C
import os

import numpy as np
import pytest

import vector_indexer_py as vip
from test_exact_abi_cpu import new_handle
from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64, u32, f32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_float

PROTOTYPES = {
    "vi_exact_range_opts_init": (None, [C.POINTER(N.ExactRangeOpts)]),
    "vi_indexer_range_search_exact": (C.c_int, [vp, vp, C.POINTER(N.ExactRangeOpts), vp, u64, u32, f32, C.POINTER(vp)]),
    "vi_indexer_range_search_exact_device": (C.c_int, [vp, vp, C.POINTER(N.ExactRangeOpts), vp, u64, f32, C.POINTER(vp)]),
    "vi_exact_range_last_stats": (C.c_int, [C.POINTER(N.ExactRangeStats)]),
}
DECLARATIONS = [
    "typedef struct vi_exact_range_opts { const float *radii; uint64_t pool_cap; } vi_exact_range_opts;",
    "void vi_exact_range_opts_init(vi_exact_range_opts *opts);",
    "vi_status vi_indexer_range_search_exact(const vi_indexer *ix, const vi_filter *f, const vi_exact_range_opts *opts, "
    "const float *queries, uint64_t nq, uint32_t query_dim, float radius2, vi_range_result **out);",
    "vi_status vi_indexer_range_search_exact_device(const vi_indexer *ix, const vi_filter *f, const vi_exact_range_opts *opts, "
    "const float *queries_dev, uint64_t nq, float radius2, vi_range_result **out);",
    "typedef struct vi_exact_range_stats { uint64_t nq, query_tile, block_splits, chunks; uint64_t survivors, hits, sweeps, pool_cap; "
    "float ms_prepare, ms_sweep, ms_place, ms_sort, ms_output, ms_total; } vi_exact_range_stats;",
    "vi_status vi_exact_range_last_stats(vi_exact_range_stats *out);",
    "not meant for vi_range_merge_device",
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
    assert C.sizeof(N.ExactRangeOpts) == 16 and C.sizeof(N.ExactRangeStats) == 8 * 8 + 6 * 4
    o = N.ExactRangeOpts(7, 7)
    L.vi_exact_range_opts_init(C.byref(o))
    assert (o.radii, o.pool_cap) == (None, 0)
    L.vi_exact_range_opts_init(None)
    assert L.vi_exact_range_last_stats(None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()


@pytest.mark.parametrize("device", [False, True])
def test_bad_arguments_are_errors_before_any_device_work_and_leave_no_result(device):
    L = N.lib()
    h = new_handle()
    q = (f32 * 16)(*([1.0] * 16))
    radii = N.ExactRangeOpts(C.cast((f32 * 2)(1.0, 1.0), vp), 0)

    def call(ix, radius2=1.0, dim=8, queries=q, opts=None, out=True):
        res = vp(7)
        ref = C.byref(res) if out else None
        if device:
            return L.vi_indexer_range_search_exact_device(ix, None, opts, queries, 2, radius2, ref), res.value
        return L.vi_indexer_range_search_exact(ix, None, opts, queries, 2, dim, radius2, ref), res.value

    try:
        cases = {"out is required": dict(ix=h, out=False), "null indexer": dict(ix=None), "NaN": dict(ix=h, radius2=float("nan")),
                 "null pointer": dict(ix=h, queries=None), "no index": dict(ix=h),
                 "no index ": dict(ix=h, radius2=float("nan"), opts=C.byref(radii))}   # (per-query radii: the scalar is not read)
        if not device:
            cases["dimension"] = dict(ix=h, dim=9)
        for message, kw in cases.items():
            status, res = call(**kw)
            assert status == N.VI_ERR_INVALID_INPUT, message
            assert message.strip().encode() in L.vi_last_error(), (message, L.vi_last_error())
            assert res == (7 if not kw.get("out", True) else None)
    finally:
        L.vi_indexer_free(h)


def test_the_python_wrappers_check_their_arguments_first():
    idx = vip.VectorIndex(new_handle(), 8)
    with pytest.raises(RuntimeError, match="2-dimensional"):
        idx.range_search_exact_sync(np.zeros(8, dtype=np.float32), 1.0)
    with pytest.raises(RuntimeError, match="doesn't match index dimension"):
        idx.range_search_exact_sync(np.zeros((2, 9), dtype=np.float32), 1.0)
    with pytest.raises(RuntimeError, match="3 radii for 2 queries"):
        idx.range_search_exact_sync(np.zeros((2, 8), dtype=np.float32), 1.0, radii=[1.0, 2.0, 3.0])
    with pytest.raises(TypeError, match="unknown exact-range options"):
        idx.range_search_exact_sync(np.zeros((2, 8), dtype=np.float32), 1.0, opts={"pool": 1})
    with pytest.raises(N.ViError, match="radius2 is NaN") as e:
        idx.range_search_exact_sync(np.zeros((2, 8), dtype=np.float32), float("nan"))
    assert e.value.kind == "InvalidInput"
