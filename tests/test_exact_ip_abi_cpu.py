"""CPU: the entries of the C ABI for the exact (flat) inner-product search (vi_indexer_search_exact_ip, host and device
form, vi_exact_ip_last_stats) exist in libvi_amd.so with the prototypes include/vi_amd.h documents, the errors that need
no device are errors with a message that write none of the outputs, and the Python wrappers check the shapes of their
arguments before they call.  (Loading the library needs no GPU.)"""
import ctypes as C
import os

import numpy as np
import pytest

import vector_indexer_py as vip
from vector_indexer_py import _native as N
from vector_indexer_py import api, harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64, u32, f32, i64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_int64

PROTOTYPES = {
    "vi_indexer_search_exact_ip": (C.c_int, [vp, vp, C.POINTER(N.ExactOpts), vp, u64, u32, u64, vp, vp, vp, vp]),
    "vi_indexer_search_exact_ip_device": (C.c_int, [vp, vp, C.POINTER(N.ExactOpts), vp, u64, u64, vp, vp, vp, vp]),
    "vi_exact_ip_last_stats": (C.c_int, [C.POINTER(N.ExactStats)]),
}
DECLARATIONS = [
    "vi_status vi_indexer_search_exact_ip(const vi_indexer *ix, const vi_filter *f, const vi_exact_opts *opts, const float *queries, "
    "uint64_t nq, uint32_t query_dim, uint64_t k, float *S, int64_t *I, uint64_t *ord, uint64_t *counts);",
    "vi_status vi_indexer_search_exact_ip_device(const vi_indexer *ix, const vi_filter *f, const vi_exact_opts *opts, "
    "const float *queries_dev, uint64_t nq, uint64_t k, float *S_dev, int64_t *I_dev, uint64_t *ord_dev, uint64_t *counts_dev);",
    "vi_status vi_exact_ip_last_stats(vi_exact_stats *out);",
    "s = 0.0f; for i in 0..dimension: s = s + q[i] * v[i]",
    "equal scores go to the LOWER list-order ORDINAL",
    "padded with -inf / -1 / UINT64_MAX",
]


def new_handle(dim=8):
    """a handle from vi_indexer_new: it holds no index"""
    cfg = N.Config()
    N.lib().vi_config_init(C.byref(cfg), dim)
    h = vp()
    N.check(N.lib().vi_indexer_new(C.byref(cfg), C.byref(h)))
    return h


def test_the_symbols_resolve_and_the_header_declares_them_verbatim():
    L = N.lib()
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)      # AttributeError: not exported
        assert fn.restype == res and list(fn.argtypes) == args, name
        assert N.SIGNATURES[name] == (res, args), name
    flat = " ".join(open(os.path.join(ROOT, "include", "vi_amd.h")).read().split())
    for decl in DECLARATIONS:
        assert " ".join(decl.split()) in flat, decl
    assert L.vi_exact_ip_last_stats(None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()
    assert L.vi_exact_ip_last_stats(C.byref(N.ExactStats())) == N.VI_OK
    for owner, name in [(vip.VectorIndex, "search_exact_ip_sync"), (vip.VectorIndex, "search_exact_ip_device"),
                        (vip.VectorIndex, "exact_ip_stats"), (api.VectorIndexer, "search_exact_ip"),
                        (harness.FaissStyleAdapter, "exact_ip_search")]:
        assert callable(getattr(owner, name)), name


@pytest.mark.parametrize("device", [False, True])
def test_bad_arguments_are_errors_before_any_device_work_and_write_nothing(device):
    L = N.lib()
    h = new_handle()
    q = (f32 * 16)(*([1.0] * 16))
    S, I, R, n = (f32 * 4)(7, 7, 7, 7), (i64 * 4)(7, 7, 7, 7), (u64 * 4)(7, 7, 7, 7), (u64 * 2)(7, 7)

    def call(ix, k, dim=8, queries=q, S=S, I=I):
        if device:
            return L.vi_indexer_search_exact_ip_device(ix, None, None, queries, 2, k, S, I, R, n)
        return L.vi_indexer_search_exact_ip(ix, None, None, queries, 2, dim, k, S, I, R, n)

    try:
        cases = {"null indexer": (None, 2), "k": (h, 0), "in 1..128": (h, 129), "no index": (h, 2)}
        cases.update({"null pointer": (h, 2, 8, None)} if device else {"dimension": (h, 2, 9), "null pointer": (h, 2, 8, q, None)})
        for message, args in cases.items():
            assert call(*args) == N.VI_ERR_INVALID_INPUT, message
            assert message.encode() in L.vi_last_error(), (message, L.vi_last_error())
            assert list(S) == [7] * 4 and list(I) == [7] * 4 and list(R) == [7] * 4 and list(n) == [7] * 2
    finally:
        L.vi_indexer_free(h)


def test_the_python_wrappers_check_their_arguments_first():
    idx = vip.VectorIndex(new_handle(), 8)
    with pytest.raises(RuntimeError, match="2-dimensional"):
        idx.search_exact_ip_sync(np.zeros(8, dtype=np.float32), 3)
    with pytest.raises(RuntimeError, match="doesn't match index dimension"):
        idx.search_exact_ip_sync(np.zeros((2, 9), dtype=np.float32), 3)
    with pytest.raises(TypeError, match="unknown exact-search options"):
        idx.search_exact_ip_sync(np.zeros((2, 8), dtype=np.float32), 3, opts={"seed": 1})
    with pytest.raises(N.ViError, match="in 1..128") as e:
        idx.search_exact_ip_sync(np.zeros((2, 8), dtype=np.float32), 129)
    assert e.value.kind == "InvalidInput"
