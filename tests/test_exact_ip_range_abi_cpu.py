"""CPU: the entries of the C ABI for the exact (flat) inner-product threshold search (vi_indexer_range_search_exact_ip, host
and device form, vi_exact_ip_range_opts_init, vi_exact_ip_range_last_stats) exist in libvi_amd.so with the prototypes
include/vi_amd.h documents, the header names the contract's points, and the errors that need no device are errors with a
message that leave no result.  (Loading the library needs no GPU.)"""
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
    "vi_exact_ip_range_opts_init": (None, [C.POINTER(N.ExactIpRangeOpts)]),
    "vi_indexer_range_search_exact_ip": (C.c_int, [vp, vp, C.POINTER(N.ExactIpRangeOpts), vp, u64, u32, f32, C.POINTER(vp)]),
    "vi_indexer_range_search_exact_ip_device": (C.c_int, [vp, vp, C.POINTER(N.ExactIpRangeOpts), vp, u64, f32, C.POINTER(vp)]),
    "vi_exact_ip_range_last_stats": (C.c_int, [C.POINTER(N.ExactRangeStats)]),
}
HEADER = [
    "typedef struct vi_exact_ip_range_opts { const float *min_scores; uint64_t pool_cap; } vi_exact_ip_range_opts;",
    "void vi_exact_ip_range_opts_init(vi_exact_ip_range_opts *opts);",
    "vi_status vi_indexer_range_search_exact_ip(const vi_indexer *ix, const vi_filter *f, const vi_exact_ip_range_opts *opts, "
    "const float *queries, uint64_t nq, uint32_t query_dim, float min_score, vi_range_result **out);",
    "vi_status vi_indexer_range_search_exact_ip_device(const vi_indexer *ix, const vi_filter *f, const vi_exact_ip_range_opts *opts, "
    "const float *queries_dev, uint64_t nq, float min_score, vi_range_result **out);",
    "vi_status vi_exact_ip_range_last_stats(vi_exact_range_stats *out);",
    "s == min_score is inside", "keeps s > thresh, strictly", "fails >= and is never a hit", "score descending",
    "D carries the scores", "not meant for vi_range_merge_device", "min_score: NaN: VI_ERR_INVALID_INPUT; -inf: every admitted record",
    "+inf included, is compared as it is", "A NaN entry gives that query an empty row", "0 = max(2^22, 256 per query)",
    "the pool grows to the count and the sweep runs once more", "chunks of 65536",
]


def test_the_symbols_resolve_and_the_header_states_the_contract():
    L = N.lib()
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)      # AttributeError: not exported
        assert (fn.restype is res or fn.restype == res) and list(fn.argtypes) == args, name
        assert N.SIGNATURES[name] == (res, args), name
    flat = " ".join(open(os.path.join(ROOT, "include", "vi_amd.h")).read().replace(" * ", " ").split())
    for text in HEADER:
        assert " ".join(text.split()) in flat, text
    assert C.sizeof(N.ExactIpRangeOpts) == 16
    o = N.ExactIpRangeOpts(7, 7)
    L.vi_exact_ip_range_opts_init(C.byref(o))
    assert (o.min_scores, o.pool_cap) == (None, 0)
    L.vi_exact_ip_range_opts_init(None)
    assert L.vi_exact_ip_range_last_stats(None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()


@pytest.mark.parametrize("device", [False, True])
def test_bad_arguments_are_errors_before_any_device_work_and_leave_no_result(device):
    L = N.lib()
    h = new_handle()
    q = (f32 * 16)(*([1.0] * 16))
    per_query = N.ExactIpRangeOpts(C.cast((f32 * 2)(1.0, 1.0), vp), 0)

    def call(ix, min_score=1.0, dim=8, queries=q, opts=None, out=True):
        res = vp(7)
        ref = C.byref(res) if out else None
        if device:
            return L.vi_indexer_range_search_exact_ip_device(ix, None, opts, queries, 2, min_score, ref), res.value
        return L.vi_indexer_range_search_exact_ip(ix, None, opts, queries, 2, dim, min_score, ref), res.value

    try:
        cases = {"out is required": dict(ix=h, out=False), "null indexer": dict(ix=None), "min_score is NaN": dict(ix=h, min_score=float("nan")),
                 "null pointer": dict(ix=h, queries=None), "no index": dict(ix=h), "no index ": dict(ix=h, min_score=float("-inf")),
                 "no index  ": dict(ix=h, min_score=float("nan"), opts=C.byref(per_query))}   # (per-query: the scalar is not read)
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
        idx.range_search_exact_ip_sync(np.zeros(8, dtype=np.float32), 1.0)
    with pytest.raises(RuntimeError, match="3 min_scores for 2 queries"):
        idx.range_search_exact_ip_sync(np.zeros((2, 8), dtype=np.float32), 1.0, min_scores=[1.0, 2.0, 3.0])
    with pytest.raises(TypeError, match="unknown exact-ip-range options"):
        idx.range_search_exact_ip_sync(np.zeros((2, 8), dtype=np.float32), 1.0, opts={"pool": 1})
    with pytest.raises(N.ViError, match="min_score is NaN") as e:
        idx.range_search_exact_ip_sync(np.zeros((2, 8), dtype=np.float32), float("nan"))
    assert e.value.kind == "InvalidInput"
