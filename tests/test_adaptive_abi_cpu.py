"""CPU: the entries of the C ABI for adaptive probing (vi_indexer_prune_probes_device, vi_indexer_search_adaptive, its
device form, and vi_prune_last_stats) exist in libvi_amd.so with the prototypes include/vi_amd.h documents, and the errors
that need no device are VI_ERR_INVALID_INPUT with a message that write none of the outputs, not crashes.  (Loading the
library needs no GPU.)"""
import ctypes as C
import os
import threading

from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64, u32, f32, i64 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_float, C.c_int64
RULE = C.POINTER(N.ProbeRuleC)

# name -> (return type, argument types), as declared in include/vi_amd.h
PROTOTYPES = {
    "vi_indexer_prune_probes_device": (C.c_int, [vp, vp, u64, u64, vp, vp, RULE, vp]),
    "vi_indexer_search_adaptive": (C.c_int, [vp, vp, RULE, vp, u64, u32, u64, u64, vp, vp, vp, vp, vp, C.POINTER(u64)]),
    "vi_indexer_search_adaptive_device": (C.c_int, [vp, vp, RULE, vp, u64, u64, u64, vp, vp, vp, vp]),
    "vi_prune_last_stats": (C.c_int, [C.POINTER(u64), C.POINTER(u64), C.POINTER(f32)]),
}
DECLARATIONS = [
    "typedef struct vi_probe_rule { uint32_t min_probe; /* 0 => 1 */ float ratio2; /* 0 = off; else finite and >= 1 */ "
    "uint64_t max_codes; /* 0 = off */ const uint32_t *n_probe_q; /* NULL = off; nq entries, host memory for the host entry, "
    "device for _device */ } vi_probe_rule;",
    "vi_status vi_indexer_prune_probes_device(const vi_indexer *ix, const float *queries_dev, uint64_t nq, uint64_t n_probe_eff, "
    "uint32_t *probes_dev, uint32_t *order_dev, const vi_probe_rule *rule, uint32_t *n_kept_dev);",
    "vi_status vi_indexer_search_adaptive(const vi_indexer *ix, const vi_filter *f, const vi_probe_rule *rule, const float *queries, "
    "uint64_t nq, uint32_t query_dim, uint64_t k, uint64_t n_probe, float *D, int64_t *I, float *V, uint64_t *counts, "
    "uint32_t *n_probed, uint64_t *k_out);",
    "vi_status vi_indexer_search_adaptive_device(const vi_indexer *ix, const vi_filter *f, const vi_probe_rule *rule, "
    "const float *queries_dev, uint64_t nq, uint64_t k, uint64_t n_probe, float *D_dev, int64_t *I_dev, uint64_t *tie_dev, "
    "uint32_t *n_probed_dev);",
    "vi_status vi_prune_last_stats(uint64_t *probes_in, uint64_t *probes_kept, float *ms_prune);",
]
DIM = 8


def new_handle(dim=DIM, world_size=0, rank=0):
    """a handle from vi_indexer_new: it holds no index"""
    cfg = N.Config()
    N.lib().vi_config_init(C.byref(cfg), dim)
    cfg.world_size, cfg.rank = world_size, rank
    h = vp()
    N.check(N.lib().vi_indexer_new(C.byref(cfg), C.byref(h)))
    return h


def rule(min_probe=0, ratio2=0.0, max_codes=0):
    return N.ProbeRuleC(min_probe, ratio2, max_codes, None)


class Out:
    """the outputs of the host entry (and stand-ins for the device entries' pointers, which no failing call may follow)
    with a pattern that shows any write"""

    def __init__(self):
        self.q = (f32 * (2 * DIM))(*([0.5] * (2 * DIM)))
        self.D, self.I, self.V = (f32 * 6)(*([7.0] * 6)), (i64 * 6)(*([7] * 6)), (f32 * (6 * DIM))(*([7.0] * (6 * DIM)))
        self.counts, self.probed, self.kout = (u64 * 2)(7, 7), (u32 * 2)(7, 7), u64(7)
        self.probes, self.order = (u32 * 8)(*([7] * 8)), (u32 * 8)(*([7] * 8))

    def untouched(self):
        return (list(self.D) == [7.0] * 6 and list(self.I) == [7] * 6 and list(self.V) == [7.0] * (6 * DIM)
                and list(self.counts) == [7, 7] and list(self.probed) == [7, 7] and self.kout.value == 7
                and list(self.probes) == [7] * 8 and list(self.order) == [7] * 8)


def host(L, h, r, o, k=3, n_probe=4, dim=DIM, flt=None):
    return L.vi_indexer_search_adaptive(h, flt, C.byref(r) if r is not None else None, o.q, 2, dim, k, n_probe, o.D, o.I, o.V, o.counts,
                                        o.probed, C.byref(o.kout))


def device(L, h, r, o, k=3, n_probe=4, flt=None):
    return L.vi_indexer_search_adaptive_device(h, flt, C.byref(r) if r is not None else None, o.q, 2, k, n_probe, o.D, o.I, None, o.probed)


def prune(L, h, r, o, n_probe=4):
    return L.vi_indexer_prune_probes_device(h, o.q, 2, n_probe, o.probes, o.order, C.byref(r) if r is not None else None, o.probed)


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


def test_the_rule_structure_is_the_headers():
    assert C.sizeof(N.ProbeRuleC) == 24
    assert [(n, t) for n, t in N.ProbeRuleC._fields_] == [("min_probe", u32), ("ratio2", f32), ("max_codes", u64), ("n_probe_q", vp)]
    assert N.ProbeRuleC.ratio2.offset == 4 and N.ProbeRuleC.max_codes.offset == 8 and N.ProbeRuleC.n_probe_q.offset == 16
    import vector_indexer_py as vip
    r, keep = vip.ProbeRule()._native_rule(5, device=False)
    assert (r.min_probe, r.ratio2, r.max_codes, r.n_probe_q, keep) == (1, 0.0, 0, None, None)
    r, keep = vip.ProbeRule(2, 1.5, 1000, [3, 1, 2])._native_rule(3, device=False)
    assert (r.min_probe, r.ratio2, r.max_codes) == (2, 1.5, 1000) and r.n_probe_q == keep.ctypes.data and keep.tolist() == [3, 1, 2]


def test_prune_stats_read_zeros_on_a_fresh_thread():
    L = N.lib()
    assert L.vi_prune_last_stats(None, None, None) == N.VI_ERR_INVALID_INPUT and L.vi_last_error()
    a, b, ms = u64(99), u64(99), f32(99.0)

    def fresh():        # a thread that has pruned nothing reads zeros: the figures are the calling thread's own
        assert L.vi_prune_last_stats(C.byref(a), C.byref(b), C.byref(ms)) == N.VI_OK

    t = threading.Thread(target=fresh)
    t.start()
    t.join()
    assert (a.value, b.value, ms.value) == (0, 0, 0.0)
    a.value = 99
    assert L.vi_prune_last_stats(C.byref(a), None, None) == N.VI_OK     # any one pointer is enough


def test_null_indexer_and_null_rule_are_errors_with_a_message():
    L = N.lib()
    o = Out()
    h = new_handle()
    try:
        for call in (host, device, prune):
            assert call(L, None, rule(), o) == N.VI_ERR_INVALID_INPUT, call.__name__
            assert L.vi_last_error() and o.untouched(), call.__name__
            assert call(L, h, None, o) == N.VI_ERR_INVALID_INPUT, call.__name__
            assert b"rule" in L.vi_last_error() and o.untouched(), call.__name__
    finally:
        L.vi_indexer_free(h)


def test_bad_arguments_are_errors_before_any_device_work_and_write_nothing():
    L = N.lib()
    h = new_handle()
    try:
        o = Out()
        nan, inf = float("nan"), float("inf")
        for call in (host, device, prune):
            name = call.__name__
            assert call(L, h, rule(), o) == N.VI_ERR_INVALID_INPUT, name               # a handle with no index
            assert b"no index" in L.vi_last_error() and o.untouched(), name
            for bad in (nan, inf, -inf, -1.0, 0.5, 0.999999, 1e-30):
                assert call(L, h, rule(ratio2=bad), o) == N.VI_ERR_INVALID_INPUT, (name, bad)
                assert b"ratio2" in L.vi_last_error() and o.untouched(), (name, bad)
            assert call(L, h, rule(), o, n_probe=0) == N.VI_ERR_INVALID_INPUT, name
            assert b"n_probe" in L.vi_last_error() and o.untouched(), name
        for call in (host, device):
            assert call(L, h, rule(), o, k=0) == N.VI_ERR_INVALID_INPUT, call.__name__
            assert b"k and n_probe" in L.vi_last_error() and o.untouched(), call.__name__
        # a legal ratio passes that check: the next one answers
        for ok in (0.0, 1.0, 2.5, 3.0e38):
            assert host(L, h, rule(ratio2=ok), o) == N.VI_ERR_INVALID_INPUT and b"no index" in L.vi_last_error()
        assert o.untouched()
    finally:
        L.vi_indexer_free(h)


def test_dimension_filter_and_partition_errors_answer_before_the_handles_state():
    """a query_dim mismatch, a filter that is not this index's (no index: every filter is foreign; it is never followed)
    and max_codes on a handle configured as one rank of two"""
    L = N.lib()
    h, part = new_handle(), new_handle(world_size=2, rank=1)
    try:
        o = Out()
        assert host(L, h, rule(), o, dim=DIM + 1) == N.VI_ERR_INVALID_INPUT
        assert b"dimension" in L.vi_last_error() and o.untouched()
        fake = (u64 * 64)()
        for call in (host, device):
            assert call(L, h, rule(), o, flt=C.cast(fake, vp)) == N.VI_ERR_INVALID_INPUT, call.__name__
            assert b"filter" in L.vi_last_error() and o.untouched(), call.__name__
        for call in (host, device, prune):
            assert call(L, part, rule(max_codes=1000), o) == N.VI_ERR_INVALID_INPUT, call.__name__
            assert b"max_codes" in L.vi_last_error() and o.untouched(), call.__name__
            assert call(L, part, rule(ratio2=2.0), o) == N.VI_ERR_INVALID_INPUT, call.__name__    # the ratio is no such error
            assert b"no index" in L.vi_last_error() and o.untouched(), call.__name__
    finally:
        L.vi_indexer_free(h)
        L.vi_indexer_free(part)

