"""CPU: the entries of the C ABI for rebalancing an index (vi_rebalance_rule_init, vi_indexer_rebalance,
vi_indexer_last_rebalance_stats) exist in libvi_amd.so with the prototypes include/vi_amd.h documents, the ABI version is
still 2 (the change is additive), the ctypes mirrors have the header's fields and sizes, the defaults are the documented
ones, and every refusal that needs no index is VI_ERR_INVALID_INPUT with a message, not a crash.  (Loading the library
needs no GPU.)"""
import ctypes as C
import math
import os
import shutil
import subprocess

from vector_indexer_py import _native as N

from test_refine_abi_cpu import REFINE_FIELDS, header, new_handle, squeezed, struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64 = C.c_void_p, C.c_uint64

PROTOTYPES = {
    "vi_rebalance_rule_init": (None, [C.POINTER(N.RebalanceRuleC)]),
    "vi_indexer_rebalance": (C.c_int, [vp, C.POINTER(N.RebalanceRuleC), C.POINTER(u64)]),
    "vi_indexer_last_rebalance_stats": (C.c_int, [vp, C.POINTER(N.RebalanceStats)]),
}
DECLARATIONS = [
    "void vi_rebalance_rule_init(vi_rebalance_rule *r);",
    "vi_status vi_indexer_rebalance(vi_indexer *ix, const vi_rebalance_rule *rule, uint64_t *moved_out);",
    "vi_status vi_indexer_last_rebalance_stats(const vi_indexer *ix, vi_rebalance_stats *out);",
]
RULE_FIELDS = ["iters", "split_rounds", "split_factor", "receiver_max_len", "max_splits", "split_iters", "reserved0"]
SPLIT_FIELDS = ["pairs_planned", "splits_done", "splits_skipped", "inner_iterations", "split_bytes", "ms_split", "ms_split_kernels"]
CTYPE = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double}


def default_rule():
    r = N.RebalanceRuleC()
    N.lib().vi_rebalance_rule_init(C.byref(r))
    return r


def test_the_header_declares_the_entries():
    h = squeezed(header())
    for d in DECLARATIONS:
        assert d in h, d
    for phrase in ("len descending, index ascending", "len ascending, index ascending", "is a donor only", "lowest position among equals",
                   "a tie goes to side 0", "the pair is SKIPPED", "split_rounds == 0: the call IS vi_indexer_refine(iters)"):
        assert phrase in h, phrase


def test_the_structs_match_the_ctypes_mirrors():
    for name, cls, fields in (("vi_rebalance_rule", N.RebalanceRuleC, RULE_FIELDS),
                              ("vi_rebalance_stats", N.RebalanceStats, REFINE_FIELDS + SPLIT_FIELDS)):
        got = struct_fields(name)
        assert [n for _, n in got] == fields == [f for f, _ in cls._fields_], name
        assert [CTYPE[t] for t, _ in got] == [t for _, t in cls._fields_], name
    assert C.sizeof(N.RebalanceRuleC) == 48 and C.sizeof(N.RebalanceStats) == C.sizeof(N.RefineStats) + 48 == 136


def test_the_struct_sizes_are_the_c_compilers(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        return
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "vi_amd.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(vi_rebalance_rule), '
                   'sizeof(vi_rebalance_stats), sizeof(vi_refine_stats)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    done = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    out = subprocess.run([exe], capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(N.RebalanceRuleC), C.sizeof(N.RebalanceStats), C.sizeof(N.RefineStats)]


def test_abi_version_is_still_2_and_the_symbols_resolve():
    L = N.lib()
    assert L.vi_abi_version() == 2
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)
        assert (fn.restype, list(fn.argtypes)) == (res, args) == N.SIGNATURES[name], name


def test_the_defaults():
    r = N.RebalanceRuleC()
    C.memset(C.byref(r), 0xAB, C.sizeof(r))
    N.lib().vi_rebalance_rule_init(C.byref(r))
    assert [getattr(r, f) for f in RULE_FIELDS] == [1, 1, 2.0, 0, 0, 4, 0]
    N.lib().vi_rebalance_rule_init(None)      # a null rule is left alone
    import vector_indexer_py as vip
    p = vip.RebalanceRule()._native_rule()
    assert [getattr(p, f) for f in RULE_FIELDS] == [1, 1, 2.0, 0, 0, 4, 0]
    q = vip.RebalanceRule(iters=3, split_rounds=2, split_factor=1.5, receiver_max_len=7, max_splits=9, split_iters=11)._native_rule()
    assert [getattr(q, f) for f in RULE_FIELDS] == [3, 2, 1.5, 7, 9, 11, 0]


def test_refusals_that_need_no_index():
    L = N.lib()
    moved = u64(7)
    r = default_rule()
    assert L.vi_indexer_rebalance(None, C.byref(r), C.byref(moved)) == N.VI_ERR_INVALID_INPUT and moved.value == 0
    assert b"null" in L.vi_last_error()
    bs = N.RebalanceStats()
    assert L.vi_indexer_last_rebalance_stats(None, C.byref(bs)) == N.VI_ERR_INVALID_INPUT
    h = new_handle()
    try:
        assert L.vi_indexer_last_rebalance_stats(h, None) == N.VI_ERR_INVALID_INPUT and b"null" in L.vi_last_error()
        moved = u64(7)
        assert L.vi_indexer_rebalance(h, None, C.byref(moved)) == N.VI_ERR_INVALID_INPUT and moved.value == 0
        assert b"null rule" in L.vi_last_error()
        bad = [("iters", 0, b"at least one iteration"), ("split_rounds", 2, b"split_rounds"), ("split_factor", 0.99, b"split_factor"),
               ("split_factor", math.nan, b"split_factor"), ("split_factor", math.inf, b"split_factor"),
               ("split_factor", -2.0, b"split_factor"), ("split_iters", 0, b"split_iters"), ("split_iters", 65, b"split_iters"),
               ("reserved0", 1, b"reserved0")]
        for f, v, msg in bad:
            r = default_rule()
            setattr(r, f, v)
            moved = u64(7)
            assert L.vi_indexer_rebalance(h, C.byref(r), C.byref(moved)) == N.VI_ERR_INVALID_INPUT and moved.value == 0, (f, v)
            assert msg in L.vi_last_error(), (f, v, L.vi_last_error())
        # a valid rule on a handle that holds no index: refused before any device is asked for
        for f, v in (("iters", 1), ("iters", 5), ("split_iters", 64), ("split_iters", 1), ("split_factor", 1.0), ("split_rounds", 0)):
            r = default_rule()
            setattr(r, f, v)
            assert L.vi_indexer_rebalance(h, C.byref(r), None) == N.VI_ERR_INVALID_INPUT
            assert b"holds no index" in L.vi_last_error(), (f, v)
        assert L.vi_indexer_last_rebalance_stats(h, C.byref(bs)) == N.VI_OK
        assert all(getattr(bs, f) == 0 for f in REFINE_FIELDS + SPLIT_FIELDS)      # no rebalance has run on this handle
    finally:
        L.vi_indexer_free(h)


def test_python_layers_offer_the_calls():
    import vector_indexer_py as vip
    from vector_indexer_py.api import VectorIndexer
    from vector_indexer_py.harness import FaissStyleAdapter
    assert "RebalanceRule" in vip.__all__
    for cls, names in ((vip.VectorIndex, ("rebalance", "rebalance_stats")), (VectorIndexer, ("rebalance_lists",)),
                       (FaissStyleAdapter, ("rebalance", "imbalance_factor"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
