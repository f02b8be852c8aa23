"""CPU: the entries of the C ABI for refining an index (vi_indexer_refine, vi_indexer_last_refine_stats,
vi_indexer_list_stats) exist in libvi_amd.so with the prototypes include/vi_amd.h documents, the ABI version is still 2, and
the errors that need no device are VI_ERR_INVALID_INPUT with a message, not crashes.  (Loading the library needs no GPU.)"""
import ctypes as C
import os
import re

from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp, u64 = C.c_void_p, C.c_uint64

PROTOTYPES = {
    "vi_indexer_refine": (C.c_int, [vp, u64, C.POINTER(u64)]),
    "vi_indexer_last_refine_stats": (C.c_int, [vp, C.POINTER(N.RefineStats)]),
    "vi_indexer_list_stats": (C.c_int, [vp, C.POINTER(N.ListStats)]),
}
DECLARATIONS = [
    "vi_status vi_indexer_refine(vi_indexer *ix, uint64_t iters, uint64_t *moved_out);",
    "vi_status vi_indexer_last_refine_stats(const vi_indexer *ix, vi_refine_stats *out);",
    "vi_status vi_indexer_list_stats(const vi_indexer *ix, vi_list_stats *out);",
]
REFINE_FIELDS = ["iterations_run", "moved", "lists_emptied", "shards_rewritten", "bytes_written", "means_bytes", "rehome_bytes",
                 "ms_total", "ms_means", "ms_label", "ms_rehome", "ms_images", "ms_files", "ms_means_kernel", "ms_rehome_kernel"]
LIST_FIELDS = ["lists", "empty_lists", "min_len", "max_len", "mean_len", "imbalance"]


def header():
    return open(os.path.join(ROOT, "include", "vi_amd.h")).read()


def squeezed(text):
    return re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", text))   # (without the leaders of comment lines)


def new_handle(dim=8, world_size=0):
    """a handle from vi_indexer_new: it holds no index"""
    cfg = N.Config()
    N.lib().vi_config_init(C.byref(cfg), dim)
    cfg.world_size = world_size
    h = vp()
    N.check(N.lib().vi_indexer_new(C.byref(cfg), C.byref(h)))
    return h


def test_the_header_declares_the_entries():
    h = squeezed(header())
    for d in DECLARATIONS:
        assert d in h, d


def struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            out += [(typ, n.strip()) for n in names.split(",")]
    return out


def test_the_structs_match_the_ctypes_mirrors():
    ctype = {"uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
    for name, cls, fields in (("vi_refine_stats", N.RefineStats, REFINE_FIELDS), ("vi_list_stats", N.ListStats, LIST_FIELDS)):
        got = struct_fields(name)
        assert [n for _, n in got] == fields == [f for f, _ in cls._fields_], name
        assert [ctype[t] for t, _ in got] == [t for _, t in cls._fields_], name


def test_the_contract_is_in_the_header():
    h = squeezed(header())
    for phrase in ("update_centroids_parallel", "keeps C[l] bit for bit", "deliberate deviation", "lowest list index among equal distances",
                   "index.bin last", "mixes old and new files", "iters == 0"):
        assert phrase in h, phrase


def test_abi_version_is_still_2_and_the_symbols_resolve():
    L = N.lib()
    assert L.vi_abi_version() == 2
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(L, name)
        assert (fn.restype, list(fn.argtypes)) == (res, args) == N.SIGNATURES[name], name


def test_null_handle_and_null_outputs_are_refused():
    L = N.lib()
    moved = u64(7)
    assert L.vi_indexer_refine(None, 1, C.byref(moved)) == N.VI_ERR_INVALID_INPUT and moved.value == 0
    assert b"null" in L.vi_last_error()
    assert L.vi_indexer_refine(None, 0, None) == N.VI_ERR_INVALID_INPUT
    rs, ls = N.RefineStats(), N.ListStats()
    assert L.vi_indexer_last_refine_stats(None, C.byref(rs)) == N.VI_ERR_INVALID_INPUT
    assert L.vi_indexer_list_stats(None, C.byref(ls)) == N.VI_ERR_INVALID_INPUT
    h = new_handle()
    try:
        assert L.vi_indexer_last_refine_stats(h, None) == N.VI_ERR_INVALID_INPUT and b"null" in L.vi_last_error()
        assert L.vi_indexer_list_stats(h, None) == N.VI_ERR_INVALID_INPUT and b"null" in L.vi_last_error()
        # a handle that holds no index: refused, with or without iterations, before any device is asked for
        for iters in (0, 1, 3):
            moved = u64(7)
            assert L.vi_indexer_refine(h, iters, C.byref(moved)) == N.VI_ERR_INVALID_INPUT and moved.value == 0
            assert b"holds no index" in L.vi_last_error()
        assert L.vi_indexer_refine(h, 1, None) == N.VI_ERR_INVALID_INPUT
        assert L.vi_indexer_list_stats(h, C.byref(ls)) == N.VI_ERR_INVALID_INPUT and b"holds no index" in L.vi_last_error()
        assert L.vi_indexer_last_refine_stats(h, C.byref(rs)) == N.VI_OK
        assert all(getattr(rs, f) == 0 for f in REFINE_FIELDS)      # no refine has run on this handle
    finally:
        L.vi_indexer_free(h)


def test_python_layers_offer_the_calls():
    import vector_indexer_py as vip
    from vector_indexer_py.api import VectorIndexer
    from vector_indexer_py.harness import FaissStyleAdapter
    for cls, names in ((vip.VectorIndex, ("refine", "refine_stats", "list_stats")), (VectorIndexer, ("refine_lists",)),
                       (FaissStyleAdapter, ("imbalance_factor",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
