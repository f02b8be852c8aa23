"""CPU: the ladder's report of the exact inner-product search (vi_exact_ip_seed_last_stats, vi_exact_ip_seed_stats) exists in
libvi_amd.so with the prototype and the struct include/vi_amd.h documents, refuses a NULL out, and reports zeros on a
thread that has searched nothing.  (Loading the library needs no GPU.)"""
import ctypes as C
import os
import threading

import vector_indexer_py as vip
from vector_indexer_py import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_resolves_and_the_header_declares_it_verbatim():
    L = N.lib()
    proto = (C.c_int, [C.POINTER(N.ExactIpSeedStats)])
    fn = L.vi_exact_ip_seed_last_stats      # AttributeError: not exported
    assert (fn.restype, list(fn.argtypes)) == proto == N.SIGNATURES["vi_exact_ip_seed_last_stats"]
    flat = " ".join(open(os.path.join(ROOT, "include", "vi_amd.h")).read().split())
    for decl in ["vi_status vi_exact_ip_seed_last_stats(vi_exact_ip_seed_stats *out);",
                 "typedef struct vi_exact_ip_seed_stats { uint64_t levels, ratio; uint64_t strides[8]; uint64_t level_survivors[8], "
                 "level_candidates[8]; uint64_t rows_tightened, rows_level_overflow; float ms_ladder; } vi_exact_ip_seed_stats;"]:
        assert decl in flat, decl
    assert C.sizeof(N.ExactIpSeedStats) == 8 * (2 + 3 * 8 + 2) + 8      # (the float, padded to the struct's alignment)
    assert C.sizeof(N.ExactOpts) == 16                                   # (vi_exact_opts did not grow)
    assert L.vi_exact_ip_seed_last_stats(None) == N.VI_ERR_INVALID_INPUT and b"null pointer" in L.vi_last_error()
    st, rc = N.ExactIpSeedStats(levels=7), []
    fresh = threading.Thread(target=lambda: rc.append(L.vi_exact_ip_seed_last_stats(C.byref(st))))
    fresh.start()      # (the stats are per thread, and this one may have searched in an earlier GPU test of the run)
    fresh.join()
    assert rc == [N.VI_OK] and st.levels == 0 and st.ms_ladder == 0.0
    assert callable(vip.VectorIndex.exact_ip_seed_stats)
