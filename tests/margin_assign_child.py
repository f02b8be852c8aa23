"""Child process of test_rank_margin_gpu.py::test_assign_f32_first_tier_in_a_fresh_process: the exact assign of every
k-means case of margin_cases.py under the environment the parent gives it.  VI_ASSIGN_BF16 is read once per process
(assign_mfma.hip), so the f32 MFMA first tier (VI_ASSIGN_BF16=0) cannot be chosen inside a pytest process that has already
assigned.  The cases are deterministic: the parent builds the same ones and compares the labels with the oracle's.

usage: margin_assign_child.py out.npz"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vector-indexer_amd"), os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import margin_cases as M  # noqa: E402
from hiprt import Hip  # noqa: E402
from vector_indexer_py import _native as N  # noqa: E402

CASES = {"H-D4": lambda: M.assign_case(4), "H-D16": lambda: M.assign_case(16), "H-D4-n3600": lambda: M.assign_case(4, 3600, 2400),
         "H-D16-n3600": lambda: M.assign_case(16, 3600, 2400), "H-sweep-D16": M.assign_sweep_case}


def assign_with_stats(hip, X, Cn):
    """(labels, vi_assign_stats) of the exact assign through the device entry"""
    n, d = X.shape
    Xd, Cd, lab = hip.upload(X), hip.upload(Cn), hip.alloc(n * 4)
    st = N.AssignStats()
    N.check(N.lib().vi_assign_device(0, Xd, n, d, Cd, Cn.shape[0], 42, N.VI_ASSIGN_EXACT, lab, C.byref(st)))
    return hip.download(lab, (n,), np.uint32).astype(np.uint64), st


def main():
    out = {}
    hip = Hip()
    try:
        for name, make in CASES.items():
            h = make()
            assert h["name"] == name
            labels, st = assign_with_stats(hip, h["X"], h["centroids"])
            out[name] = labels
            out[name + "/stats"] = np.array([st.used_mfma, st.tier1_rows, st.ambiguous_rows], dtype=np.uint64)
    finally:
        hip.close()
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
