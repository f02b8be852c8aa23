"""Child process of test_exact_ip_seed_gpu.py::test_the_switch_skips_the_ladder_and_changes_no_row: VI_EXACT_IP_LADDER is
read from the environment, so the parent sets it for this process only.  Builds an index of the given rows, searches it
exactly by inner product and saves the rows it returned, the index's export and the ladder's level count.

usage: exact_ip_ladder_child.py work_dir in.npz out.npz"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vector-indexer_amd")]

import numpy as np  # noqa: E402

import vector_indexer_py as vip  # noqa: E402


def main():
    work, src, dst = sys.argv[1:4]
    data = np.load(src)
    idx = vip.build(data["X"], work, nlist=8, now_secs=1_700_000_000)
    ext, X, _, _ = idx.export()
    S, I, R = idx.search_exact_ip_sync(data["Q"], 10, with_ordinals=True)
    np.savez(dst, S=S, I=I, R=R, ext=ext, X=X, levels=idx.exact_ip_seed_stats()["levels"])


if __name__ == "__main__":
    main()
