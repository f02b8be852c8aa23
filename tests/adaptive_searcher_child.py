"""Child process of test_adaptive_probe_gpu.py::test_gpu_searcher_with_a_rule: drives distributed.gpu_searcher(...).search(rule=)
— probe_device, prune_probes_device, search_probed_device behind one call — on an unpartitioned handle (world 1) and, through
the closures, on two in-process ranks whose results its merge joins.  torch initialises its HIP runtime first (the order a
multi-GPU worker has), which is why this is a process of its own.

usage: adaptive_searcher_child.py index_dir shards_dir dim k n_probe ratio2 in.npz out.npz"""
import os
import sys

import torch

torch.cuda.init()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vector-indexer_amd")]

import numpy as np  # noqa: E402

import vector_indexer_py as vip  # noqa: E402
from vector_indexer_py import distributed as VD  # noqa: E402


def main():
    idx, sh, dim, k, n_probe, ratio2, src, dst = sys.argv[1:9]
    dim, k, n_probe = int(dim), int(k), int(n_probe)
    dev = torch.device("cuda", 0)
    xq = torch.from_numpy(np.load(src)["Q"]).to(dev)
    rule = vip.ProbeRule(ratio2=float(ratio2))
    out = {}
    whole = VD.gpu_searcher(vip.load(idx, sh, dim), 0)
    assert whole.world == 1
    D, I = whole.search(xq, k, n_probe, rule=rule)
    out["D"], out["I"] = D.cpu().numpy(), I.cpu().numpy()
    D, I = whole.search(xq, k, n_probe)                     # (and without a rule: the call as it was)
    out["D_plain"], out["I_plain"] = D.cpu().numpy(), I.cpu().numpy()
    ranks = [VD.gpu_searcher(vip.load(idx, sh, dim, rank=r, world_size=2), 0) for r in range(2)]
    parts = [s._local_search(xq, k, n_probe, rule=rule) for s in ranks]
    D, I = ranks[0]._merge(*[torch.stack([p[c] for p in parts]) for c in range(3)])
    out["D_ranks"], out["I_ranks"] = D.cpu().numpy(), I.cpu().numpy()
    np.savez(dst, **out)


if __name__ == "__main__":
    main()
