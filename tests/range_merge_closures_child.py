"""Child process of test_range_merge_gpu.py::test_gpu_searcher_closures_with_in_process_ranks: drives the closures of
vector_indexer_py.distributed.gpu_searcher with `world` in-process ranks on one GPU.  torch initialises its HIP runtime
first (the order a multi-GPU worker has), which is why this is a process of its own.  The all-gathers are simulated: the
ranks' lims are stacked and the buffers pack_range_part makes are concatenated.

usage: range_merge_closures_child.py index_dir shards_dir dim world n_probe in.npz out.npz"""
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
    idx, sh, dim, world, n_probe, src, dst = sys.argv[1:8]
    dim, world, n_probe = int(dim), int(world), int(n_probe)
    inp = np.load(src)
    dev = torch.device("cuda", 0)
    xq = torch.from_numpy(inp["Q"]).to(dev)
    ranks = [vip.load(idx, sh, dim, rank=r, world_size=world) for r in range(world)]
    searchers = [VD.gpu_searcher(ix, 0) for ix in ranks]
    assert all(s.world == 1 for s in searchers)        # (no process group here: the exchange is simulated below)

    def merged_range(radius2, filters=None):
        locals_ = [s.local_range_search(xq, radius2, n_probe, **({} if filters is None else {"filter": f}))
                   for s, f in zip(searchers, filters or [None] * world)]
        lims_all = torch.stack([x[0] for x in locals_])
        cap = int(lims_all[:, -1].max().item())
        if cap == 0:
            return locals_[0]
        packed = torch.cat([VD.pack_range_part(cap, *x[1:]) for x in locals_]).view(world, VD.range_part_layout(cap)[2])
        return searchers[0].merge_range(lims_all, packed, cap)

    out = {}
    for name, r in zip(inp["names"], inp["radii"]):
        res = merged_range(float(r))
        for key, t in zip(("lims", "D", "I", "T"), res):
            out[f"{key}_{name}"] = t.cpu().numpy()
    window = [int(x) for x in inp["window"]]
    filters = [ix.filter_timestamps(*window) for ix in ranks]          # every rank's own filter from the same predicate
    r100 = float(inp["radii"][list(inp["names"]).index("r100")])
    for key, t in zip(("lims", "D", "I", "T"), merged_range(r100, filters)):
        out[f"{key}_f"] = t.cpu().numpy()
    # top-k with a filter through local_search and the existing merge
    parts = [s._local_search(xq, 10, n_probe, filter=f) for s, f in zip(searchers, filters)]
    D, I = searchers[0]._merge(*[torch.stack([p[c] for p in parts]) for c in range(3)])
    out["D_k"], out["I_k"] = D.cpu().numpy(), I.cpu().numpy()
    np.savez(dst, **out)


if __name__ == "__main__":
    main()
