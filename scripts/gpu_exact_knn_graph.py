#!/usr/bin/env python3
"""Measure the exact k-NN graph on the bench index and write profiles/r33_exact_knn_graph.json.

On the benchmark's C2 shape (N = 1e6, D = 128, 8-bit data, 4096 lists; --n / --nlist shrink it) at k = 10 it records,
--repeats calls each, wall time (host clock around calls that end synchronised), min and max, of
  * knn_graph_exact_device;
  * the exact graph a caller could already get: export_device + search_exact_device over all rows in chunks of 65 536,
    k + 1 wide (the row itself is among its own neighbours);
  * the probed knn_graph_device at n_probe 32 (--probed-repeats calls), with its recall from VectorIndexer.knn_graph_recall;
and, from one more call of the new entry under VI_EXACT_TIMING, the phases, sweeps, survivors and candidates per row.
Needs an MI355X; nothing here falls back to the CPU."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vector-indexer_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--probed-repeats", type=int, default=2)
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r33_exact_knn_graph.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_exact_knn_graph.py needs an MI355X")
    import bench
    import vector_indexer_py as vip
    from vector_indexer_py.api import VectorIndexer, VectorIndexerConfig
    dev = torch.device("cuda", 0)

    def clock(fn):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) * 1e3, out

    def span(fn, repeats):
        fn()  # warm-up: code objects, workspace
        t = [clock(fn)[0] for _ in range(repeats)]
        return [min(t), max(t)]

    xb, _ = bench.make_dataset(args.n, args.d, 16, 1234, dev)
    k = args.k
    res = {"shape": {"n": args.n, "d": args.d, "nlist": args.nlist, "k": k}, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as work:
        index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000)
        N = index.num_vectors
        res["rows"] = N
        D = torch.empty((N, k), dtype=torch.float32, device=dev)
        I = torch.empty((N, k), dtype=torch.int64, device=dev)
        exact = lambda: index.knn_graph_exact_device(k, D.data_ptr(), I.data_ptr())  # noqa: E731
        res["knn_graph_exact"] = {"ms": span(exact, args.repeats)}
        os.environ["VI_EXACT_TIMING"] = "1"
        exact()
        st = index.exact_knn_stats()
        del os.environ["VI_EXACT_TIMING"]
        res["knn_graph_exact"].update({"sweeps": st["sweeps"], "tiles": st["tiles"], "segments": st["segments"], "seed_probe": st["seed_probe"],
                                       "survivors_per_row": st["survivors"] / N, "candidates_per_row": st["candidates"] / N,
                                       "unbounded_rows": st["unbounded_rows"], "pool_cap": st["pool_cap"], "chunk_rows": st["chunk_rows"],
                                       "phases_ms": {f: st[f] for f in ("ms_seed", "ms_prepare", "ms_sweep", "ms_finish")}})
        Dx = D.clone()

        rows = torch.empty((N, args.d), dtype=torch.float32, device=dev)     # the stored rows in list order
        D1 = torch.empty((65536, k + 1), dtype=torch.float32, device=dev)
        I1 = torch.empty((65536, k + 1), dtype=torch.int64, device=dev)
        Dc = torch.empty((N, k + 1), dtype=torch.float32, device=dev)

        def chunked():  # what a caller could do before: every ordered pair
            index.export_device(0, N, values_ptr=rows.data_ptr())
            for q0 in range(0, N, 65536):
                m = min(65536, N - q0)
                index.search_exact_device(rows[q0:q0 + m].data_ptr(), m, k + 1, D1.data_ptr(), I1.data_ptr())
                Dc[q0:q0 + m] = D1[:m]
        res["export_plus_search_exact_chunks"] = {"ms": span(chunked, args.repeats)}
        # the same k-th distances either way (row u's own slot is one of its k + 1 nearest at distance 0)
        res["kth_distances_equal"] = bool((Dc[:, k] == Dx[:, k - 1]).all().item())

        P = min(args.n_probe, index.num_centroids)
        probed = lambda: index.knn_graph_device(0, N, k, P, D.data_ptr(), I.data_ptr())  # noqa: E731
        res["probed"] = {"n_probe": P, "knn_graph_ms": span(probed, args.probed_repeats)}
        ix = VectorIndexer.load(VectorIndexerConfig.new(args.d).with_index_dir(os.path.join(work, "index")).with_shards_dir(os.path.join(work, "shards")))
        res["probed"]["recall"] = ix.knn_graph_recall(k, P)
        res["ratio_exact_to_chunks"] = res["knn_graph_exact"]["ms"][0] / res["export_plus_search_exact_chunks"]["ms"][0]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
