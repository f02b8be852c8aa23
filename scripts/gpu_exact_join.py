#!/usr/bin/env python3
"""Measure the exact radius self-join on the bench index and write profiles/r32_exact_join.json.

On the benchmark's C2 shape (N = 1e6, D = 128, 4096 lists; --n / --nlist shrink it) at the median distance of a stored
record to its 10th other record (from search_exact_device on a sample of stored rows) it records, --repeats calls each,
wall time (host clock around calls that end synchronised), min and max, of
  * cluster_radius_exact_device, components (min_pts 1) and min_pts 5, and radius_graph_exact;
  * the directed exact graph a caller could already get: export_device + range_search_exact_device over all rows in
    chunks of 65 536;
  * the probed cluster_radius_device / radius_graph at n_probe 32 (--probed-repeats calls);
and, per call of the new entries once more under VI_EXACT_TIMING, sweeps, survivors and pairs per row and the phases.
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
    ap.add_argument("--sample", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--probed-repeats", type=int, default=2)
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r32_exact_join.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_exact_join.py needs an MI355X")
    import bench
    import vector_indexer_py as vip
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
    res = {"shape": {"n": args.n, "d": args.d, "nlist": args.nlist}, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as work:
        index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000)
        N = index.num_vectors
        rows = torch.empty((N, args.d), dtype=torch.float32, device=dev)     # the stored rows in list order
        index.export_device(0, N, values_ptr=rows.data_ptr())
        s = min(args.sample, N)
        D = torch.empty((s, 11), dtype=torch.float32, device=dev)
        I = torch.empty((s, 11), dtype=torch.int64, device=dev)
        index.search_exact_device(rows[:: max(N // s, 1)][:s].contiguous().data_ptr(), s, 11, D.data_ptr(), I.data_ptr())
        radius = float(D[:, 10].median().item())                              # (column 0 is the record itself)
        res["radius2"], res["rows"] = radius, N
        labels = torch.empty(N, dtype=torch.int64, device=dev)

        def timed_stats(fn):
            os.environ["VI_EXACT_TIMING"] = "1"
            fn()
            st = index.exact_join_stats()
            del os.environ["VI_EXACT_TIMING"]
            return {"sweeps": st["sweeps"], "tiles": st["tiles"], "segments": st["segments"], "survivors_per_row": st["survivors"] / N,
                    "pairs_per_row": st["pairs"] / N, "hits": st["hits"], "pool_cap": st["pool_cap"], "chunk_rows": st["chunk_rows"],
                    "phases_ms": {f: st[f] for f in ("ms_resolve", "ms_prepare", "ms_sweep", "ms_finish")}}

        calls = {"cluster_exact_components": lambda: index.cluster_radius_exact_device(labels.data_ptr(), 0, radius, 1),
                 "cluster_exact_min_pts_5": lambda: index.cluster_radius_exact_device(labels.data_ptr(), 0, radius, 5),
                 "radius_graph_exact": lambda: index.radius_graph_exact(radius).free()}
        for name, fn in calls.items():
            res[name] = {"ms": span(fn, args.repeats), **timed_stats(fn)}

        def chunked():  # what a caller could do before: every ordered pair, the whole directed graph
            total = 0
            for q0 in range(0, N, 65536):
                m = min(65536, N - q0)
                r = index.range_search_exact_device(rows[q0:q0 + m].data_ptr(), m, radius)
                total += r.total
                r.free()
            return total
        res["export_plus_range_exact_chunks"] = {"ms": span(chunked, args.repeats), "hits": chunked()}
        P = min(args.n_probe, index.num_centroids)
        res["probed"] = {"n_probe": P,
                         "cluster_radius_components_ms": span(lambda: index.cluster_radius_device(labels.data_ptr(), 0, radius, P, 1), args.probed_repeats),
                         "radius_graph_ms": span(lambda: index.radius_graph(radius, P).free(), args.probed_repeats)}
        res["ratio_graph_exact_to_chunks"] = res["radius_graph_exact"]["ms"][0] / res["export_plus_range_exact_chunks"]["ms"][0]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
