#!/usr/bin/env python3
"""Measure the exact (flat) radius search on the bench index and write profiles/r31_exact_range.json.

On the benchmark's C2 shape (N = 1e6, D = 128, 4096 lists, 10 000 device-resident queries; --n / --nq / --nlist shrink it)
it takes three radii — the median distance to the 1st, 10th and 100th neighbour, from search_exact_device — and records
  * range_search_exact_device at each radius against search_exact_device at k = 1 / 10 / 100 on the same handle, the two
    calls alternating, --repeats calls each: wall time (host clock around calls that end synchronised), min and max;
  * per radius, in a separate call under VI_EXACT_TIMING: hits and survivors per query, sweeps, the phase split;
  * range_search_device at n_probe = every list on --nq-probed queries (the generic engine: what the tree offered before),
    and whether its hits equal the exact ones as sets of (distance bits, id).
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
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--nq-probed", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_exact_range.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_exact_range.py needs an MI355X")
    import bench
    import vector_indexer_py as vip
    dev = torch.device("cuda", 0)

    def clock(fn):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t) * 1e3, out

    xb, xq = bench.make_dataset(args.n, args.d, args.nq, 1234, dev)
    nq = args.nq
    res = {"shape": {"n": args.n, "d": args.d, "nlist": args.nlist, "nq": nq}, "device": torch.cuda.get_device_name(0), "radii": {}}
    with tempfile.TemporaryDirectory() as work:
        index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000)
        res["lists"] = index.num_centroids
        ks = [k for k in (1, 10, 100) if k <= min(100, args.n)]
        D = {k: torch.empty((nq, k), dtype=torch.float32, device=dev) for k in ks}
        I = {k: torch.empty((nq, k), dtype=torch.int64, device=dev) for k in ks}
        knn = lambda k: index.search_exact_device(xq.data_ptr(), nq, k, D[k].data_ptr(), I[k].data_ptr())  # noqa: E731
        knn(ks[-1])
        for k in ks:
            radius = float(D[ks[-1]][:, k - 1].median().item())
            rng = lambda: index.range_search_exact_device(xq.data_ptr(), nq, radius).free()  # noqa: E731,B023
            knn(k), rng()  # warm-up: code objects, workspace
            t_knn, t_rng = [], []
            for _ in range(args.repeats):
                t_knn.append(clock(lambda: knn(k))[0])  # noqa: B023
                t_rng.append(clock(rng)[0])
            os.environ["VI_EXACT_TIMING"] = "1"
            rng()
            st = index.exact_range_stats()
            del os.environ["VI_EXACT_TIMING"]
            res["radii"][f"median_neighbour_{k}"] = {
                "radius2": radius, "range_exact_ms": [min(t_rng), max(t_rng)], "search_exact_ms": {"k": k, "ms": [min(t_knn), max(t_knn)]},
                "hits_per_query": st["hits"] / nq, "survivors_per_query": st["survivors"] / nq, "sweeps": st["sweeps"],
                "pool_cap": st["pool_cap"], "block_splits": st["block_splits"],
                "phases_ms": {f: st[f] for f in ("ms_prepare", "ms_sweep", "ms_place", "ms_sort", "ms_output", "ms_total")}}
        # the probed engine at every list, on a handful of queries
        g, radius = min(args.nq_probed, nq), res["radii"][f"median_neighbour_{ks[-1] if 10 not in ks else 10}"]["radius2"]
        probed = lambda: index.range_search_device(xq.data_ptr(), g, radius, index.num_centroids)  # noqa: E731
        probed().free()
        t_probed = []
        for _ in range(2):
            ms, r = clock(probed)
            t_probed.append(ms)
            lp, Dp, Ip = r.copy()
            r.free()
        ms_exact, r = clock(lambda: index.range_search_exact_device(xq.data_ptr(), g, radius))
        le, De, Ie = r.copy()
        r.free()
        rows = lambda l, Dx, Ix: [sorted(zip(Dx[int(l[q]):int(l[q + 1])].view("uint32").tolist(), Ix[int(l[q]):int(l[q + 1])].tolist()))  # noqa: E731
                                  for q in range(g)]
        res["probed_all_lists"] = {"nq": g, "radius2": radius, "ms": t_probed, "range_exact_ms_same_queries": ms_exact,
                                   "equals_exact": rows(lp, Dp, Ip) == rows(le, De, Ie)}
        per_q_probed = min(t_probed) / g
        per_q_exact = res["radii"][f"median_neighbour_{ks[-1] if 10 not in ks else 10}"]["range_exact_ms"][0] / nq
        res["per_query_ms"] = {"probed_all_lists": per_q_probed, "range_exact": per_q_exact, "ratio": per_q_probed / per_q_exact}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
