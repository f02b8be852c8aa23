#!/usr/bin/env python3
"""Measurement (not a test): what the device merge of per-rank radius results costs beside the ranks' own radius searches,
on the C2-shaped synthetic index bench.py builds.

The index is built once and loaded as 4 and as 8 in-process stripe ranks on one GPU.  10 000 device-resident queries,
nprobe 32, two radii: the median over the queries of their 10th and 100th neighbour distance (from a top-k search of the
unpartitioned handle).  Every shape is warmed up once.  Recorded per (world, radius): each rank's
vi_indexer_range_search_device time (host clock; the call returns complete), the merge's time (host clock around
vi_range_merge_device, which ends synchronised), the two kernels' HIP-event times and the time between them (lims
read-back, synchronisation, allocation) under VI_RANGE_MERGE_TIMING, the entries merged, and the byte floor: 20 B in + 20 B
out per entry plus the lims, over the HBM peak rate.  The yardstick is the slowest rank's radius search of the same batch in
the same run.  --headline DIR adds the bench.py figures of parent and branch found there (bench_<side>_<n>.json, the JSON
line each run printed); with --headline-only that is all it does, to the file --out names (no GPU needed).  Writes
profiles/r18_range_merge.json."""
import argparse
import glob
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "vector-indexer_amd")]

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (6.3 TB/s is what a float4 copy reaches)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--nq", type=int, default=10_000)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--worlds", type=int, nargs="+", default=[4, 8])
ap.add_argument("--headline", default=None, help="directory with bench_parent_<n>.json / bench_this_<n>.json")
ap.add_argument("--headline-only", action="store_true", help="add --headline to the existing --out file and stop")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_range_merge.json"))
args = ap.parse_args()


def measure():
    import torch

    import bench
    import vector_indexer_py as vip
    from vector_indexer_py import _native

    dev = torch.device("cuda", 0)
    xb, xq = bench.make_dataset(args.n, args.d, args.nq, 42, dev)
    work = tempfile.mkdtemp(prefix="vi_range_merge_")
    whole = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000)
    idx, sh = os.path.join(work, "index"), os.path.join(work, "shards")
    nq, P = args.nq, args.nprobe
    D = torch.empty((nq, 100), dtype=torch.float32, device=dev)
    I = torch.empty((nq, 100), dtype=torch.int64, device=dev)
    whole.search_device(xq.data_ptr(), nq, 100, P, D.data_ptr(), I.data_ptr(), 0)
    torch.cuda.synchronize()
    radii = {k: float(D[:, k - 1][torch.isfinite(D[:, k - 1])].median().item()) for k in (10, 100)}

    def ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    def med(v):
        return round(statistics.median(v), 4)

    def kernel_times():
        import ctypes as C
        a, b, c = C.c_float(0), C.c_float(0), C.c_float(0)
        _native.check(_native.lib().vi_range_merge_last_times(C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist} nprobe={P} nq={nq}; in-process stripe ranks on one GPU; one warm-up, "
                          f"then the median of {args.repeats} repeats", "lists": whole.num_centroids, "hbm_peak_gb_s": HBM_PEAK_GBS,
              "cases": {}}
    for world in args.worlds:
        ranks = [vip.load(idx, sh, args.d, rank=r, world_size=world) for r in range(world)]
        for kth, r in radii.items():
            per_rank, merge_ms, lims_ms, alloc_ms, place_ms, merge_timed_ms = [[] for _ in range(world)], [], [], [], [], []
            total = 0
            for rep in range(args.repeats + 1):      # (rep 0: the warm-up)
                parts = []
                for i, ix in enumerate(ranks):
                    t, res = ms(lambda: ix.range_search_device(xq.data_ptr(), nq, r, P))
                    parts.append(res)
                    if rep:
                        per_rank[i].append(t)
                t, merged = ms(lambda: vip.merge_range_results(0, parts))
                total = merged.total
                merged.free()
                os.environ["VI_RANGE_MERGE_TIMING"] = "1"
                try:
                    t2, merged = ms(lambda: vip.merge_range_results(0, parts))
                    k = kernel_times()
                finally:
                    del os.environ["VI_RANGE_MERGE_TIMING"]
                merged.free()
                for x in parts:
                    x.free()
                if rep:
                    merge_ms.append(t)
                    merge_timed_ms.append(t2)
                    lims_ms.append(k[0]), alloc_ms.append(k[1]), place_ms.append(k[2])
            whole_ms = []
            for rep in range(3):
                t, res = ms(lambda: whole.range_search_device(xq.data_ptr(), nq, r, P))
                res.free()
                whole_ms.append(t)
            floor_bytes = 40 * total + (world + 1) * (nq + 1) * 8
            slowest = max(med(v) for v in per_rank)
            result["cases"][f"world_{world}_neighbour_{kth}"] = {
                "world": world, "radius2": r, "radius_is_median_distance_of_neighbour": kth, "entries_merged": total,
                "mean_hits_per_query": round(total / nq, 3),
                "rank_range_search_ms": [med(v) for v in per_rank], "slowest_rank_ms": slowest,
                "unpartitioned_range_search_ms": med(whole_ms),
                "merge_wall_ms": med(merge_ms), "merge_wall_min_ms": round(min(merge_ms), 4), "merge_wall_max_ms": round(max(merge_ms), 4),
                "merge_wall_with_events_ms": med(merge_timed_ms),
                "lims_kernel_ms": med(lims_ms), "between_kernels_ms": med(alloc_ms), "place_kernel_ms": med(place_ms),
                "byte_floor_bytes": floor_bytes, "byte_floor_ms": round(floor_bytes / (HBM_PEAK_GBS * 1e9) * 1e3, 5),
                "place_kernel_gb_s": round(40 * total / (med(place_ms) * 1e-3) / 1e9, 1) if med(place_ms) > 0 else None,
                "merge_over_slowest_rank": round(med(merge_ms) / slowest, 3) if slowest else None}
        del ranks
    return result


if args.headline_only:
    result = json.load(open(args.out))
else:
    result = measure()

if args.headline:
    runs = {}
    for path in sorted(glob.glob(os.path.join(args.headline, "bench_*_*.json"))):
        side = os.path.basename(path).split("_")[1]
        for line in open(path):
            line = line.strip()
            if line.startswith("{") and '"metric"' in line:
                runs.setdefault(side, []).append(json.loads(line)["value"])
    result["headline"] = {"what": "bench.py --gpus 1 --steps 20 --warmup 5, a fresh process per run, in the order parent, this, this, parent",
                          "unit": "queries/s", "parent": runs.get("parent", []), "this": runs.get("this", [])}
    if runs.get("parent") and runs.get("this"):
        lo, hi = min(runs["parent"]), max(runs["parent"])
        result["headline"]["this_inside_parent_range"] = [lo <= v <= hi for v in runs["this"]]
        result["headline"]["this_above_parent_maximum"] = [v > hi for v in runs["this"]]
        result["headline"]["this_below_parent_minimum"] = [v < lo for v in runs["this"]]

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
