#!/usr/bin/env python3
"""Measurement (not a test): what clustering the stored records by radius costs, on the C2-shaped synthetic index bench.py
builds (N = 1e6, D = 128, 4096 lists, nprobe 32).  Writes profiles/r22_cluster_radius.json.

The radius is the median 10th-neighbour distance of 10 000 stored records, taken from a top-k search (k = 11, the record
itself first) of their stored vectors on the same handle.  One process per figure, all loading the same index files
(--work, built by the first); a job that runs several stops at the first that fails.

  --part graph    radius_graph(exclude_self = 1) over the whole index, the result freed inside the timed call.  It needs
                  nothing of this feature: with --root it runs against ANY checkout, and the yardstick of (a) is this part
                  on the parent commit's library, in processes that alternate with --part cluster of this one.
  --part cluster  (a) cluster_radius_device(min_pts = 1), (b) min_pts = 5 (two passes), with the HIP-event times and
                  bytes of the link and label kernels (VI_SIMILAR_TIMING), and (c) the peak device memory of a call:
                  hipMemGetInfo sampled from a second thread while it runs, beside the bytes of the per-slot arrays.
  --part merge    the bound of (a) from the series in --out, and (d) --bench-dir: the headline figures of alternating
                  bench.py runs of the parent and of this checkout (bench_parent_<i>.json / bench_branch_<i>.json)."""
import argparse
import glob
import json
import os
import statistics
import sys
import threading
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE, help="checkout whose library is measured")
ap.add_argument("--part", choices=["graph", "cluster", "merge"], default="cluster")
ap.add_argument("--label", default=None, help="name of this process's series in the output (e.g. parent_0, branch_0)")
ap.add_argument("--work", default="/tmp/vi_cluster_radius", help="index files: built if absent, loaded otherwise")
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--nq", type=int, default=10_000)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--bench-dir", default=None)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r22_cluster_radius.json"))
args = ap.parse_args()


def merge_out(update):
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            res = json.load(fh)

    def deep(into, new):
        for key, val in new.items():
            if isinstance(val, dict) and isinstance(into.get(key), dict):
                deep(into[key], val)
            else:
                into[key] = val

    deep(res, update)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return res


def spread(ms):
    return {"runs_ms": [round(x, 3) for x in ms], "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3)}


if args.part == "merge":
    res = {}
    if args.bench_dir:
        series = {}
        for who in ("parent", "branch"):
            vals = []
            for path in sorted(glob.glob(os.path.join(args.bench_dir, f"bench_{who}_*.json"))):
                with open(path) as fh:
                    lines = [ln for ln in fh.read().splitlines() if ln.startswith("{")]
                vals.append(json.loads(lines[-1])["value"])
            series[who] = vals
        if series["parent"] and series["branch"]:
            lo, hi = min(series["parent"]), max(series["parent"])
            res["d_bench_alternating"] = {
                "command": "bench.py --gpus 1 --steps 20 --warmup 3, processes alternating parent / branch", "unit": "queries/s",
                "parent": series["parent"], "branch": series["branch"], "parent_min": lo, "parent_max": hi,
                "branch_min": min(series["branch"]), "branch_max": max(series["branch"]),
                "ranges_overlap": bool(min(series["branch"]) <= hi and lo <= max(series["branch"]))}
    out = merge_out(res)
    par = [v for key, v in sorted(out.get("a_graph_runs", {}).items()) if key.startswith("parent")]
    own = [v for _, v in sorted(out.get("a_cluster_runs", {}).items())]
    if par and own:
        graph = [x for run in par for x in run["runs_ms"]]
        clus = [x for run in own for x in run["min_pts_1"]["runs_ms"]]
        kernels = max(run["min_pts_1"]["ms_link"] + run["min_pts_1"]["ms_label"] for run in own)
        allowed = max(graph) + kernels + (max(graph) - min(graph))
        merge_out({"a_summary": {"parent_radius_graph_ms": {"min": min(graph), "max": max(graph)},
                                 "cluster_radius_min_pts_1_ms": {"min": min(clus), "max": max(clus)},
                                 "event_timed_link_and_label_kernels_ms": round(kernels, 4),
                                 "allowed_ms (parent max + kernels + parent max - min)": round(allowed, 3),
                                 "within_allowed": bool(max(clus) <= allowed)}})
    print(json.dumps(merge_out({})))
    sys.exit(0)

sys.path[:0] = [args.root, os.path.join(args.root, "tests"), os.path.join(args.root, "vector-indexer_amd")]
os.environ["VI_SIMILAR_TIMING"] = "1"
import bench  # noqa: E402
import vector_indexer_py as vip  # noqa: E402

dev = torch.device("cuda", 0)
n, d, nq, P = args.n, args.d, args.nq, args.nprobe
rows = np.arange(n, dtype=np.uint64)
ext = ((rows % np.uint64(5)) << np.uint64(40)) | (np.uint64(7) * rows + np.uint64(3))
if os.path.exists(os.path.join(args.work, "index")):
    index = vip.load(os.path.join(args.work, "index"), os.path.join(args.work, "shards"), d)
else:
    xb, _ = bench.make_dataset(n, d, nq, 42, dev)
    os.makedirs(args.work, exist_ok=True)
    index = vip.build(xb.cpu().numpy(), args.work, nlist=args.nlist, now_secs=1_700_000_000, ext_ids=ext)
    del xb
assert index.num_vectors == n

# ---- the radius: the record itself is column 0 of its own top-11 ----
rng = np.random.default_rng(7)
ids_dev = torch.from_numpy(rng.permutation(ext)[:nq].copy().view(np.int64)).to(dev)
Q = torch.empty((nq, d), dtype=torch.float32, device=dev)
Dk = torch.empty((nq, 11), dtype=torch.float32, device=dev)
Ik = torch.empty((nq, 11), dtype=torch.int64, device=dev)
index.get_device(ids_dev.data_ptr(), nq, 0, Q.data_ptr())
index.search_device(Q.data_ptr(), nq, 11, P, Dk.data_ptr(), Ik.data_ptr())
torch.cuda.synchronize()
r = float(Dk[:, 10][torch.isfinite(Dk[:, 10])].median())
del Dk, Ik, Q
label = args.label or args.part
workload = {"workload": f"N={n} D={d} nlist={args.nlist} nprobe={P}; radius2 = median 10th-neighbour distance of {nq} stored records; "
                        f"host wall clock per call, {args.steps} calls after {args.warmup} warm-up per process; one process per run, "
                        "all loading the same index files", "radius2": r}


def timed(step, after=None):
    for _ in range(args.warmup):
        step()
    ms, extra = [], []
    for _ in range(args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        ms.append((time.perf_counter() - t0) * 1e3)
        if after:
            extra.append(after())
    return ms, extra


if args.part == "graph":
    last = {}

    def graph():
        res = index.radius_graph(r, P, exclude_self=True)
        last["total"] = res.total
        res.free()

    run = spread(timed(graph)[0])
    run.update({"hits": last["total"], "result_bytes (28 per hit + lims)": last["total"] * 28 + (n + 1) * 8})
    print(json.dumps(merge_out({**workload, "a_graph_runs": {label: run}})["a_graph_runs"][label]))
    sys.exit(0)

# ---- (a) min_pts 1, (b) min_pts 5, (c) the memory of a call ----
labels = torch.empty(n, dtype=torch.int64, device=dev)
degree = torch.empty(n, dtype=torch.int32, device=dev)
run = {}
for min_pts in (1, 5):
    got = {}

    def cluster():
        got["n_clusters"] = index.cluster_radius_device(labels.data_ptr(), degree.data_ptr(), r, P, min_pts)

    ms, st = timed(cluster, after=index.cluster_stats)
    e = spread(ms)
    s = st[-1]
    link = statistics.median(x["ms_link"] for x in st)
    e.update({k: s[k] for k in ("rows", "hits", "passes", "n_core", "n_border", "n_noise", "n_clusters", "chunk_rows", "link_bytes")})
    e.update({"ms_resolve": round(statistics.median(x["ms_resolve"] for x in st), 3),
              "ms_search": round(statistics.median(x["ms_search"] for x in st), 3), "ms_link": round(link, 4),
              "ms_label": round(statistics.median(x["ms_label"] for x in st), 4),
              "link_GB_per_s": round(s["link_bytes"] / link / 1e6, 1) if link > 0 else None,
              "labelled_records_not_below_their_label (core records; a border record may precede its cluster)": bool((labels[labels >= 0] <= torch.nonzero(labels >= 0).flatten()).all()),
              "n_clusters_returned": got["n_clusters"], "distinct_labels": int(torch.unique(labels[labels >= 0]).numel())})
    run[f"min_pts_{min_pts}"] = e

# (c) free device memory sampled while one call runs (min_pts 1), against the level before it
torch.cuda.synchronize()
free0 = torch.cuda.mem_get_info()[0]
low, stop = [free0], threading.Event()


def sample():
    while not stop.is_set():
        low[0] = min(low[0], torch.cuda.mem_get_info()[0])
        time.sleep(0.0005)


t = threading.Thread(target=sample, daemon=True)
t.start()
index.cluster_radius_device(labels.data_ptr(), degree.data_ptr(), r, P, 1)
stop.set()
t.join()
hits = run["min_pts_1"]["hits"]
memory = {"free_before_call": free0, "lowest_free_sampled_during_call": low[0], "peak_extra_bytes_sampled": free0 - low[0],
          "note": "the search context's workspace and chunk result are grow-only and already allocated by the calls before: the "
                  "sampled figure is the call's own scratch (12 bytes and one bit per slot, counters), freed on return",
          "radius_graph_result_bytes_for_comparison": hits * 28 + (n + 1) * 8, "labels_bytes": n * 8}
print(json.dumps(merge_out({**workload, "a_cluster_runs": {label: run}, "c_memory": {label: memory}})["a_cluster_runs"][label]))
