#!/usr/bin/env python3
"""Measurement (not a test): what a search by stored record costs, on the C2-shaped synthetic index bench.py builds
(N = 1e6, D = 128, 4096 lists, nprobe 32, k = 10).  Writes profiles/r20_similar_search.json.

  (a) search_by_ids_device for 10 000 resident ids, the record itself excluded and not, beside what a caller composes
      from the entries that existed before it: get_device (ids -> vectors) followed by search_device at the same k.  The
      composition needs nothing of this feature, so --part compose runs it alone against ANY checkout (--root): the
      yardstick is that composition timed on the parent commit's library, in processes that alternate with this one's
      (--part entry: the composition and the new entry; --part all: the rest as well).
      Every process loads the same index files (--work, built by the first).
  (b) knn_graph_device over the whole index, rows per second, per chunk size, beside export_device + search_device on the
      same rows in chunks of the same size.
  (c) self_drop_kernel: bytes moved against its HIP-event time (VI_SIMILAR_TIMING), on the graph's rows.
  (d) --bench-dir: the headline figures of alternating bench.py runs of the parent and of this checkout (files
      bench_parent_<i>.json / bench_branch_<i>.json holding bench.py's result line), recorded as two series.

Parts are merged into --out: a run adds its own keys and keeps the others."""
import argparse
import glob
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=HERE, help="checkout whose library is measured")
ap.add_argument("--part", choices=["compose", "entry", "all", "merge"], default="all")
ap.add_argument("--label", default=None, help="name of this process's series in the output (compose: e.g. parent_0)")
ap.add_argument("--work", default="/tmp/vi_similar_search", help="index files: built if absent, loaded otherwise")
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--nq", type=int, default=10_000)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--chunks", default="16384,65536,262144")
ap.add_argument("--bench-dir", default=None)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r20_similar_search.json"))
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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


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
                "branch_median": statistics.median(series["branch"]), "parent_median": statistics.median(series["parent"]),
                "branch_median_inside_parent_spread": bool(lo <= statistics.median(series["branch"]) <= hi),
                "branch_runs_below_parent_min": int(sum(v < lo for v in series["branch"]))}
    out = merge_out(res)
    a = out.get("a_by_ids", {})
    par = [v for key, v in sorted(a.get("compose_runs", {}).items()) if key.startswith("parent")]
    own = [v for key, v in sorted(a.get("compose_runs", {}).items()) if key.startswith("branch")]
    if par and "entry" in a:
        med = lambda runs, f: statistics.median(r[f]["median_ms"] for r in runs)  # noqa: E731
        summary = {"parent_compose_ms (get_device + search_device, k)": {"median_of_runs": round(med(par, "compose_k"), 4),
                                                                           "runs": [r["compose_k"]["median_ms"] for r in par]},
                   "entry_exclude_on_ms": {"median_of_runs": round(statistics.median(r["exclude_on"]["median_ms"] for r in a["entry"].values()), 4),
                                           "runs": [r["exclude_on"]["median_ms"] for _, r in sorted(a["entry"].items())]},
                   "entry_exclude_off_ms": {"median_of_runs": round(statistics.median(r["exclude_off"]["median_ms"] for r in a["entry"].values()), 4),
                                            "runs": [r["exclude_off"]["median_ms"] for _, r in sorted(a["entry"].items())]},
                   "drop_kernel_ms": {"runs": [r["exclude_on"]["ms_drop_per_call"] for _, r in sorted(a["entry"].items())]}}
        if own:
            summary["branch_compose_ms (same composition, this checkout)"] = {"median_of_runs": round(med(own, "compose_k"), 4),
                                                                               "runs": [r["compose_k"]["median_ms"] for r in own]}
        merge_out({"a_by_ids": {"summary": summary}})
    print(json.dumps(merge_out({})))
    sys.exit(0)

sys.path[:0] = [args.root, os.path.join(args.root, "tests"), os.path.join(args.root, "vector-indexer_amd")]
os.environ["VI_SIMILAR_TIMING"] = "1"
import bench  # noqa: E402
import vector_indexer_py as vip  # noqa: E402

dev = torch.device("cuda", 0)
n, d, nq, k, P = args.n, args.d, args.nq, args.k, args.nprobe
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
rng = np.random.default_rng(7)
ids = rng.permutation(ext)[:nq].copy()
ids_dev = torch.from_numpy(ids.view(np.int64)).to(dev)
Q = torch.empty((nq, d), dtype=torch.float32, device=dev)
D = torch.empty((nq, k + 1), dtype=torch.float32, device=dev)
I = torch.empty((nq, k + 1), dtype=torch.int64, device=dev)


def timed(step, after=None):
    """host wall clock per call (every entry returns with its results complete): warm-up, then args.steps calls"""
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


def compose(kk):
    index.get_device(ids_dev.data_ptr(), nq, 0, Q.data_ptr())
    index.search_device(Q.data_ptr(), nq, kk, P, D.data_ptr(), I.data_ptr())


label = args.label or ("run" if args.part == "compose" else "branch")
runs = {"compose_k": spread(timed(lambda: compose(k))[0]), "compose_k_plus_1": spread(timed(lambda: compose(k + 1))[0]),
        "get_device_alone": spread(timed(lambda: index.get_device(ids_dev.data_ptr(), nq, 0, Q.data_ptr()))[0]),
        "search_device_alone_k": spread(timed(lambda: index.search_device(Q.data_ptr(), nq, k, P, D.data_ptr(), I.data_ptr()))[0])}
result = {"workload": f"N={n} D={d} nlist={args.nlist} nprobe={P} k={k}; {nq} resident ids in device memory; host wall clock per "
                      f"call, {args.steps} calls after {args.warmup} warm-up calls per run; one process per run, all loading the same index files",
          "a_by_ids": {"compose_runs": {label: runs}}}
if args.part == "compose":
    merge_out(result)
    print(json.dumps(result))
    sys.exit(0)

# ---- (a) the new entry ----
entry = {}
for name, excl in (("exclude_on", True), ("exclude_off", False)):
    ms, tm = timed(lambda: index.search_by_ids_device(ids_dev.data_ptr(), nq, k, P, D.data_ptr(), I.data_ptr(), exclude_self=excl),
                   after=index.similar_times)
    entry[name] = spread(ms)
    entry[name].update({"ms_resolve_per_call": round(statistics.median(t["ms_resolve"] for t in tm), 4),
                        "ms_search_per_call": round(statistics.median(t["ms_search"] for t in tm), 4),
                        "ms_drop_per_call": round(statistics.median(t["ms_drop"] for t in tm), 4),
                        "drop_bytes": tm[-1]["drop_bytes"]})
# the entry's rows against the composition's (k + 1 wide, the record's own hit deleted by id: the ids here are unique)
index.search_by_ids_device(ids_dev.data_ptr(), nq, k, P, D.data_ptr(), I.data_ptr(), exclude_self=True)
Ie = I.view(-1)[: nq * k].view(nq, k).clone()
compose(k + 1)
Ic = I.view(-1)[: nq * (k + 1)].view(nq, k + 1)
own = Ic == ids_dev[:, None]
keep = (~own).cumsum(dim=1) <= k
same = bool(all(torch.equal(Ic[r][(~own[r]) & keep[r]][:k], Ie[r]) for r in range(0, nq, 97)))
result["a_by_ids"]["entry"] = {label: entry}
result["a_by_ids"]["entry_rows_equal_composition_less_own_hit (sampled)"] = same
merge_out(result)
if args.part == "entry":
    print(json.dumps(result))
    sys.exit(0)

# ---- (b) the k-NN graph of the whole index, (c) the drop kernel ----
Dg = torch.empty((n, k), dtype=torch.float32, device=dev)
Ig = torch.empty((n, k), dtype=torch.int64, device=dev)
graph, drop = {}, {}
for C in [int(c) for c in args.chunks.split(",")]:
    os.environ["VI_GRAPH_CHUNK"] = str(C)
    Qc = torch.empty((C, d), dtype=torch.float32, device=dev)
    g = {}
    for name, excl in (("exclude_on", True), ("exclude_off", False)):
        index.knn_graph_device(0, min(n, 2 * C), k, P, Dg.data_ptr(), Ig.data_ptr(), exclude_self=excl)   # warm-up: two chunks
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index.knn_graph_device(0, n, k, P, Dg.data_ptr(), Ig.data_ptr(), exclude_self=excl)
        s = time.perf_counter() - t0
        tm = index.similar_times()
        g[name] = {"seconds": round(s, 4), "rows_per_s": round(n / s, 1), "ms_resolve": round(tm["ms_resolve"], 3),
                   "ms_search": round(tm["ms_search"], 3), "ms_drop": round(tm["ms_drop"], 4), "chunk_rows": tm["chunk_rows"]}
        if excl and tm["ms_drop"] > 0:
            drop[str(C)] = {"bytes": tm["drop_bytes"], "ms": round(tm["ms_drop"], 4), "launches": -(-n // C),
                            "GB_per_s": round(tm["drop_bytes"] / tm["ms_drop"] / 1e6, 1)}

    def by_export():
        for at in range(0, n, C):
            m = min(C, n - at)
            index.export_device(at, m, 0, Qc.data_ptr())
            index.search_device(Qc.data_ptr(), m, k, P, Dg.data_ptr() + at * k * 4, Ig.data_ptr() + at * k * 8)

    by_export() if 2 * C >= n else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    by_export()
    s = time.perf_counter() - t0
    g["export_device + search_device (no exclusion possible)"] = {"seconds": round(s, 4), "rows_per_s": round(n / s, 1)}
    graph[str(C)] = g
    del Qc
os.environ.pop("VI_GRAPH_CHUNK", None)
result["b_knn_graph"] = {"rows": n, "chunk_sizes_tried": [int(c) for c in args.chunks.split(",")], "by_chunk": graph}
result["c_self_drop_kernel"] = {"note": "bytes: D, I, slots of k + 1 entries read, D, I of k entries written, three words per row; "
                                        "HIP events around the launches of one graph call, summed over its chunks", "by_chunk": drop}
print(json.dumps(merge_out(result)))
