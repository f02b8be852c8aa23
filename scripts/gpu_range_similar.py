#!/usr/bin/env python3
"""Measurement (not a test): what a radius search by stored record costs, on the C2-shaped synthetic index bench.py builds
(N = 1e6, D = 128, 4096 lists, nprobe 32).  Writes profiles/r21_range_similar.json.

The radii are the medians over the 10 000 chosen records of their 1st, 10th and 100th neighbour distance, taken from a
top-k search (k = 101, the record itself first) of their stored vectors on the same handle.

  (a) range_search_by_ids_device for 10 000 resident ids in device memory, the record itself excluded and not, at the three
      radii, beside what a caller composes from the entries that existed before it: get_device (ids -> vectors) followed
      by range_search_device.  The composition needs nothing of this feature, so --part compose runs it alone against ANY
      checkout (--root): the yardstick is that composition timed on the parent commit's library, in processes that
      alternate with this one's (--part entry: the composition and the new entry; --part all: the rest as well; --part
      check: nothing timed, only the entry's arrays against the composition's).  Every process loads the same index
      files (--work, built by the first).
  (b) range_find_kernel + range_move_kernel: bytes moved against their HIP-event time (VI_SIMILAR_TIMING) at the three
      radii, from the calls of (a).
  (c) radius_graph over the whole index at the 10th-neighbour radius, per chunk size: rows per second, total hits, bytes
      of the result.
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
ap.add_argument("--part", choices=["compose", "entry", "all", "merge", "check"], default="all",
                help="check: only the comparison of the entry's rows with the composition's")
ap.add_argument("--label", default=None, help="name of this process's series in the output (e.g. parent_0, branch_0)")
ap.add_argument("--work", default="/tmp/vi_range_similar", help="index files: built if absent, loaded otherwise")
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--nq", type=int, default=10_000)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--steps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--chunks", default="16384,65536,262144")
ap.add_argument("--bench-dir", default=None)
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "r21_range_similar.json"))
args = ap.parse_args()
RADII = ("r1", "r10", "r100")


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
                "command": "bench.py --gpus 1 --steps 20 --warmup 3, processes alternating parent / branch, the first of a pair swapped "
                           "from pair to pair", "unit": "queries/s",
                "parent": series["parent"], "branch": series["branch"], "parent_min": lo, "parent_max": hi,
                "branch_min": min(series["branch"]), "branch_max": max(series["branch"]),
                "ranges_overlap": bool(min(series["branch"]) <= hi and lo <= max(series["branch"])),
                "branch_runs_below_parent_min": int(sum(v < lo for v in series["branch"]))}
    out = merge_out(res)
    a = out.get("a_by_ids", {})
    par = [v for key, v in sorted(a.get("compose_runs", {}).items()) if key.startswith("parent")]
    ent = [v for _, v in sorted(a.get("entry", {}).items())]
    if par and ent:
        summary = {}
        for r in RADII:
            pc = [run[r]["median_ms"] for run in par]
            row = {"parent_compose_ms (get_device + range_search_device)": {"runs": pc, "min": min(pc), "max": max(pc)}}
            for name in ("exclude_on", "exclude_off"):
                e = [run[r][name]["median_ms"] for run in ent]
                added = max(run[r][name]["ms_drop_per_call"] for run in ent)
                allowed = max(pc) + added + (max(pc) - min(pc))
                row["entry_" + name + "_ms"] = {"runs": e, "min": min(e), "max": max(e), "event_timed_kernels_ms": added,
                                                "allowed_ms (parent max + kernels + parent spread)": round(allowed, 4),
                                                "within_allowed": bool(max(e) <= allowed)}
            summary[r] = row
        merge_out({"a_by_ids": {"summary": summary}})
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
rng = np.random.default_rng(7)
ids = rng.permutation(ext)[:nq].copy()
ids_dev = torch.from_numpy(ids.view(np.int64)).to(dev)
Q = torch.empty((nq, d), dtype=torch.float32, device=dev)

# ---- the radii: the record itself is column 0 of its own top-101 ----
Dk = torch.empty((nq, 101), dtype=torch.float32, device=dev)
Ik = torch.empty((nq, 101), dtype=torch.int64, device=dev)
index.get_device(ids_dev.data_ptr(), nq, 0, Q.data_ptr())
index.search_device(Q.data_ptr(), nq, 101, P, Dk.data_ptr(), Ik.data_ptr())
torch.cuda.synchronize()
radii = {name: float(Dk[:, col][torch.isfinite(Dk[:, col])].median()) for name, col in zip(RADII, (1, 10, 100))}
del Dk, Ik


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


last = {}


def compose(r):
    index.get_device(ids_dev.data_ptr(), nq, 0, Q.data_ptr())
    res = index.range_search_device(Q.data_ptr(), nq, r, P)
    last["total"] = res.total
    res.free()


label = args.label or ("run" if args.part == "compose" else "branch")
runs = {}
for name, r in ([] if args.part == "check" else radii.items()):
    runs[name] = spread(timed(lambda: compose(r))[0])
    runs[name]["hits"] = last["total"]
result = {"workload": f"N={n} D={d} nlist={args.nlist} nprobe={P}; {nq} resident ids in device memory; host wall clock per call, the "
                      f"result freed inside it; {args.steps} calls after {args.warmup} warm-up calls per run; one process per run, all "
                      "loading the same index files",
          "radii2 (median 1st / 10th / 100th neighbour distance of the chosen records)": radii,
          "a_by_ids": {"compose_runs": {label: runs}} if runs else {}}
if args.part == "compose":
    merge_out(result)
    print(json.dumps(result))
    sys.exit(0)


# ---- (a) the new entry, (b) its two kernels ----
def entry_call(r, excl):
    res = index.range_search_by_ids_device(ids_dev.data_ptr(), nq, r, P, exclude_self=excl)
    last["total"] = res.total
    res.free()


entry, kernels = {}, {}
for name, r in ([] if args.part == "check" else radii.items()):
    entry[name] = {}
    for ename, excl in (("exclude_on", True), ("exclude_off", False)):
        ms, tm = timed(lambda: entry_call(r, excl), after=index.similar_times)
        e = spread(ms)
        e.update({"hits": last["total"],
                  "ms_resolve_per_call": round(statistics.median(t["ms_resolve"] for t in tm), 4),
                  "ms_search_per_call": round(statistics.median(t["ms_search"] for t in tm), 4),
                  "ms_drop_per_call": round(statistics.median(t["ms_drop"] for t in tm), 4),
                  "drop_bytes": tm[-1]["drop_bytes"]})
        entry[name][ename] = e
        if e["ms_drop_per_call"] > 0:
            kernels.setdefault(name, {})[ename] = {"bytes": e["drop_bytes"], "ms": e["ms_drop_per_call"], "hits": e["hits"],
                                                   "GB_per_s": round(e["drop_bytes"] / e["ms_drop_per_call"] / 1e6, 1)}
# the entry's rows against the composition's: without exclusion the same arrays; with it the composition's less the one
# entry per row that carries the row's id (the ids are unique here) — a row whose own list is not among the probed ones
# has no such entry, in either
r = radii["r10"]
index.get_device(ids_dev.data_ptr(), nq, 0, Q.data_ptr())
plain = index.range_search_device(Q.data_ptr(), nq, r, P)
same = index.range_search_by_ids_device(ids_dev.data_ptr(), nq, r, P, exclude_self=False)
less = index.range_search_by_ids_device(ids_dev.data_ptr(), nq, r, P, exclude_self=True)
lp, Dp, Ip = plain.copy()
ls, Ds, Is = same.copy()
lx, Dx, Ix = less.copy()
rowof = np.repeat(np.arange(nq), np.diff(lp.astype(np.int64)))
keep = Ip != ids.view(np.int64)[rowof]
checks = {"exclude_off_equals_composition": bool(np.array_equal(lp, ls) and np.array_equal(Ip, Is) and np.array_equal(Dp.view(np.uint32), Ds.view(np.uint32))),
          "exclude_on_equals_composition_less_own_hit": bool(np.array_equal(Ip[keep], Ix) and np.array_equal(Dp[keep].view(np.uint32), Dx.view(np.uint32))
                                                             and int(lx[-1]) == int(keep.sum())),
          "rows_whose_own_record_was_among_the_hits": int((~keep).sum()), "rows": nq}
for x in (plain, same, less):
    x.free()
if entry:
    result["a_by_ids"]["entry"] = {label: entry}
result["a_by_ids"]["entry_rows_checked_at_r10"] = checks
if args.part == "check":
    print(json.dumps(merge_out({"a_by_ids": {"entry_rows_checked_at_r10": checks}})["a_by_ids"]["entry_rows_checked_at_r10"]))
    sys.exit(0)
result["b_kernels"] = {"note": "range_find_kernel + range_move_kernel of one call: HIP events around the two launches; bytes: per row "
                               "68 (bounds, slot, count, position, length), 8 per input entry scanned for the own slot (counted in full "
                               "though the scan ends at the match), 56 per entry moved (28 read, 28 written)",
                       "by_run": {label: kernels}}
merge_out(result)
if args.part == "entry":
    print(json.dumps(result))
    sys.exit(0)

# ---- (c) the radius graph of the whole index at the 10th-neighbour radius ----
graph = {}
for C in [int(c) for c in args.chunks.split(",")]:
    os.environ["VI_GRAPH_CHUNK"] = str(C)
    g = {}
    for ename, excl in (("exclude_on", True), ("exclude_off", False)):
        index.radius_graph(r, P, first=0, count=min(n, 2 * C), exclude_self=excl).free()   # warm-up: two chunks
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = index.radius_graph(r, P, exclude_self=excl)
        s = time.perf_counter() - t0
        tm = index.similar_times()
        g[ename] = {"seconds": round(s, 4), "rows_per_s": round(n / s, 1), "total_hits": res.total,
                    "result_bytes (28 per hit + lims; its buffers hold at most twice the hits)": res.total * 28 + (n + 1) * 8,
                    "ms_resolve": round(tm["ms_resolve"], 3), "ms_search": round(tm["ms_search"], 3), "ms_drop": round(tm["ms_drop"], 4),
                    "drop_GB_per_s": round(tm["drop_bytes"] / tm["ms_drop"] / 1e6, 1) if tm["ms_drop"] > 0 else None,
                    "chunk_rows": tm["chunk_rows"]}
        res.free()
    graph[str(C)] = g
os.environ.pop("VI_GRAPH_CHUNK", None)
result["c_radius_graph"] = {"rows": n, "radius2": r, "chunk_sizes_tried": [int(c) for c in args.chunks.split(",")], "by_chunk": graph}
print(json.dumps(merge_out(result)))
