#!/usr/bin/env python3
"""Measurement (not a test): what a radius search costs beside the top-k search, on the C2-shaped synthetic index
bench.py builds.

10 000 device-resident queries, nprobe 32.  Three radii: the median over the queries of their 1st, 10th and 100th
neighbour distance (from a top-k search of the same handle).  Timed: vi_indexer_range_search_device per radius beside
vi_indexer_search_device at k = 1 / 10 / 100 (wall clock per step, median and spread of several repeats, the two
alternating so that drift lands on both alike), then the phase split from HIP events — coarse, grouping and rank are the
same launches, the difference is the select's — and, per radius: mean hits per query, sub-blocks re-evaluated per query
(VI_FILTER_STATS) and the split of the radius select into bound pass / evaluation / sort / placing + output
(VI_FILTER_STATS=3 prints it).  Writes profiles/r05_range_search.json."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "vector-indexer_amd")]
import bench  # noqa: E402
import vector_indexer_py as vip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--nq", type=int, default=10_000)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_range_search.json"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
xb, xq = bench.make_dataset(args.n, args.d, args.nq, 42, dev)
work = tempfile.mkdtemp(prefix="vi_range_")
index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000)
nq, P = args.nq, args.nprobe
KS = (1, 10, 100)
D = torch.empty((nq, max(KS)), dtype=torch.float32, device=dev)
I = torch.empty((nq, max(KS)), dtype=torch.int64, device=dev)


def topk_step(k):
    index.search_device(xq.data_ptr(), nq, k, P, D.data_ptr(), I.data_ptr(), 0)


def range_step(r):
    res = index.range_search_device(xq.data_ptr(), nq, r, P)
    total = res.total
    res.free()
    return total


def wall(step, arg):
    """ms per step: args.repeats x (warm-up + timed steps); both entries return with their results complete"""
    out = []
    for _ in range(args.repeats):
        for _ in range(args.warmup):
            step(arg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(arg)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / args.steps)
    return out


def phases(step, arg):
    index.enable_timing(True)
    acc = {}
    for r in range(args.warmup + 8):
        step(arg)
        if r >= args.warmup:
            st = index.last_stats()
            for f, name in (("ms_coarse", "coarse"), ("ms_group", "grouping"), ("ms_scan", "list_rank"), ("ms_merge", "select"),
                            ("ms_total", "total")):
                acc.setdefault(name, []).append(st[f])
    index.enable_timing(False)
    return {name: round(statistics.median(v), 4) for name, v in acc.items()}, index.last_stats()


def with_stderr(fn):
    """fn() with file descriptor 2 captured (the library prints its diagnostic clocks there)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return out, tmp.read().decode("utf-8", "replace")


def select_counters(r):
    """sub-blocks re-evaluated per query and the radius select's own step clocks"""
    os.environ["VI_FILTER_STATS"] = "3"
    index.enable_timing(True)
    try:
        for _ in range(3):
            range_step(r)
        _, err = with_stderr(lambda: range_step(r))
        st = index.last_stats()
    finally:
        index.enable_timing(False)
        del os.environ["VI_FILTER_STATS"]
    m = re.search(r"range select ms: bound pass ([\d.]+), evaluation ([\d.]+), sort ([\d.]+), placing \+ output ([\d.]+); hits (\d+) of a bound of (\d+)", err)
    steps = dict(zip(("bound_pass", "evaluation", "sort", "place_output"), (float(x) for x in m.groups()[:4]))) if m else None
    out = {"vectors_reevaluated_per_query": round(st["filter_rechecked"] / nq, 2),
           "sub_blocks_reevaluated_per_query": round(st["filter_rechecked"] / 16.0 / nq, 2),   # (an upper bound: tail sub-blocks hold fewer)
           "select_steps_ms_with_counters_on": steps}
    if steps:
        tot = sum(steps.values())
        out["sizing_sort_output_share"] = round((steps["bound_pass"] + steps["sort"] + steps["place_output"]) / tot, 3) if tot else None
        out["bound_keys"] = int(m.group(6))
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs_ms": [round(v, 4) for v in ms]}


topk_step(max(KS))
torch.cuda.synchronize()
radii = {k: float(D[:, k - 1][torch.isfinite(D[:, k - 1])].median().item()) for k in KS}
result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist} nprobe={P} nq/step={nq}; device entries, {args.steps} timed steps "
                      f"after {args.warmup} warm-up steps per run, {args.repeats} runs per case, top-k and radius alternating",
          "lists": index.num_centroids, "cases": {}}
for k in KS:
    r = radii[k]
    walls = {"topk": [], "range": []}
    for _ in range(2):      # alternate
        walls["topk"].extend(wall(topk_step, k))
        walls["range"].extend(wall(range_step, r))
    ph_t, st_t = phases(topk_step, k)
    ph_r, st_r = phases(range_step, r)
    total = range_step(r)
    case = {"radius2": r, "radius_is_median_distance_of_neighbour": k,
            "topk": {"k": k, "wall": summary(walls["topk"]), "phases_ms": ph_t},
            "range": {"wall": summary(walls["range"]), "phases_ms": ph_r, "mean_hits_per_query": round(total / nq, 3),
                      "rank_mode": int(st_r["rank_mode"]), "rank_int8": int(st_r["rank_int8"]),
                      "scanned_vectors": int(st_r["scanned_vectors"])},
            "wall_ratio_range_over_topk": round(statistics.median(walls["range"]) / statistics.median(walls["topk"]), 3),
            "select_ratio_range_over_topk": round(ph_r["select"] / ph_t["select"], 3) if ph_t["select"] else None}
    case["range"].update(select_counters(r))
    result["cases"][f"neighbour_{k}"] = case
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
