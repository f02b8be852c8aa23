#!/usr/bin/env python3
"""Measurement (not a test): what a timestamp-window filter costs on the C2-shaped synthetic index bench.py builds.

Timestamps are spread uniformly over 1000 values.  Timed: the device entry unfiltered and with windows admitting 100 %,
50 %, 10 % and 1 % of the stored vectors (wall clock per step, median and spread of several repeats; then the phase split
from HIP events, where `select` is the part a narrow window moves work into), and the creation of a filter beside the
HBM floor of its streams.  Writes profiles/r05_filtered_search.json."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
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
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--nprobe", type=int, default=32)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_filtered_search.json"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
xb, xq = bench.make_dataset(args.n, args.d, args.nq, 42, dev)
ts = (1 + (np.arange(args.n, dtype=np.uint64) * 7919) % 1000).astype(np.uint64)   # 1 .. 1000, uniform
work = tempfile.mkdtemp(prefix="vi_filtered_")
index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000, timestamps=ts)
nq, k, P = args.nq, args.k, args.nprobe
D = torch.empty((nq, k), dtype=torch.float32, device=dev)
I = torch.empty((nq, k), dtype=torch.int64, device=dev)


def step(flt):
    index.search_device(xq.data_ptr(), nq, k, P, D.data_ptr(), I.data_ptr(), 0, filter=flt)


def wall(flt):
    """ms per step: args.repeats x (warm-up + timed steps); the entry returns with its results complete"""
    out = []
    for _ in range(args.repeats):
        for _ in range(args.warmup):
            step(flt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(flt)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / args.steps)
    return out


def phases(flt):
    index.enable_timing(True)
    acc = {}
    for r in range(args.warmup + 8):
        step(flt)
        if r >= args.warmup:
            st = index.last_stats()
            for f, name in (("ms_coarse", "coarse"), ("ms_group", "grouping"), ("ms_scan", "list_rank"), ("ms_merge", "select"),
                            ("ms_total", "total")):
                acc.setdefault(name, []).append(st[f])
    index.enable_timing(False)
    ph = {name: round(statistics.median(v), 4) for name, v in acc.items()}
    ph["select_share"] = round(ph["select"] / ph["total"], 3) if ph["total"] else None
    return ph, index.last_stats()


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs_ms": [round(v, 4) for v in ms]}


windows = {"100%": (1, 1000), "50%": (1, 500), "10%": (1, 100), "1%": (1, 10)}
filters, creation = {}, {}
for name, (lo, hi) in windows.items():
    t = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = index.filter_timestamps(lo, hi)
        t.append((time.perf_counter() - t0) * 1e3)
    filters[name] = f
    creation[name] = {"ms_first": round(t[0], 4), "ms_median_of_later": round(statistics.median(t[1:]), 4),
                      "num_allowed": f.num_allowed}

# unfiltered and 100 % alternate, so that drift over the run lands on both alike
order = ["unfiltered", "100%", "unfiltered", "100%", "50%", "10%", "1%"]
walls = {}
for name in order:
    walls.setdefault(name, []).extend(wall(filters.get(name)))
result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist} nprobe={P} k={k} nq/step={nq}, timestamps uniform over 1000 values; "
                      f"device entry, {args.steps} timed steps after {args.warmup} warm-up steps per run",
          "lists": index.num_centroids, "cases": {}}
for name in ["unfiltered", "100%", "50%", "10%", "1%"]:
    ph, st = phases(filters.get(name))
    counts = (I >= 0).sum(dim=1)
    result["cases"][name] = {"wall": summary(walls[name]), "phases_ms": ph, "rank_mode": int(st["rank_mode"]),
                             "rank_int8": int(st["rank_int8"]), "scanned_vectors": int(st["scanned_vectors"]),
                             "mean_results_per_query": round(float(counts.float().mean().item()), 3),
                             "queries_with_fewer_than_k": int((counts < k).sum().item())}
Iu = None
step(None)
Iu = I.clone()
step(filters["100%"])
result["all_admitting_equals_unfiltered"] = bool(torch.equal(Iu, I))
slots = (args.n + 63 * index.num_centroids)   # upper bound of the padded slots (every list padded to whole blocks)
floor_bytes = (8 + 3 * 4) * slots
result["filter_creation"] = {"per_window": creation, "slots_upper_bound": slots, "hbm_floor_bytes": floor_bytes,
                             "hbm_floor_ms_at_8TBps": round(floor_bytes / 8e12 * 1e3, 4),
                             "note": "creation = allocation of the filter's arrays + one kernel + the read-back of the count, "
                                     "host wall clock; the first of a process also pays the code-object load"}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
