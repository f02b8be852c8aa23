#!/usr/bin/env python3
"""Measurement (not a test): what an external-id filter costs on the C2-shaped synthetic index bench.py builds.

Timed, in one process and on one index: the creation of an id filter for sets of 1e3, 1e5 and all 1e6 ids, in both modes,
from host ids and from ids already in device memory; the creation of a timestamp filter (the yardstick: it streams the
same norm arrays and has no lookup); beside both, the HBM floor of the streams.  Then one 10 000-query search at nprobe
32 with allow sets admitting 100 %, 10 % and 1 % of the index, beside the unfiltered search.
Writes profiles/r06_id_filter.json."""
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
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--creations", type=int, default=9, help="creations timed per case (the first is reported apart)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_id_filter.json"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
xb, xq = bench.make_dataset(args.n, args.d, args.nq, 42, dev)
rng = np.random.default_rng(7)
rows = np.arange(args.n, dtype=np.uint64)
ext = ((rows % np.uint64(5)) << np.uint64(40)) | (np.uint64(7) * rows + np.uint64(3))   # many ids differ only above bit 32
ts = (1 + (rows * 7919) % 1000).astype(np.uint64)                                      # 1 .. 1000, uniform
work = tempfile.mkdtemp(prefix="vi_id_filter_")
index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000, ext_ids=ext, timestamps=ts)
nq, k, P = args.nq, args.k, args.nprobe
D = torch.empty((nq, k), dtype=torch.float32, device=dev)
I = torch.empty((nq, k), dtype=torch.int64, device=dev)


def timed(make):
    """host wall clock of `make()` (which returns with the filter complete), args.creations times; the filter of the
    previous round is freed before the clock starts"""
    t, f = [], None
    for _ in range(args.creations):
        f = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = make()
        t.append((time.perf_counter() - t0) * 1e3)
    return f, {"ms_first": round(t[0], 4), "ms_median_of_later": round(statistics.median(t[1:]), 4),
               "ms_min_of_later": round(min(t[1:]), 4), "ms_max_of_later": round(max(t[1:]), 4), "num_allowed": f.num_allowed}


def capacity_of(n):
    c = 2
    while c < 2 * n:
        c *= 2
    return c


slots = args.n + 63 * index.num_centroids   # upper bound of the padded slots (every list padded to whole blocks)
creation = {}
_, creation["timestamps 100%"] = timed(lambda: index.filter_timestamps(1, 1000))   # (also pays the code-object load)
_, creation["timestamps 10%"] = timed(lambda: index.filter_timestamps(1, 100))
ts_ms = creation["timestamps 10%"]["ms_median_of_later"]
sets = {}
for size in (1_000, 100_000, args.n):
    size = min(size, args.n)
    ids = rng.permutation(ext)[:size].copy()
    sets[size] = ids
    ids_dev = torch.from_numpy(ids.view(np.int64)).to(dev)
    for exclude in (False, True):
        for where in ("host", "device"):
            make = ((lambda: index.filter_ids(ids, exclude=exclude)) if where == "host"
                    else (lambda: index.filter_ids_device(ids_dev.data_ptr(), size, exclude=exclude)))
            _, c = timed(make)
            assert c["num_allowed"] == (args.n - size if exclude else size)
            floor = (8 + 3 * 4) * slots + 16 * capacity_of(size)
            c.update({"table_capacity": capacity_of(size), "hbm_floor_bytes": floor,
                      "hbm_floor_ms_at_8TBps": round(floor / 8e12 * 1e3, 4),
                      "ratio_to_timestamp_filter": round(c["ms_median_of_later"] / ts_ms, 3)})
            creation[f"ids {size} {'deny' if exclude else 'allow'} from {where}"] = c
    del ids_dev
_, creation["timestamps 10% (again, after the id filters)"] = timed(lambda: index.filter_timestamps(1, 100))


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


filters = {"unfiltered": None, "100%": index.filter_ids(ext), "10%": index.filter_ids(rng.permutation(ext)[:args.n // 10]),
           "1%": index.filter_ids(rng.permutation(ext)[:args.n // 100])}
walls = {}
for name in ["unfiltered", "100%", "unfiltered", "100%", "10%", "1%"]:   # (alternating: drift lands on both alike)
    walls.setdefault(name, []).extend(wall(filters[name]))
search = {}
for name, flt in filters.items():
    step(flt)
    counts = (I >= 0).sum(dim=1)
    ms = walls[name]
    search[name] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                    "mean_results_per_query": round(float(counts.float().mean().item()), 3),
                    "queries_with_fewer_than_k": int((counts < k).sum().item())}
step(None)
Iu = I.clone()
step(filters["100%"])
result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist}; search: nprobe={P} k={k} nq/step={nq}, device entry, "
                      f"{args.steps} timed steps after {args.warmup} warm-up steps, {args.repeats} runs",
          "lists": index.num_centroids, "slots_upper_bound": slots,
          "filter_creation": creation,
          "filter_creation_note": "creation = allocation of the filter's arrays (and of the table and, from host ids, the upload) "
                                  "+ kernels + the read-back of the count, host wall clock; ratio_to_timestamp_filter divides "
                                  "by the median of the 10 % timestamp window made in the same process; hbm floor = "
                                  "(8 + 3*4) B x slots + 16 B x table capacity",
          "search": search, "all_admitting_equals_unfiltered": bool(torch.equal(Iu, I))}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
