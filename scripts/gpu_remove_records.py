#!/usr/bin/env python3
"""Measurement (not a test): what removing records from a built index costs on the C2-shaped synthetic index bench.py
builds (N = 1e6, D = 128, 4096 lists), against loading the files the removal wrote.

For 1 000, 10 000 and 100 000 random external ids (remove_ids) and for a timestamp window that keeps half of the records
(retain), `--repeats` times each: a copy of the base index's files is loaded, the records are removed (vi_remove_stats),
the resulting directories are loaded afresh (wall clock around vi_indexer_load), and one record is added to the shrunken
index (vi_add_stats: update_blocks_kernel's rate without a filter on the same index, in the same run).  Its HIP-event
time with the filter and the bytes it moved give its achieved bandwidth, beside the float4-copy bandwidth measured on this chip
(6.29 TB/s).  Writes profiles/r11_remove_records.json."""
import argparse
import json
import os
import shutil
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
ap.add_argument("--sizes", default="1000,10000,100000")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_remove_records.json"))
args = ap.parse_args()
sizes = [int(s) for s in args.sizes.split(",")]
COPY_TBPS = 6.29   # float4 copy, read + write bytes, measured on MI355X
NOW = 1_700_000_000

dev = torch.device("cuda", 0)
xb, pool = bench.make_dataset(args.n, args.d, 1, 42, dev)
xb, pool = xb.cpu().numpy(), pool.cpu().numpy()
ext = np.arange(args.n, dtype=np.uint64)
ts = np.uint64(1000) + (ext * np.uint64(7919)) % np.uint64(1000)      # the window [1000, 1499] keeps half
work = tempfile.mkdtemp(prefix="vi_remove_records_")
base_dir = os.path.join(work, "base")
base = vip.build(xb, base_dir, nlist=args.nlist, now_secs=NOW, ext_ids=ext, timestamps=ts)
nlists = base.num_centroids
del base
rng = np.random.default_rng(7)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def rate(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e12, 3) if ms > 0 else None


cases = [(f"remove_ids_{s}", s) for s in sizes] + [("retain_half", None)]
result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist} ({nlists} kept lists), {args.repeats} repeats per case",
          "copy_bandwidth_TBps": COPY_TBPS, "cases": {}}
for name, s in cases:
    rem, adds, loads, reloads = [], [], [], []
    for r in range(args.repeats):
        d = os.path.join(work, f"{name}_{r}")
        shutil.copytree(base_dir, d)
        dirs = (os.path.join(d, "index"), os.path.join(d, "shards"))
        t1 = time.perf_counter()
        idx = vip.load(*dirs, args.d, now_secs=NOW)
        loads.append((time.perf_counter() - t1) * 1e3)
        if s is None:
            n_removed = idx.retain(idx.filter_timestamps(1000, 1499))
        else:
            n_removed = idx.remove_ids(rng.choice(ext, s, replace=False))
        st = idx.remove_stats()
        assert st["n_removed"] == n_removed and idx.num_vectors == args.n - n_removed and (s is None or n_removed == s)
        rem.append(st)
        t1 = time.perf_counter()
        fresh = vip.load(*dirs, args.d, now_secs=NOW)
        reloads.append((time.perf_counter() - t1) * 1e3)
        assert fresh.num_vectors == idx.num_vectors
        del fresh
        idx.add(pool[:1])
        adds.append(idx.add_stats())
        del idx
        shutil.rmtree(d)
    phases = ("ms_total", "ms_plan", "ms_files", "ms_index", "ms_kernel")
    entry = {"remove": {f: spread([a[f] for a in rem]) for f in phases},
             "n_removed": rem[0]["n_removed"], "lists_touched": rem[0]["lists_touched"], "lists_emptied": rem[0]["lists_emptied"],
             "shards_rewritten": rem[0]["shards_rewritten"], "bytes_written": rem[0]["bytes_written"],
             "kernel_bytes": rem[0]["kernel_bytes"],
             "resident_half_ms": spread([a["ms_plan"] + a["ms_index"] for a in rem]),      # everything but the files
             "load_of_the_base_ms": spread(loads), "load_of_the_new_files_ms": spread(reloads),
             "append_kernel_ms": spread([a["ms_kernel"] for a in adds]), "append_kernel_bytes": adds[0]["kernel_bytes"],
             "runs": {"remove_ms_total": [round(a["ms_total"], 3) for a in rem], "remove_ms_kernel": [round(a["ms_kernel"], 4) for a in rem],
                      "reload_ms": [round(v, 3) for v in reloads], "append_ms_kernel": [round(a["ms_kernel"], 4) for a in adds]}}
    entry["kernel_TBps"] = rate(rem[0]["kernel_bytes"], statistics.median(a["ms_kernel"] for a in rem))
    entry["append_kernel_TBps"] = rate(adds[0]["kernel_bytes"], statistics.median(a["ms_kernel"] for a in adds))
    entry["remove_total_over_reload"] = round(entry["remove"]["ms_total"]["median"] / entry["load_of_the_new_files_ms"]["median"], 3)
    entry["resident_half_over_reload"] = round(entry["resident_half_ms"]["median"] / entry["load_of_the_new_files_ms"]["median"], 3)
    result["cases"][name] = entry
    print(name, json.dumps(entry), flush=True)
shutil.rmtree(work, ignore_errors=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
