#!/usr/bin/env python3
"""Measurement (not a test): what adding records to a built index costs on the C2-shaped synthetic index bench.py builds
(N = 1e6, D = 128, 4096 lists), against building the final set from scratch.

For 1 000, 10 000 and 100 000 added records, `--repeats` times each: a copy of the base index's files is loaded, the
records are added (vi_add_stats), and the same final set is built in full (ms_total and ms_index of vi_build_stats).  The
added records come from the mixture the base was drawn from.  update_blocks_kernel's HIP-event time and the bytes it moved
give its achieved bandwidth, beside the float4-copy bandwidth measured on this chip (6.29 TB/s).
Writes profiles/r09_add_records.json."""
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
ap.add_argument("--skip-rebuild", action="store_true", help="adds only (the full builds take most of the run)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_add_records.json"))
args = ap.parse_args()
sizes = [int(s) for s in args.sizes.split(",")]
COPY_TBPS = 6.29   # float4 copy, read + write bytes, measured on MI355X

dev = torch.device("cuda", 0)
xb, pool = bench.make_dataset(args.n, args.d, max(sizes), 42, dev)
xb, pool = xb.cpu().numpy(), pool.cpu().numpy()
work = tempfile.mkdtemp(prefix="vi_add_records_")
base_dir = os.path.join(work, "base")
base = vip.build(xb, base_dir, nlist=args.nlist, now_secs=1_700_000_000)
base_stats = base.build_stats()
nlists = base.num_centroids
del base


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist} ({nlists} kept lists), {args.repeats} repeats per size",
          "base_build": {f: round(base_stats[f], 3) if isinstance(base_stats[f], float) else base_stats[f] for f in base_stats},
          "copy_bandwidth_TBps": COPY_TBPS, "sizes": {}}
for s in sizes:
    adds, rebuilds, loads = [], [], []
    for r in range(args.repeats):
        d = os.path.join(work, f"add_{s}_{r}")
        shutil.copytree(base_dir, d)
        t1 = time.perf_counter()
        idx = vip.load(os.path.join(d, "index"), os.path.join(d, "shards"), args.d, now_secs=1_700_000_000)
        loads.append((time.perf_counter() - t1) * 1e3)
        idx.add(pool[:s])
        st = idx.add_stats()
        assert st["n"] == s and idx.num_vectors == args.n + s
        adds.append(st)
        del idx
        shutil.rmtree(d)
        if not args.skip_rebuild:
            d = os.path.join(work, f"full_{s}_{r}")
            full = vip.build(np.concatenate([xb, pool[:s]]), d, nlist=args.nlist, now_secs=1_700_000_000)
            bs = full.build_stats()
            rebuilds.append(bs)
            del full
            shutil.rmtree(d)
    entry = {"add": {f: spread([a[f] for a in adds]) for f in ("ms_total", "ms_assign", "ms_files", "ms_index", "ms_kernel")},
             "lists_touched": adds[0]["lists_touched"], "shards_rewritten": adds[0]["shards_rewritten"],
             "bytes_written": adds[0]["bytes_written"], "kernel_bytes": adds[0]["kernel_bytes"],
             "load_of_the_base_ms": spread(loads),
             # every run's own figures (what a comparison of two commits takes its medians and maxima from)
             "runs": {"load_ms": [round(v, 3) for v in loads], "add_ms_index": [round(a["ms_index"], 3) for a in adds],
                      "add_ms_kernel": [round(a["ms_kernel"], 4) for a in adds],
                      "rebuild_ms_index": [round(b["ms_index"], 3) for b in rebuilds]}}
    kms = statistics.median(a["ms_kernel"] for a in adds)
    entry["kernel_TBps"] = round(adds[0]["kernel_bytes"] / (kms * 1e-3) / 1e12, 3) if kms > 0 else None
    entry["kernel_share_of_copy_bandwidth"] = round(entry["kernel_TBps"] / COPY_TBPS, 3) if kms > 0 else None
    if rebuilds:
        entry["rebuild"] = {f: spread([b[f] for b in rebuilds]) for f in ("ms_total", "ms_kmeans", "ms_export", "ms_index")}
        entry["add_total_over_rebuild_total"] = round(entry["add"]["ms_total"]["median"] / entry["rebuild"]["ms_total"]["median"], 4)
        entry["add_index_over_rebuild_index"] = round(entry["add"]["ms_index"]["median"] / entry["rebuild"]["ms_index"]["median"], 4)
    result["sizes"][str(s)] = entry
    print(s, json.dumps(entry), flush=True)
shutil.rmtree(work, ignore_errors=True)
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
