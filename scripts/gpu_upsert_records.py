#!/usr/bin/env python3
"""Measurement (not a test): what upserting records in a built index costs on the C2-shaped synthetic index bench.py
builds (N = 1e6, D = 128, 4096 lists: the index of scripts/gpu_add_records.py), against the two calls it replaces.

For 1 000, 10 000 and 100 000 random external ids with new rows from the mixture the base was drawn from, `--repeats`
times each: a copy of the base index's files is loaded and the records are upserted (vi_upsert_stats); a second copy is
loaded and the same ids and rows go through remove_ids() and add() (vi_remove_stats + vi_add_stats), in the same process.
The first repeat of every size also compares the shard files the two ways wrote.  The three block kernels' HIP-event
times and the bytes they moved give their rates in the same run.

The yardstick is the pair; DESIGN §4i states what is expected of the comparison before it was measured, and this script
reports both expectations as they fall (`expectations`), with every run's own figures.

This process never opens the GPU: the base build and every size run in a child process of their own under a time limit,
and nothing more is started after a child that failed or ran out of time.  Writes profiles/r13_upsert_records.json."""
import argparse
import filecmp
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOW = 1_700_000_000

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--sizes", default="1000,10000,100000")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--build-timeout", type=int, default=240, help="seconds for the child that builds the base")
ap.add_argument("--size-timeout", type=int, default=180, help="seconds for the child of one size")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_upsert_records.json"))
ap.add_argument("--child", choices=["build", "size"], help=argparse.SUPPRESS)
ap.add_argument("--work", help=argparse.SUPPRESS)
ap.add_argument("--size", type=int, help=argparse.SUPPRESS)
args = ap.parse_args()
sizes = [int(s) for s in args.sizes.split(",")]


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def rate(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e12, 3) if ms > 0 else None


def dataset():
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "vector-indexer_amd")]
    import bench
    xb, pool = bench.make_dataset(args.n, args.d, max(sizes), 42, torch.device("cuda", 0))
    return xb.cpu().numpy(), pool.cpu().numpy()


def child_build():
    import numpy as np
    xb, _ = dataset()
    import vector_indexer_py as vip
    base = vip.build(xb, os.path.join(args.work, "base"), nlist=args.nlist, now_secs=NOW, ext_ids=np.arange(args.n, dtype=np.uint64))
    with open(os.path.join(args.work, "base.json"), "w") as fh:
        json.dump({"kept_lists": base.num_centroids}, fh)


def child_size():
    import numpy as np
    _, pool = dataset()
    import vector_indexer_py as vip
    s = args.size
    base_dir = os.path.join(args.work, "base")
    rng = np.random.default_rng(7 + s)
    ups, rems, adds = [], [], []
    same_files = None
    for r in range(args.repeats):
        ids = rng.choice(np.arange(args.n, dtype=np.uint64), s, replace=False)
        rows = np.ascontiguousarray(pool[:s])
        d_up, d_pair = os.path.join(args.work, f"upsert_{s}_{r}"), os.path.join(args.work, f"pair_{s}_{r}")
        shutil.copytree(base_dir, d_up)
        shutil.copytree(base_dir, d_pair)
        idx = vip.load(os.path.join(d_up, "index"), os.path.join(d_up, "shards"), args.d, now_secs=NOW)
        assert idx.upsert(rows, ids) == s and idx.num_vectors == args.n
        ups.append(idx.upsert_stats())
        del idx
        idx = vip.load(os.path.join(d_pair, "index"), os.path.join(d_pair, "shards"), args.d, now_secs=NOW)
        assert idx.remove_ids(ids) == s
        idx.add(rows, ext_ids=ids)
        assert idx.num_vectors == args.n
        rems.append(idx.remove_stats())
        adds.append(idx.add_stats())
        del idx
        if r == 0:
            names = sorted(os.listdir(os.path.join(d_up, "shards")))
            _, differ, errors = filecmp.cmpfiles(os.path.join(d_up, "shards"), os.path.join(d_pair, "shards"), names, shallow=False)
            same_files = not differ and not errors and names == sorted(os.listdir(os.path.join(d_pair, "shards")))
        shutil.rmtree(d_up)
        shutil.rmtree(d_pair)
    pair_total = [a["ms_total"] + b["ms_total"] for a, b in zip(rems, adds)]
    phases = ("ms_total", "ms_plan", "ms_files", "ms_index", "ms_kernel")
    entry = {"upsert": {f: spread([u[f] for u in ups]) for f in phases},
             "pair_ms_total": spread(pair_total),
             "pair_remove": {f: spread([a[f] for a in rems]) for f in ("ms_total", "ms_files", "ms_index", "ms_kernel")},
             "pair_add": {f: spread([a[f] for a in adds]) for f in ("ms_total", "ms_files", "ms_index", "ms_kernel")},
             "n_replaced": ups[0]["n_replaced"], "lists_touched": ups[0]["lists_touched"], "lists_emptied": ups[0]["lists_emptied"],
             "shards_rewritten": ups[0]["shards_rewritten"], "bytes_written": ups[0]["bytes_written"],
             "pair_bytes_written": rems[0]["bytes_written"] + adds[0]["bytes_written"],
             "files_equal_first_repeat": same_files,
             "kernel_bytes": {"update": ups[0]["kernel_bytes"], "compact": rems[0]["kernel_bytes"], "append": adds[0]["kernel_bytes"]},
             "kernel_TBps": {"update": rate(ups[0]["kernel_bytes"], statistics.median(u["ms_kernel"] for u in ups)),
                             "compact": rate(rems[0]["kernel_bytes"], statistics.median(a["ms_kernel"] for a in rems)),
                             "append": rate(adds[0]["kernel_bytes"], statistics.median(a["ms_kernel"] for a in adds))},
             "runs": {"upsert_ms_total": [round(u["ms_total"], 3) for u in ups], "pair_ms_total": [round(v, 3) for v in pair_total],
                      "update_ms_kernel": [round(u["ms_kernel"], 4) for u in ups],
                      "compact_ms_kernel": [round(a["ms_kernel"], 4) for a in rems],
                      "append_ms_kernel": [round(a["ms_kernel"], 4) for a in adds]}}
    t = entry["kernel_TBps"]
    entry["expectations"] = {
        "upsert_below_pair_with_disjoint_ranges": entry["upsert"]["ms_total"]["max"] < entry["pair_ms_total"]["min"],
        "update_rate_between_append_and_compact": None if None in t.values() else
        min(t["append"], t["compact"]) <= t["update"] <= max(t["append"], t["compact"])}
    entry["upsert_over_pair"] = round(entry["upsert"]["ms_total"]["median"] / entry["pair_ms_total"]["median"], 3)
    with open(os.path.join(args.work, f"size_{s}.json"), "w") as fh:
        json.dump(entry, fh)


def run_child(extra, seconds):
    """one GPU step in a process of its own, under its own time limit -> whether to go on"""
    cmd = [sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--d", str(args.d), "--nlist", str(args.nlist),
           "--sizes", args.sizes, "--repeats", str(args.repeats)] + extra
    try:
        rc = subprocess.run(cmd, timeout=seconds).returncode
    except subprocess.TimeoutExpired:
        print(f"{extra}: no result within {seconds} s; nothing more is started", flush=True)
        return False
    if rc != 0:
        print(f"{extra}: exit status {rc}; nothing more is started", flush=True)
    return rc == 0


def main():
    work = tempfile.mkdtemp(prefix="vi_upsert_records_")
    result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist}, {args.repeats} repeats per size; upsert and the "
                          "remove_ids + add pair on copies of the same files, same ids and rows, one process per size",
              "sizes": {}, "complete": False}
    try:
        ok = run_child(["--child", "build", "--work", work], args.build_timeout)
        if ok:
            result["kept_lists"] = json.load(open(os.path.join(work, "base.json")))["kept_lists"]
        for s in sizes:
            if not ok:
                break
            ok = run_child(["--child", "size", "--size", str(s), "--work", work], args.size_timeout)
            if ok:
                result["sizes"][str(s)] = json.load(open(os.path.join(work, f"size_{s}.json")))
                print(s, json.dumps(result["sizes"][str(s)]), flush=True)
        result["complete"] = ok
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps(result))
    return 0 if result["complete"] else 1


if __name__ == "__main__":
    if args.child == "build":
        child_build()
    elif args.child == "size":
        child_size()
    else:
        sys.exit(main())
