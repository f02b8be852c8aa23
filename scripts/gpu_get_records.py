#!/usr/bin/env python3
"""Measurement (not a test): what reading records back costs on the C2-shaped synthetic index bench.py builds
(N = 1e6, D = 128, 4096 lists: the index of scripts/gpu_add_records.py).

get: for 1, 1 000, 100 000 and 1 000 000 random stored ids, host and device forms, `--repeats` times each after one
warm-up: vi_fetch_stats' HIP-event times (ms_table / ms_match / ms_gather / ms_total) and the wall clock of the call.
Beside ms_match, the wall clock of vi_indexer_filter_ids / _device for the same set in the same run: the existing kernel
that makes the same scan of the resident external ids (it also writes a filter: 12-16 bytes per slot).

export: all records with the device form, GB/s over vi_fetch_stats.bytes_moved, beside a hipMemcpyDtoD of 4 N D bytes
timed with HIP events in the same run, and their ratio.

This process never opens the GPU: the base build, the gets and the export run in child processes of their own under a
time limit each, and nothing more is started after a child that failed or ran out of time.  Writes
profiles/r15_get_records.json."""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOW = 1_700_000_000

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--sizes", default="1,1000,100000,1000000")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--build-timeout", type=int, default=240, help="seconds for the child that builds the base")
ap.add_argument("--step-timeout", type=int, default=180, help="seconds for the child of the gets and of the export")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_get_records.json"))
ap.add_argument("--child", choices=["build", "get", "export"], help=argparse.SUPPRESS)
ap.add_argument("--work", help=argparse.SUPPRESS)
args = ap.parse_args()
sizes = [int(s) for s in args.sizes.split(",")]


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def wall_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def open_base():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "vector-indexer_amd")]
    import vector_indexer_py as vip
    base = os.path.join(args.work, "base")
    return vip.load(os.path.join(base, "index"), os.path.join(base, "shards"), args.d, now_secs=NOW)


def child_build():
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "vector-indexer_amd")]
    import bench
    import vector_indexer_py as vip
    xb, _ = bench.make_dataset(args.n, args.d, 16, 42, torch.device("cuda", 0))
    base = vip.build(xb.cpu().numpy(), os.path.join(args.work, "base"), nlist=args.nlist, now_secs=NOW,
                     ext_ids=np.arange(args.n, dtype=np.uint64))
    with open(os.path.join(args.work, "base.json"), "w") as fh:
        json.dump({"kept_lists": base.num_centroids}, fh)


def child_get():
    import numpy as np
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)   # (torch's HIP runtime has to open the GPU before the library's does)
    idx = open_base()
    idx.enable_timing(True)
    rng = np.random.default_rng(11)
    out = {}
    for s in sizes:
        ids = rng.choice(np.arange(args.n, dtype=np.uint64), s, replace=s > args.n)
        d_ids = torch.from_numpy(ids.view(np.int64)).to(dev)
        c = torch.zeros(s, dtype=torch.int32, device=dev)
        v = torch.zeros((s, args.d), dtype=torch.float32, device=dev)
        t, w = torch.zeros(s, dtype=torch.int64, device=dev), torch.zeros(s, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        forms = {"host": lambda: idx.get(ids),
                 "device": lambda: idx.get_device(d_ids.data_ptr(), s, c.data_ptr(), v.data_ptr(), t.data_ptr(), w.data_ptr()),
                 "device_contains": lambda: idx.get_device(d_ids.data_ptr(), s, c.data_ptr())}
        entry = {}
        for form, call in forms.items():
            call()   # warm-up: the context's buffers are reserved here
            runs = []
            for _ in range(args.repeats):
                ms = wall_ms(call)
                st = idx.fetch_stats()
                assert st["n"] == s and st["n_found"] == s
                runs.append(dict(wall_ms=ms, **{f: st[f] for f in ("ms_total", "ms_table", "ms_match", "ms_gather")}))
            entry[form] = {f: spread([r[f] for r in runs]) for f in runs[0]}
            entry[form]["bytes_moved"] = st["bytes_moved"]
        filt = {"filter_ids_wall_ms": [], "filter_ids_device_wall_ms": []}
        for _ in range(args.repeats + 1):
            filt["filter_ids_wall_ms"].append(wall_ms(lambda: idx.filter_ids(ids)))
            filt["filter_ids_device_wall_ms"].append(wall_ms(lambda: idx.filter_ids_device(d_ids.data_ptr(), s)))
        entry["same_scan_by_the_id_filter"] = {k: spread(v[1:]) for k, v in filt.items()}
        out[str(s)] = entry
        print(s, json.dumps(entry), flush=True)
    with open(os.path.join(args.work, "get.json"), "w") as fh:
        json.dump(out, fh)


def child_export():
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)   # (torch's HIP runtime has to open the GPU before the library's does)
    idx = open_base()
    idx.enable_timing(True)
    n, d = idx.num_vectors, args.d
    e, t, w = (torch.zeros(n, dtype=torch.int64, device=dev) for _ in range(3))
    v = torch.zeros((n, d), dtype=torch.float32, device=dev)
    src = torch.ones((n, d), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoD.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    runs, copies = [], []
    for r in range(args.repeats + 1):
        ms = wall_ms(lambda: idx.export_device(0, n, e.data_ptr(), v.data_ptr(), t.data_ptr(), w.data_ptr()))
        st = idx.fetch_stats()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert hip.hipMemcpyDtoD(v.data_ptr(), src.data_ptr(), 4 * n * d) == 0
        b.record()
        torch.cuda.synchronize()
        if r:   # (the first round warms both up)
            runs.append(dict(wall_ms=ms, ms_gather=st["ms_gather"], ms_total=st["ms_total"]))
            copies.append(a.elapsed_time(b))
    values_only = []
    for r in range(args.repeats + 1):
        idx.export_device(0, n, 0, v.data_ptr())
        values_only.append(idx.fetch_stats()["ms_gather"])
    kernel_ms, copy_ms = statistics.median(x["ms_gather"] for x in runs), statistics.median(copies)
    out = {"records": n, "bytes_moved": st["bytes_moved"], "export": {f: spread([x[f] for x in runs]) for f in runs[0]},
           "export_GBps": round(st["bytes_moved"] / (kernel_ms * 1e-3) / 1e9, 1),
           "values_only_ms_gather": spread(values_only[1:]),
           "values_only_GBps": round(8 * n * d / (statistics.median(values_only[1:]) * 1e-3) / 1e9, 1),
           "memcpy_dtod_bytes": 4 * n * d, "memcpy_dtod_ms": spread(copies),
           "memcpy_dtod_GBps": round(8 * n * d / (copy_ms * 1e-3) / 1e9, 1)}   # (a copy reads and writes its bytes)
    out["export_over_memcpy"] = round(out["export_GBps"] / out["memcpy_dtod_GBps"], 3)
    out["values_only_over_memcpy"] = round(out["values_only_GBps"] / out["memcpy_dtod_GBps"], 3)
    with open(os.path.join(args.work, "export.json"), "w") as fh:
        json.dump(out, fh)
    print("export", json.dumps(out), flush=True)


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
    work = tempfile.mkdtemp(prefix="vi_get_records_")
    result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist}, {args.repeats} repeats after one warm-up; ids drawn "
                          "from the stored ones; one process for the gets, one for the export",
              "get": {}, "export": {}, "complete": False}
    try:
        ok = run_child(["--child", "build", "--work", work], args.build_timeout)
        if ok:
            result["kept_lists"] = json.load(open(os.path.join(work, "base.json")))["kept_lists"]
            ok = run_child(["--child", "get", "--work", work], args.step_timeout)
        if ok:
            result["get"] = json.load(open(os.path.join(work, "get.json")))
            ok = run_child(["--child", "export", "--work", work], args.step_timeout)
        if ok:
            result["export"] = json.load(open(os.path.join(work, "export.json")))
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
    elif args.child == "get":
        child_get()
    elif args.child == "export":
        child_export()
    else:
        sys.exit(main())
