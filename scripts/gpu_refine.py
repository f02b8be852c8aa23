#!/usr/bin/env python3
"""Measurement (not a test): what refining a built index costs on the C2-shaped synthetic index bench.py builds (N = 1e6,
D = 128, 4096 lists: the index of scripts/gpu_add_records.py) after 100 000 drifted records were added to it, against the
only route the index had before: export every record to the host and build again at the same list count.

The drifted records come from a mixture of 16 components the base never saw (centres shifted by +25), so they pile into
the few lists nearest to those centres.  Steps, each in a child process of its own under its own time limit:
  build    the base, the add of the drifted records; list statistics before and after the add
  refine   `--repeats` times, refine(1) and refine(3) alternating, each on a fresh copy of the files: the phases
           (vi_refine_stats), the two kernels' bytes/s, the labelling rate (records x iterations / ms_label), list statistics
           and recall@10 at n_probe 8 / 32 before and after; and in the same process an upsert of as many records as the
           refine moved (update_blocks_kernel's rate)
  rebuild  export() to the host and build() of the exported records at the same list count, timed the same way, with the
           recall and the statistics of what it gives
Figures of other runs quoted beside them (`beside`) are read from their profiles (r15: export, r20: knn_graph rows/s),
not measured again.

This process never opens the GPU; nothing more is started after a child that failed or ran out of time.  Writes
profiles/r27_refine.json."""
import argparse
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
ap.add_argument("--drift", type=int, default=100_000)
ap.add_argument("--nq", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--build-timeout", type=int, default=240)
ap.add_argument("--refine-timeout", type=int, default=300)
ap.add_argument("--rebuild-timeout", type=int, default=240)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_refine.json"))
ap.add_argument("--child", choices=["build", "refine", "rebuild"], help=argparse.SUPPRESS)
ap.add_argument("--work", help=argparse.SUPPRESS)
args = ap.parse_args()


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def rate(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / 1e12, 3) if ms > 0 else None


def dataset():
    """(base rows, drifted rows, queries: half from each mixture) as numpy, and the torch device"""
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "vector-indexer_amd")]
    import bench
    dev = torch.device("cuda", 0)
    xb, qb = bench.make_dataset(args.n, args.d, args.nq // 2, 42, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(43)
    centres = torch.randn(16, args.d, generator=g, device=dev) * 30.0 + 85.0

    def draw(m):
        comp = torch.randint(0, 16, (m,), generator=g, device=dev)
        x = centres[comp] + torch.randn(m, args.d, generator=g, device=dev) * 14.0
        return torch.clamp(torch.round(x.abs()), 0, 218).to(torch.float32).contiguous()
    xd, qd = draw(args.drift), draw(args.nq - args.nq // 2)
    return xb.cpu().numpy(), xd.cpu().numpy(), torch.cat([qb, qd]).cpu().numpy()


def recall_at_10(idx, Q, gt, n_probe):
    """share of the 10 true neighbours (external ids) among the 10 returned"""
    import numpy as np
    D, I = idx.search_sync(Q, 10, n_probe)
    hit = (I[:, :, None] == gt[:, None, :]).any(axis=2).sum(axis=1)
    return round(float(hit.mean()) / 10, 4)


def ground_truth(xb, xd, Q):
    import numpy as np
    import torch
    import bench
    dev = torch.device("cuda", 0)
    allx = torch.from_numpy(np.concatenate([xb, xd])).to(dev)
    return bench.ground_truth(allx, torch.from_numpy(Q).to(dev), 10).cpu().numpy()   # row index = external id


def child_build():
    import numpy as np
    xb, xd, Q = dataset()
    import vector_indexer_py as vip
    t0 = time.perf_counter()
    base = vip.build(xb, os.path.join(args.work, "base"), nlist=args.nlist, now_secs=NOW, ext_ids=np.arange(args.n, dtype=np.uint64))
    t1 = time.perf_counter()
    before_add = base.list_stats()
    base.add(xd, ext_ids=np.arange(args.n, args.n + args.drift, dtype=np.uint64))
    out = {"kept_lists": base.num_centroids, "build_ms": round((t1 - t0) * 1e3, 1), "build_stats": base.build_stats(),
           "add_stats": base.add_stats(), "list_stats_before_add": before_add, "list_stats_after_add": base.list_stats()}
    np.save(os.path.join(args.work, "gt.npy"), ground_truth(xb, xd, Q))
    with open(os.path.join(args.work, "build.json"), "w") as fh:
        json.dump(out, fh)


def child_refine():
    import numpy as np
    xb, xd, Q = dataset()
    gt = np.load(os.path.join(args.work, "gt.npy"))
    import vector_indexer_py as vip
    base_dir = os.path.join(args.work, "base")
    n = args.n + args.drift
    runs = {1: [], 3: []}
    upserts = []
    first = None
    for r in range(args.repeats):
        for iters in (1, 3):   # alternating
            d = os.path.join(args.work, f"refine_{iters}_{r}")
            shutil.copytree(base_dir, d)
            idx = vip.load(os.path.join(d, "index"), os.path.join(d, "shards"), args.d, now_secs=NOW)
            if first is None:
                first = {"list_stats": idx.list_stats(), "recall10_p8": recall_at_10(idx, Q, gt, 8), "recall10_p32": recall_at_10(idx, Q, gt, 32)}
            t0 = time.perf_counter()
            moved = idx.refine(iters)
            wall = (time.perf_counter() - t0) * 1e3
            st = idx.refine_stats()
            st.update(wall_ms=round(wall, 2), list_stats=idx.list_stats(), recall10_p8=recall_at_10(idx, Q, gt, 8),
                      recall10_p32=recall_at_10(idx, Q, gt, 32))
            runs[iters].append(st)
            if iters == 1:   # update_blocks_kernel in the same process: an upsert of as many records as the refine moved
                rng = np.random.default_rng(5 + r)
                ids = rng.choice(np.arange(n, dtype=np.uint64), max(1, moved), replace=False)
                rows = np.ascontiguousarray(np.concatenate([xb, xd])[ids.astype(np.int64)])
                idx.upsert(rows, ids)
                upserts.append(idx.upsert_stats())
            del idx
            shutil.rmtree(d)
    phases = ("ms_total", "ms_means", "ms_label", "ms_rehome", "ms_images", "ms_files", "ms_means_kernel", "ms_rehome_kernel", "wall_ms")
    out = {"before": first, "upsert_of_moved": {"n": upserts[0]["n"], "ms_total": spread([u["ms_total"] for u in upserts]),
                                                "ms_kernel": spread([u["ms_kernel"] for u in upserts]), "kernel_bytes": upserts[0]["kernel_bytes"],
                                                "update_blocks_TBps": rate(upserts[0]["kernel_bytes"], statistics.median(u["ms_kernel"] for u in upserts))}}
    for iters, rs in runs.items():
        e = {f: spread([x[f] for x in rs]) for f in phases}
        e.update(iterations_run=rs[0]["iterations_run"], moved=rs[0]["moved"], lists_emptied=rs[0]["lists_emptied"],
                 shards_rewritten=rs[0]["shards_rewritten"], bytes_written=rs[0]["bytes_written"], means_bytes=rs[0]["means_bytes"],
                 rehome_bytes=rs[0]["rehome_bytes"], list_stats=rs[0]["list_stats"], recall10_p8=rs[0]["recall10_p8"],
                 recall10_p32=rs[0]["recall10_p32"],
                 list_means_TBps=rate(rs[0]["means_bytes"], statistics.median(x["ms_means_kernel"] for x in rs)),
                 rehome_blocks_TBps=rate(rs[0]["rehome_bytes"], statistics.median(x["ms_rehome_kernel"] for x in rs)),
                 label_rows_per_s=round(n * rs[0]["iterations_run"] / (statistics.median(x["ms_label"] for x in rs) * 1e-3)),
                 runs={f: [round(x[f], 3) for x in rs] for f in ("ms_total", "ms_means_kernel", "ms_rehome_kernel", "ms_label", "ms_files")})
        out[f"refine_{iters}"] = e
    # the gather path of list_means_kernel (iterations 2, 3) beside its streaming path (iteration 1), from the kernel sums
    m1 = statistics.median(x["ms_means_kernel"] for x in runs[1])
    m3 = statistics.median(x["ms_means_kernel"] for x in runs[3])
    out["list_means_ms_per_iteration"] = {"streaming": round(m1, 4), "gather": round((m3 - m1) / 2, 4)}
    with open(os.path.join(args.work, "refine.json"), "w") as fh:
        json.dump(out, fh)


def child_rebuild():
    import numpy as np
    xb, xd, Q = dataset()
    gt = np.load(os.path.join(args.work, "gt.npy"))
    import vector_indexer_py as vip
    base_dir = os.path.join(args.work, "base")
    runs = []
    for r in range(args.repeats):
        idx = vip.load(os.path.join(base_dir, "index"), os.path.join(base_dir, "shards"), args.d, now_secs=NOW)
        t0 = time.perf_counter()
        ext, X, ts, _ = idx.export()
        t1 = time.perf_counter()
        new = vip.build(X, os.path.join(args.work, f"rebuild_{r}"), nlist=args.nlist, now_secs=NOW, ext_ids=ext, timestamps=ts)
        t2 = time.perf_counter()
        runs.append({"export_ms": (t1 - t0) * 1e3, "build_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3, "list_stats": new.list_stats(),
                     "kept_lists": new.num_centroids, "recall10_p8": recall_at_10(new, Q, gt, 8), "recall10_p32": recall_at_10(new, Q, gt, 32)})
        del idx, new
        shutil.rmtree(os.path.join(args.work, f"rebuild_{r}"))
    out = {f: spread([x[f] for x in runs]) for f in ("export_ms", "build_ms", "total_ms")}
    out.update({f: runs[0][f] for f in ("list_stats", "kept_lists", "recall10_p8", "recall10_p32")})
    with open(os.path.join(args.work, "rebuild.json"), "w") as fh:
        json.dump(out, fh)


def run_child(step, seconds, work):
    """one GPU step in a process of its own, under its own time limit -> whether to go on"""
    cmd = [sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--d", str(args.d), "--nlist", str(args.nlist),
           "--drift", str(args.drift), "--nq", str(args.nq), "--repeats", str(args.repeats), "--child", step, "--work", work]
    try:
        rc = subprocess.run(cmd, timeout=seconds).returncode
    except subprocess.TimeoutExpired:
        print(f"{step}: no result within {seconds} s; nothing more is started", flush=True)
        return False
    if rc != 0:
        print(f"{step}: exit status {rc}; nothing more is started", flush=True)
    return rc == 0


def quoted():
    """figures of earlier runs this one is read beside, from their profiles as they stand (not measured again)"""
    out = {}
    try:
        e = json.load(open(os.path.join(ROOT, "profiles", "r15_get_records.json")))["export"]
        out["r15_export_TBps"] = {"ids_values_timestamps_where": round(e["export_GBps"] / 1e3, 3),
                                  "values_only": round(e["values_only_GBps"] / 1e3, 3), "memcpy_dtod": round(e["memcpy_dtod_GBps"] / 1e3, 3)}
    except (OSError, ValueError, KeyError):
        out["r15_export_TBps"] = None
    try:
        g = json.load(open(os.path.join(ROOT, "profiles", "r20_similar_search.json")))["b_knn_graph"]["by_chunk"]["65536"]
        out["r20_knn_graph_rows_per_s_chunk_65536"] = {k: round(v["rows_per_s"]) for k, v in g.items() if "rows_per_s" in v}
    except (OSError, ValueError, KeyError):
        out["r20_knn_graph_rows_per_s_chunk_65536"] = None
    return out


def main():
    work = tempfile.mkdtemp(prefix="vi_refine_")
    result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist}, {args.drift} drifted records added; refine(1) and refine(3) "
                          f"alternating, {args.repeats} repeats each, every run on a fresh copy of the files, one process; the rebuild "
                          "(export to the host + build at the same list count) in a process of its own",
              "beside": quoted(), "complete": False}
    try:
        ok = True
        for step, seconds in (("build", args.build_timeout), ("refine", args.refine_timeout), ("rebuild", args.rebuild_timeout)):
            ok = run_child(step, seconds, work)
            if not ok:
                break
            result[step] = json.load(open(os.path.join(work, f"{step}.json")))
            print(step, json.dumps(result[step]), flush=True)
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
    elif args.child == "refine":
        child_refine()
    elif args.child == "rebuild":
        child_rebuild()
    else:
        sys.exit(main())
