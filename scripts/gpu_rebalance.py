#!/usr/bin/env python3
"""Measurement (not a test): what the split step of a rebalance costs and how close to a fresh build's balance it gets, at
the point scripts/gpu_refine.py measures a refine at: the C2-shaped synthetic index bench.py builds (N = 1e6, D = 128, 4096
lists) after 100 000 drifted records were added to it.

Steps, each in a child process of its own under its own time limit, every run on a fresh copy of the files:
  build     the base, the add of the drifted records, queries and ground truth
  run       one call and what it leaves: the phases (vi_rebalance_stats / vi_refine_stats), list statistics, recall@10 at
            n_probe 8.  Variants:
              refine1   refine(1)                                      (with --parent-package: by that build of the package)
              rounds0   rebalance(iters = 1, split_rounds = 0): the same code path
              default   rebalance() with vi_rebalance_rule_init's rule
              three     rebalance(iters = split_rounds = 3, receiver_max_len = 1)
            refine1 and rounds0 alternate `--repeats` times; rounds0 is "inside" when its median ms_total lies within the
            range of refine1's runs.
  rebuild   export() to the host and build() of the exported records at the same list count

--parent-package DIR: a directory that holds another build's vector_indexer_py and libvi_amd.so (the commit before this
call existed); refine1 then runs with it.  Without it refine1 runs with this build.

This process never opens the GPU; nothing more is started after a child that failed or ran out of time.  Writes
profiles/r29_rebalance.json."""
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
VARIANTS = ("refine1", "rounds0", "default", "three")

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=128)
ap.add_argument("--nlist", type=int, default=4096)
ap.add_argument("--drift", type=int, default=100_000)
ap.add_argument("--nq", type=int, default=2000)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--parent-package", default=None)
ap.add_argument("--build-timeout", type=int, default=240)
ap.add_argument("--run-timeout", type=int, default=120)
ap.add_argument("--rebuild-timeout", type=int, default=240)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_rebalance.json"))
ap.add_argument("--child", choices=["build", "run", "rebuild"], help=argparse.SUPPRESS)
ap.add_argument("--variant", choices=VARIANTS, help=argparse.SUPPRESS)
ap.add_argument("--work", help=argparse.SUPPRESS)
args = ap.parse_args()


def package(parent=False):
    sys.path[:0] = [ROOT, args.parent_package if parent and args.parent_package else os.path.join(ROOT, "vector-indexer_amd")]
    import vector_indexer_py as vip
    return vip


def recall_at_10(idx, Q, gt, n_probe):
    D, I = idx.search_sync(Q, 10, n_probe)
    hit = (I[:, :, None] == gt[:, None, :]).any(axis=2).sum(axis=1)
    return round(float(hit.mean()) / 10, 4)


def child_build():
    import numpy as np
    import torch
    vip = package()
    import bench
    dev = torch.device("cuda", 0)
    xb, qb = bench.make_dataset(args.n, args.d, args.nq // 2, 42, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(43)
    centres = torch.randn(16, args.d, generator=g, device=dev) * 30.0 + 85.0   # (the drift of scripts/gpu_refine.py)

    def draw(m):
        comp = torch.randint(0, 16, (m,), generator=g, device=dev)
        x = centres[comp] + torch.randn(m, args.d, generator=g, device=dev) * 14.0
        return torch.clamp(torch.round(x.abs()), 0, 218).to(torch.float32).contiguous()
    xd, qd = draw(args.drift), draw(args.nq - args.nq // 2)
    Q = torch.cat([qb, qd])
    gt = bench.ground_truth(torch.cat([xb, xd]), Q, 10).cpu().numpy()   # row index = external id
    base = vip.build(xb.cpu().numpy(), os.path.join(args.work, "base"), nlist=args.nlist, now_secs=NOW, ext_ids=np.arange(args.n, dtype=np.uint64))
    base.add(xd.cpu().numpy(), ext_ids=np.arange(args.n, args.n + args.drift, dtype=np.uint64))
    np.save(os.path.join(args.work, "gt.npy"), gt)
    np.save(os.path.join(args.work, "Q.npy"), Q.cpu().numpy())
    out = {"kept_lists": base.num_centroids, "list_stats": base.list_stats(), "recall10_p8": recall_at_10(base, Q.cpu().numpy(), gt, 8)}
    with open(os.path.join(args.work, "build.json"), "w") as fh:
        json.dump(out, fh)


def child_run():
    import numpy as np
    v = args.variant
    vip = package(parent=v == "refine1")
    Q, gt = np.load(os.path.join(args.work, "Q.npy")), np.load(os.path.join(args.work, "gt.npy"))
    d = os.path.join(args.work, "run")
    shutil.copytree(os.path.join(args.work, "base"), d)
    idx = vip.load(os.path.join(d, "index"), os.path.join(d, "shards"), args.d, now_secs=NOW)
    idx.search_sync(Q[:64], 10, 8)   # (the first search of a process pays for its workspaces)
    t0 = time.perf_counter()
    if v == "refine1":
        moved = idx.refine(1)
    elif v == "rounds0":
        moved = idx.rebalance(iters=1, split_rounds=0)
    elif v == "default":
        moved = idx.rebalance()
    else:
        moved = idx.rebalance(iters=3, split_rounds=3, receiver_max_len=1)
    wall = (time.perf_counter() - t0) * 1e3
    st = idx.refine_stats() if v == "refine1" else idx.rebalance_stats()
    st.update(variant=v, returned=moved, wall_ms=round(wall, 2), list_stats=idx.list_stats(), recall10_p8=recall_at_10(idx, Q, gt, 8))
    del idx
    shutil.rmtree(d)
    with open(os.path.join(args.work, "run.json"), "w") as fh:
        json.dump(st, fh)


def child_rebuild():
    import numpy as np
    vip = package()
    Q, gt = np.load(os.path.join(args.work, "Q.npy")), np.load(os.path.join(args.work, "gt.npy"))
    base_dir = os.path.join(args.work, "base")
    idx = vip.load(os.path.join(base_dir, "index"), os.path.join(base_dir, "shards"), args.d, now_secs=NOW)
    t0 = time.perf_counter()
    ext, X, ts, _ = idx.export()
    new = vip.build(X, os.path.join(args.work, "rebuild"), nlist=args.nlist, now_secs=NOW, ext_ids=ext, timestamps=ts)
    total = (time.perf_counter() - t0) * 1e3
    out = {"total_ms": round(total, 1), "list_stats": new.list_stats(), "kept_lists": new.num_centroids, "recall10_p8": recall_at_10(new, Q, gt, 8)}
    with open(os.path.join(args.work, "rebuild.json"), "w") as fh:
        json.dump(out, fh)


def run_child(step, seconds, work, variant=None):
    """one GPU step in a process of its own, under its own time limit -> whether to go on"""
    cmd = [sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--d", str(args.d), "--nlist", str(args.nlist),
           "--drift", str(args.drift), "--nq", str(args.nq), "--child", step, "--work", work]
    if variant:
        cmd += ["--variant", variant]
    if args.parent_package:
        cmd += ["--parent-package", os.path.abspath(args.parent_package)]
    try:
        rc = subprocess.run(cmd, timeout=seconds).returncode
    except subprocess.TimeoutExpired:
        print(f"{step} {variant or ''}: no result within {seconds} s; nothing more is started", flush=True)
        return False
    if rc != 0:
        print(f"{step} {variant or ''}: exit status {rc}; nothing more is started", flush=True)
    return rc == 0


PHASES = ("ms_total", "ms_means", "ms_label", "ms_rehome", "ms_images", "ms_files", "ms_means_kernel", "ms_rehome_kernel", "ms_split",
          "ms_split_kernels", "wall_ms")


def summary(runs):
    e = {f: {"median": round(statistics.median(x[f] for x in runs), 3), "runs": [round(x[f], 3) for x in runs]} for f in PHASES if f in runs[0]}
    for f in ("iterations_run", "moved", "lists_emptied", "pairs_planned", "splits_done", "splits_skipped", "inner_iterations", "split_bytes",
              "means_bytes", "list_stats", "recall10_p8"):
        if f in runs[0]:
            e[f] = runs[0][f]
    return e


def main():
    work = tempfile.mkdtemp(prefix="vi_rebalance_")
    result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist}, {args.drift} drifted records added; every run in a process of its own on a "
                          f"fresh copy of the files; refine1 and rounds0 alternate {args.repeats} times, default and three run twice",
              "refine1_build": "the parent package given on the command line" if args.parent_package else "this build", "complete": False}
    plan = [v for _ in range(args.repeats) for v in ("refine1", "rounds0")] + ["default", "three", "default", "three"]
    runs = {v: [] for v in VARIANTS}
    try:
        ok = run_child("build", args.build_timeout, work)
        if ok:
            result["before"] = json.load(open(os.path.join(work, "build.json")))
            print("build", json.dumps(result["before"]), flush=True)
        for v in plan:
            if not ok:
                break
            ok = run_child("run", args.run_timeout, work, v)
            if ok:
                runs[v].append(json.load(open(os.path.join(work, "run.json"))))
                print(v, json.dumps(runs[v][-1]), flush=True)
        if ok:
            ok = run_child("rebuild", args.rebuild_timeout, work)
            if ok:
                result["rebuild"] = json.load(open(os.path.join(work, "rebuild.json")))
                print("rebuild", json.dumps(result["rebuild"]), flush=True)
        for v in VARIANTS:
            if runs[v]:
                result[v] = summary(runs[v])
        if runs["refine1"] and runs["rounds0"]:
            lo, hi = min(x["ms_total"] for x in runs["refine1"]), max(x["ms_total"] for x in runs["refine1"])
            med = statistics.median(x["ms_total"] for x in runs["rounds0"])
            result["rounds0_inside_refine1_range"] = {"refine1_min": round(lo, 3), "refine1_max": round(hi, 3), "rounds0_median": round(med, 3),
                                                      "inside": bool(lo <= med <= hi)}
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
    elif args.child == "run":
        child_run()
    elif args.child == "rebuild":
        child_rebuild()
    else:
        sys.exit(main())
