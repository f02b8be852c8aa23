#!/usr/bin/env python3
"""Measurement (not a test): what adaptive probing buys on the C2-shaped synthetic index bench.py builds (N = 1e6, D = 128,
4096 lists, k = 10, 10 000 queries per step, device entries).

(a) fixed n_probe in {4, 8, 16, 32}: recall@10, ms per step, scanned_vectors;
(b) n_probe 32 with a sweep of ratio2 and a sweep of max_codes: recall, mean p_q, scanned_vectors, ms per step and the
    HIP-event time of probe_prune_kernel (VI_PRUNE_TIMING, in passes of their own);
(c) the zero-rule adaptive call against search_device at n_probe 32: the fixed cost of the route (it alternates with the
    plain call so that drift lands on both alike);
the step time at equal recall: (b) against (a) interpolated linearly in recall between the fixed probe counts.
Wall clock per step around calls that return with their results complete; median and spread of several repeats.
Writes profiles/r26_adaptive_probe.json.  ((d), bench.py's headline on parent and branch, is run from outside and merged in
by --bench-parent / --bench-branch: files of bench.py's JSON lines, one per run.)"""
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
ap.add_argument("--bench-parent", default=None)
ap.add_argument("--bench-branch", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_adaptive_probe.json"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
xb, xq = bench.make_dataset(args.n, args.d, args.nq, 42, dev)
gt = bench.ground_truth(xb, xq, args.k)
work = tempfile.mkdtemp(prefix="vi_adaptive_")
index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000)
nq, k, P = args.nq, args.k, args.nprobe
D = torch.empty((nq, k), dtype=torch.float32, device=dev)
I = torch.empty((nq, k), dtype=torch.int64, device=dev)
Pq = torch.zeros(nq, dtype=torch.int32, device=dev)


def plain(n_probe):
    return lambda: index.search_device(xq.data_ptr(), nq, k, n_probe, D.data_ptr(), I.data_ptr(), 0)


def adaptive(rule, n_probe=P):
    return lambda: index.search_adaptive_device(xq.data_ptr(), nq, k, n_probe, rule, D.data_ptr(), I.data_ptr(), 0, Pq.data_ptr())


def wall(step):
    """ms per step: args.repeats x (warm-up + timed steps); the entries return with their results complete"""
    out = []
    for _ in range(args.repeats):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / args.steps)
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs_ms": [round(v, 4) for v in ms]}


def describe(step, rule=None):
    """recall, scanned vectors, probe counts of one step, and its timing"""
    step()
    r1, ri = bench.recalls(I, gt)
    st = index.last_stats()
    row = {"recall_at_k": round(ri, 4), "recall_1nn_at_k": round(r1, 4), "scanned_vectors": int(st["scanned_vectors"]),
           "rank_mode": int(st["rank_mode"]), "rank_int8": int(st["rank_int8"])}
    if rule is not None:
        ps = index.prune_stats()
        row["mean_p_q"] = round(ps["probes_kept"] / nq, 3)
        row["p_q_histogram"] = {str(v): int(c) for v, c in zip(*np.unique(Pq.cpu().numpy(), return_counts=True))}
        os.environ["VI_PRUNE_TIMING"] = "1"       # (a pass of its own: the two events are not in the wall-clock runs)
        t = []
        for _ in range(args.warmup + 10):
            step()
            t.append(index.prune_stats()["ms_prune"])
        del os.environ["VI_PRUNE_TIMING"]
        row["prune_kernel_ms"] = round(statistics.median(t[args.warmup:]), 4)
    row["wall"] = summary(wall(step))
    return row


result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist} k={k} nq/step={nq}; device entries, {args.steps} timed steps after "
                      f"{args.warmup} warm-up steps per run, {args.repeats} runs", "lists": index.num_centroids}

# ---- (a) fixed probe counts ----
fixed = {}
for p in (4, 8, 16, 32):
    fixed[p] = describe(plain(p))
result["a_fixed_n_probe"] = {str(p): v for p, v in fixed.items()}

# ---- (b) the two sweeps at n_probe 32 ----
result["b_ratio2_sweep"] = {}
for ratio2 in (1.05, 1.1, 1.15, 1.2, 1.3, 1.5, 2.0):
    rule = vip.ProbeRule(ratio2=ratio2)
    result["b_ratio2_sweep"][str(ratio2)] = describe(adaptive(rule), rule)
mean_len = args.n / index.num_centroids
result["b_max_codes_sweep"] = {}
for lists in (4, 8, 12, 16, 24):
    rule = vip.ProbeRule(max_codes=int(lists * mean_len))
    result["b_max_codes_sweep"][str(rule.max_codes)] = describe(adaptive(rule), rule)


def fixed_ms_at(recall):
    """the step time a fixed n_probe needs for this recall: linear between the measured probe counts; None outside them"""
    pts = sorted((v["recall_at_k"], v["wall"]["median_ms"]) for v in fixed.values())
    for (r0, m0), (r1, m1) in zip(pts[:-1], pts[1:]):
        if r0 <= recall <= r1:
            return m0 if r1 == r0 else m0 + (m1 - m0) * (recall - r0) / (r1 - r0)
    return None


for sweep in ("b_ratio2_sweep", "b_max_codes_sweep"):
    for row in result[sweep].values():
        ms = fixed_ms_at(row["recall_at_k"])
        row["fixed_n_probe_ms_at_equal_recall"] = None if ms is None else round(ms, 4)
        row["speedup_at_equal_recall"] = None if ms is None else round(ms / row["wall"]["median_ms"], 3)

# ---- (c) the fixed cost of the route: zero rule against the plain entry, alternating ----
zero = vip.ProbeRule(min_probe=0)
walls = {"search_device": [], "zero_rule": []}
for _ in range(2):
    walls["search_device"].extend(wall(plain(P)))
    walls["zero_rule"].extend(wall(adaptive(zero)))
plain(P)()
Iu, Du = I.clone(), D.clone()
adaptive(zero)()
c = {"search_device": summary(walls["search_device"]), "zero_rule": summary(walls["zero_rule"]),
     "same_result": bool(torch.equal(Iu, I) and torch.equal(Du.view(torch.int32), D.view(torch.int32)))}
c["fixed_cost_ms"] = round(c["zero_rule"]["median_ms"] - c["search_device"]["median_ms"], 4)
index.enable_timing(True)
for name, step in (("search_device", plain(P)), ("zero_rule", adaptive(zero))):
    acc = {}
    for r in range(args.warmup + 8):
        step()
        if r >= args.warmup:
            st = index.last_stats()
            for f, ph in (("ms_coarse", "coarse"), ("ms_group", "grouping"), ("ms_scan", "list_rank"), ("ms_merge", "select"), ("ms_total", "total")):
                acc.setdefault(ph, []).append(st[f])
    c[name]["phases_ms"] = {ph: round(statistics.median(v), 4) for ph, v in acc.items()}
index.enable_timing(False)
c["note"] = ("the route prunes behind the coarse step, counts the per-list histogram again and groups without the coarse select's "
             "pair ranks (no pushed work items): phases_ms.coarse holds the prune and the histogram, phases_ms.grouping the scatter")
result["c_zero_rule_fixed_cost"] = c


# ---- (d) bench.py's headline, parent and branch alternating (run from outside) ----
def bench_lines(path):
    rows = []
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            j = json.loads(line)
            rows.append({key: j[key] for key in ("ms_per_step", "qps", "value") if key in j})
    return rows


if args.bench_parent and args.bench_branch:
    result["d_bench_headline"] = {"parent": bench_lines(args.bench_parent), "branch": bench_lines(args.bench_branch),
                                  "note": "bench.py --gpus 1, five runs each, alternating parent and branch in one call"}

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
