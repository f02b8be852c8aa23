#!/usr/bin/env python3
"""Measurement (not a test): what a composed filter costs beside the chain of calls it replaces, on the C2-shaped synthetic
index bench.py builds.

The predicate: "these 1e5 ids AND this timestamp window".  Timed, in one process and on one index, host wall clock of the
call(s) that leave the filter complete, median of eight after the first:
  chain          vi_indexer_filter_timestamps + vi_indexer_filter_ids_device + vi_filter_intersect (the entries as they
                 were before compose existed: the yardstick), and each of its three calls alone
  compose        the same predicate as one vi_indexer_filter_compose call, a fresh filter every time
  compose reuse  ... written over one filter (reuse=)
  one term       compose of the window alone beside vi_indexer_filter_timestamps: the price of the generic predicate
Then one 10 000-query search at nprobe 32 through the composed and through the chained filter.
Writes profiles/r19_filter_compose.json."""
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
ap.add_argument("--ids", type=int, default=100_000)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--creations", type=int, default=9, help="creations timed per case (the first is reported apart)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_filter_compose.json"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
xb, xq = bench.make_dataset(args.n, args.d, args.nq, 42, dev)
rng = np.random.default_rng(7)
rows = np.arange(args.n, dtype=np.uint64)
ext = ((rows % np.uint64(5)) << np.uint64(40)) | (np.uint64(7) * rows + np.uint64(3))
ts = (1 + (rows * 7919) % 1000).astype(np.uint64)                                      # 1 .. 1000, uniform
work = tempfile.mkdtemp(prefix="vi_filter_compose_")
index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000, ext_ids=ext, timestamps=ts)
nq, k, P = args.nq, args.k, args.nprobe
D = torch.empty((nq, k), dtype=torch.float32, device=dev)
I = torch.empty((nq, k), dtype=torch.int64, device=dev)
WINDOW = (1, 500)
ids = rng.permutation(ext)[:min(args.ids, args.n)].copy()
ids_dev = torch.from_numpy(ids.view(np.int64)).to(dev)
want = int((np.isin(ext, ids) & (ts >= WINDOW[0]) & (ts <= WINDOW[1])).sum())
Term = vip.Term


def timed(make, keep=False):
    """host wall clock of `make()` (which returns with the filter complete), args.creations times; unless `keep`, the
    filter of the previous round is freed before the clock starts"""
    t, f = [], None
    for _ in range(args.creations):
        if not keep:
            f = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = make()
        t.append((time.perf_counter() - t0) * 1e3)
    return f, {"ms_first": round(t[0], 4), "ms_median_of_later": round(statistics.median(t[1:]), 4),
               "ms_min_of_later": round(min(t[1:]), 4), "ms_max_of_later": round(max(t[1:]), 4), "num_allowed": f.num_allowed}


def chain():
    return index.filter_timestamps(*WINDOW) & index.filter_ids_device(ids_dev.data_ptr(), ids.size)


def terms():
    return [Term.timestamps(*WINDOW), Term.ids_device(ids_dev.data_ptr(), ids.size)]


creation = {}
_, creation["warm-up: timestamps"] = timed(lambda: index.filter_timestamps(*WINDOW))   # (also pays the code-object load)
_, creation["warm-up: compose"] = timed(lambda: index.filter_compose(terms()))
fw, creation["chain: timestamps alone"] = timed(lambda: index.filter_timestamps(*WINDOW))
fi, creation["chain: ids_device alone"] = timed(lambda: index.filter_ids_device(ids_dev.data_ptr(), ids.size))
_, creation["chain: intersect alone"] = timed(lambda: fw & fi)
f_chain, creation["chain (three calls)"] = timed(chain)
f_one, creation["compose (one call, fresh)"] = timed(lambda: index.filter_compose(terms()))
target = index.filter_timestamps(*WINDOW)
_, creation["compose (one call, reuse)"] = timed(lambda: index.filter_compose(terms(), reuse=target), keep=True)
_, creation["chain (three calls), again"] = timed(chain)
_, creation["one term: timestamps entry"] = timed(lambda: index.filter_timestamps(*WINDOW))
_, creation["one term: compose"] = timed(lambda: index.filter_compose([Term.timestamps(*WINDOW)]))
_, creation["one term: compose, reuse"] = timed(lambda: index.filter_compose([Term.timestamps(*WINDOW)], reuse=target), keep=True)
index.filter_compose(terms(), reuse=target)
for name in ("chain (three calls)", "compose (one call, fresh)", "compose (one call, reuse)", "chain (three calls), again"):
    assert creation[name]["num_allowed"] == want, (name, creation[name]["num_allowed"], want)
med = lambda name: creation[name]["ms_median_of_later"]  # noqa: E731
chain_ms = min(med("chain (three calls)"), med("chain (three calls), again"))
alone_ms = med("chain: timestamps alone") + med("chain: ids_device alone") + med("chain: intersect alone")
ratios = {"compose fresh / chain": round(med("compose (one call, fresh)") / chain_ms, 3),
          "compose reuse / chain": round(med("compose (one call, reuse)") / chain_ms, 3),
          "compose fresh / sum of the chain's calls alone": round(med("compose (one call, fresh)") / alone_ms, 3),
          "compose reuse / sum of the chain's calls alone": round(med("compose (one call, reuse)") / alone_ms, 3),
          "one term: compose / timestamps entry": round(med("one term: compose") / med("one term: timestamps entry"), 3),
          "one term: compose reuse / timestamps entry": round(med("one term: compose, reuse") / med("one term: timestamps entry"), 3),
          "sum of the chain's calls alone (ms)": round(alone_ms, 4)}


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


filters = {"chained": f_chain, "composed": f_one, "composed, reused buffer": target}
walls = {}
for name in ["chained", "composed", "chained", "composed", "composed, reused buffer"]:   # (alternating: drift lands on both alike)
    walls.setdefault(name, []).extend(wall(filters[name]))
search, results = {}, {}
for name, flt in filters.items():
    step(flt)
    results[name] = (D.clone(), I.clone())
    ms = walls[name]
    search[name] = {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                    "mean_results_per_query": round(float((I >= 0).sum(dim=1).float().mean().item()), 3)}
identical = all(torch.equal(results[n][0].view(torch.int32), results["chained"][0].view(torch.int32))
                and torch.equal(results[n][1], results["chained"][1]) for n in results)
result = {"workload": f"N={args.n} D={args.d} nlist={args.nlist}; predicate: {ids.size} ids (device memory) AND timestamps in "
                      f"[{WINDOW[0]}, {WINDOW[1]}] (admits {want}); search: nprobe={P} k={k} nq/step={nq}, device entry, "
                      f"{args.steps} timed steps after {args.warmup} warm-up steps, {args.repeats} runs",
          "lists": index.num_centroids,
          "filter_creation": creation, "ratios": ratios,
          "filter_creation_note": "host wall clock of the call(s) that leave the filter complete; median of the creations after "
                                  "the first; the chain is timed twice, around the compose cases, and the ratios divide by the "
                                  "smaller of its two medians; 'reuse' keeps the target filter, every other case frees the previous "
                                  "round's filter outside the clock; 'chain (three calls)' is the chain as a caller runs it: its two "
                                  "intermediate filters are freed inside the clock (a hipFree per device buffer), which the three 'alone' cases, "
                                  "each freeing outside the clock, do not pay",
          "search": search, "composed_results_identical_to_chained": bool(identical)}
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
