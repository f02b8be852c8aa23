#!/usr/bin/env python3
"""Measure the exact (flat) inner-product search on the bench index and write profiles/r34_exact_ip.json.

On the benchmark's shape (N = 1e6, D = 128, 4096 lists, 10 000 device-resident queries, k = 10; --n / --nq / --nlist shrink
it) and on a norm-spread copy of it (every row scaled by a factor drawn from {0.25, 1, 4}) it records, --repeats calls each
(host clock around calls that end synchronised, after a warm-up call; min and max),
  * search_exact_ip_device, and in a separate call under VI_EXACT_TIMING its phases, survivors and candidates per query
    and the overflow rows (recorded, not asserted);
  * the only route before: a torch fp32 matmul + topk over the exported rows, in chunks of 131 072 rows;
  * search_exact_device (the L2 sweep of the parent) on the same handle;
  * the rows whose ids differ from the matmul's (near-ties of the matmul form), and the sweep's rate against the bf16 peak.
With --ladder it measures the score-seeded ladder instead and writes profiles/r36_exact_ip_seed.json: on both
data sets the call with VI_EXACT_IP_LADDER=0 (the path before the ladder) and =1 in one process, the matmul route, the
phases (seed / ladder / sweep / finish), the schedule, per-level survivors and candidates per query against k r, the level
overflows, the final sweep's counts and overflow rows; k = 1 and 128 on the bench data as secondary points.
Needs an MI355X; nothing here falls back to the CPU."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vector-indexer_amd")]


def timed(fn, sync, repeats):
    out = []
    for _ in range(repeats):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return [min(out), max(out)]


def matmul_topk(rows, ids, xq, k):
    """the k largest q.v per query by fp32 matmul + topk -> external ids"""
    import torch
    best_s = torch.full((xq.shape[0], k), float("-inf"), device=xq.device)
    best_i = torch.full((xq.shape[0], k), -1, dtype=torch.int64, device=xq.device)
    for s in range(0, rows.shape[0], 131072):
        blk = rows[s:s + 131072]
        ss, ii = torch.topk(xq @ blk.T, min(k, blk.shape[0]), dim=1, largest=True)
        cat_s, cat_i = torch.cat([best_s, ss], 1), torch.cat([best_i, ids[s:s + 131072][ii]], 1)
        sel = torch.topk(cat_s, k, dim=1, largest=True)
        best_s, best_i = sel.values, torch.gather(cat_i, 1, sel.indices)
    return best_i


def measure(vip, torch, bench, xb, xq, args, dev):
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    nq, k, res = xq.shape[0], args.k, {}
    with tempfile.TemporaryDirectory() as work:
        index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000)
        n = index.num_vectors
        rows = torch.empty((n, args.d), dtype=torch.float32, device=dev)
        ids = torch.empty(n, dtype=torch.int64, device=dev)
        index.export_device(0, n, ids.data_ptr(), rows.data_ptr())
        S = torch.empty((nq, k), dtype=torch.float32, device=dev)
        I = torch.empty((nq, k), dtype=torch.int64, device=dev)
        D2, I2 = torch.empty_like(S), torch.empty_like(I)
        ip = lambda: index.search_exact_ip_device(xq.data_ptr(), nq, k, S.data_ptr(), I.data_ptr())  # noqa: E731
        l2 = lambda: index.search_exact_device(xq.data_ptr(), nq, k, D2.data_ptr(), I2.data_ptr())  # noqa: E731
        ip(), l2(), matmul_topk(rows, ids, xq, k)  # warm-up: code objects, workspaces
        res["exact_ip_ms"] = timed(ip, sync, args.repeats)
        res["exact_l2_ms"] = timed(l2, sync, args.repeats)
        res["matmul_topk_ms"] = timed(lambda: matmul_topk(rows, ids, xq, k), sync, args.repeats)
        os.environ["VI_EXACT_TIMING"] = "1"
        ip()
        st = index.exact_ip_stats()
        l2()
        st2 = index.exact_stats()
        del os.environ["VI_EXACT_TIMING"]
        res["exact_ip_phases"] = {f: st[f] for f in ("ms_seed", "ms_sweep", "ms_finish", "ms_total")}
        res["exact_l2_phases"] = {f: st2[f] for f in ("ms_seed", "ms_sweep", "ms_finish", "ms_total")}
        for name, s in (("exact_ip_counts", st), ("exact_l2_counts", st2)):
            res[name] = {"survivors_per_query": s["survivors"] / nq, "candidates_per_query": s["candidates"] / nq,
                         "overflow_rows": s["overflow_rows"], "seed_probe": s["seed_probe"], "cand_cap": s["cand_cap"],
                         "query_tile": s["query_tile"], "block_splits": s["block_splits"]}
        # the sweep's multiply-adds: N D per query and bf16 product, 2 products where every stored value is bf16-exact, else 3
        res["sweep_tflops_2_products"] = 2 * 2.0 * n * args.d * (nq - st["overflow_rows"]) / (st["ms_sweep"] * 1e-3) / 1e12
        res["bf16_peak_tflops"] = bench.MFMA_BF16_PEAK_TF
        # the same call with the widest candidate arrays the finish sorts in LDS: fewer overflow rows for 64 KB per query
        wide = lambda: index.search_exact_ip_device(xq.data_ptr(), nq, k, D2.data_ptr(), I2.data_ptr(), opts={"cand_cap": 8192})  # noqa: E731
        wide()
        res["exact_ip_cand_cap_8192"] = {"ms": timed(wide, sync, args.repeats), "overflow_rows": index.exact_ip_stats()["overflow_rows"],
                                         "equal": bool((I2 == I).all().item() and (D2.view(torch.int32) == S.view(torch.int32)).all().item())}
        gt = matmul_topk(rows, ids, xq, k)
        res["matmul_rows_differing"] = int((gt != I).any(dim=1).sum().item())
        res["ratio_ip_to_matmul"] = res["exact_ip_ms"][0] / res["matmul_topk_ms"][0]
        res["ratio_ip_to_l2"] = res["exact_ip_ms"][0] / res["exact_l2_ms"][0]
    return res


def measure_ladder(vip, torch, xb, xq, args, dev, ks):
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    nq, res = xq.shape[0], {}
    with tempfile.TemporaryDirectory() as work:
        index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000)
        n = index.num_vectors
        rows = torch.empty((n, args.d), dtype=torch.float32, device=dev)
        ids = torch.empty(n, dtype=torch.int64, device=dev)
        index.export_device(0, n, ids.data_ptr(), rows.data_ptr())
        for k in ks:
            S = {m: torch.empty((nq, k), dtype=torch.float32, device=dev) for m in "01"}
            I = {m: torch.empty((nq, k), dtype=torch.int64, device=dev) for m in "01"}
            point = {}
            for mode in "01":
                os.environ["VI_EXACT_IP_LADDER"] = mode
                ip = lambda: index.search_exact_ip_device(xq.data_ptr(), nq, k, S[mode].data_ptr(), I[mode].data_ptr())  # noqa: E731
                ip()
                r = {"ms": timed(ip, sync, args.repeats)}
                os.environ["VI_EXACT_TIMING"] = "1"
                ip()
                del os.environ["VI_EXACT_TIMING"]
                st, ss = index.exact_ip_stats(), index.exact_ip_seed_stats()
                r["phases"] = {"ms_seed": st["ms_seed"], "ms_ladder": ss["ms_ladder"], "ms_sweep": st["ms_sweep"], "ms_finish": st["ms_finish"]}
                r["final_sweep"] = {"survivors_per_query": st["survivors"] / nq, "candidates_per_query": st["candidates"] / nq,
                                    "overflow_rows": st["overflow_rows"]}
                r["ladder"] = {"levels": ss["levels"], "ratio": ss["ratio"], "strides": ss["strides"], "k_r_estimate": k * ss["ratio"],
                               "level_survivors_per_query": [v / nq for v in ss["level_survivors"]],
                               "level_candidates_per_query": [v / nq for v in ss["level_candidates"]],
                               "rows_tightened": ss["rows_tightened"], "rows_level_overflow": ss["rows_level_overflow"]}
                point["ladder_" + mode] = r
            del os.environ["VI_EXACT_IP_LADDER"]
            point["equal"] = bool((I["0"] == I["1"]).all().item() and (S["0"].view(torch.int32) == S["1"].view(torch.int32)).all().item())
            matmul_topk(rows, ids, xq, k)
            point["matmul_topk_ms"] = timed(lambda: matmul_topk(rows, ids, xq, k), sync, args.repeats)
            res["k_%d" % k] = point
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ladder", action="store_true", help="measure the score-seeded ladder (profiles/r36_exact_ip_seed.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "r36_exact_ip_seed.json" if args.ladder else "r34_exact_ip.json")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_exact_ip.py needs an MI355X")
    import bench
    import vector_indexer_py as vip
    dev = torch.device("cuda", 0)
    xb, xq = bench.make_dataset(args.n, args.d, args.nq, 1234, dev)
    res = {"shape": {"n": args.n, "d": args.d, "nlist": args.nlist, "nq": args.nq, "k": args.k, "repeats": args.repeats},
           "device": torch.cuda.get_device_name(0)}
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    factor = torch.tensor([0.25, 1.0, 4.0], device=dev)[torch.randint(0, 3, (args.n, 1), generator=g, device=dev)]
    if args.ladder:
        res["bench_data"] = measure_ladder(vip, torch, xb, xq, args, dev, [args.k, 1, 128])
        res["norm_spread"] = measure_ladder(vip, torch, (xb * factor).contiguous(), xq, args, dev, [args.k])
    else:
        res["bench_data"] = measure(vip, torch, bench, xb, xq, args, dev)
        res["norm_spread"] = measure(vip, torch, bench, (xb * factor).contiguous(), xq, args, dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
