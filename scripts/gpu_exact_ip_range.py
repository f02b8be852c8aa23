#!/usr/bin/env python3
"""Measure the exact (flat) inner-product threshold search on the bench index and write profiles/r35_exact_ip_range.json.

On the benchmark's shape (N = 1e6, D = 128, 4096 lists, 10 000 device-resident queries; --n / --nq / --nlist shrink it) and
on a norm-spread copy of it (every row scaled by a factor drawn from {0.25, 1, 4}) it records, at the median over the
queries of the 1st / 10th / 100th largest score as the threshold, --repeats calls each (host clock around calls that end
synchronised, after a warm-up call; min and max),
  * range_search_exact_ip_device, and in a separate call under VI_EXACT_TIMING its phases, survivors and hits per query and
    the number of sweeps (recorded, not asserted);
  * the only route before: a torch fp32 matmul over the exported rows + mask + nonzero, in chunks of 131 072 rows, and the
    queries whose set of ids differs from the call's (scores at the threshold that the two sums round apart);
  * search_exact_ip_device at k = 1 / 10 / 100 on the same handle (--cmp-repeats calls);
  * range_search_exact_device (L2) at the median 1st / 10th / 100th neighbour's radius: a similar number of hits;
  * once, min_score = -inf on 128 queries: every tile crowded, every record a hit.
Needs an MI355X; nothing here falls back to the CPU."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vector-indexer_amd")]
KS = (1, 10, 100)


def timed(fn, sync, repeats):
    out = []
    for _ in range(repeats):
        sync()
        t = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t) * 1e3)
    return [min(out), max(out)]


def matmul_mask(torch, rows, xq, t):
    """every (query, row) with fp32 matmul score >= t -> (query index, row index), unsorted"""
    qs, rs = [], []
    for s in range(0, rows.shape[0], 131072):
        hit = torch.nonzero(xq @ rows[s:s + 131072].T >= t)
        qs.append(hit[:, 0])
        rs.append(hit[:, 1] + s)
    return torch.cat(qs), torch.cat(rs)


def topk_values(torch, rows, xq, k, largest):
    """per query the k largest inner products (largest) or smallest squared distances, by fp32 matmul, in chunks"""
    best = None
    for s in range(0, rows.shape[0], 131072):
        blk = rows[s:s + 131072]
        v = xq @ blk.T if largest else (xq * xq).sum(1, keepdim=True) - 2.0 * (xq @ blk.T) + (blk * blk).sum(1)[None, :]
        v = torch.topk(v, k, dim=1, largest=largest).values
        best = v if best is None else torch.topk(torch.cat([best, v], 1), k, dim=1, largest=largest).values
    return best


def measure(vip, torch, xb, xq, args, dev):
    import numpy as np
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    nq, res = xq.shape[0], {}
    with tempfile.TemporaryDirectory() as work:
        index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000)
        n = index.num_vectors
        rows = torch.empty((n, args.d), dtype=torch.float32, device=dev)
        ids = torch.empty(n, dtype=torch.int64, device=dev)
        index.export_device(0, n, ids.data_ptr(), rows.data_ptr())
        top_s = topk_values(torch, rows, xq, max(KS), True)
        top_d = topk_values(torch, rows, xq, max(KS), False)
        kmax = max(KS)
        S = torch.empty((nq, kmax), dtype=torch.float32, device=dev)
        I = torch.empty((nq, kmax), dtype=torch.int64, device=dev)
        for k in KS:
            t = float(top_s[:, k - 1].median().item())
            r2 = float(top_d[:, k - 1].median().item())
            point = {"min_score": t, "radius2": r2}

            def call(t=t):
                index.range_search_exact_ip_device(xq.data_ptr(), nq, t).free()

            def l2(r2=r2):
                index.range_search_exact_device(xq.data_ptr(), nq, r2).free()

            def topk(k=k):
                index.search_exact_ip_device(xq.data_ptr(), nq, k, S.data_ptr(), I.data_ptr())

            call(), l2(), topk(), matmul_mask(torch, rows, xq, t)  # warm-up: code objects, workspaces
            point["range_exact_ip_ms"] = timed(call, sync, args.repeats)
            point["matmul_mask_ms"] = timed(lambda: matmul_mask(torch, rows, xq, t), sync, args.repeats)
            point["range_exact_l2_ms"] = timed(l2, sync, args.repeats)
            point["l2_hits_per_query"] = index.exact_range_stats()["hits"] / nq
            point["search_exact_ip_ms"] = {"k": k, "ms": timed(topk, sync, args.cmp_repeats),
                                           "overflow_rows": index.exact_ip_stats()["overflow_rows"]}
            os.environ["VI_EXACT_TIMING"] = "1"
            out = index.range_search_exact_ip_device(xq.data_ptr(), nq, t)
            st = index.exact_ip_range_stats()
            del os.environ["VI_EXACT_TIMING"]
            point["phases"] = {f: st[f] for f in ("ms_prepare", "ms_sweep", "ms_place", "ms_sort", "ms_output", "ms_total")}
            point["counts"] = {"survivors_per_query": st["survivors"] / nq, "hits_per_query": st["hits"] / nq, "sweeps": st["sweeps"],
                               "pool_cap": st["pool_cap"], "query_tile": st["query_tile"], "block_splits": st["block_splits"]}
            # the queries whose set of ids the matmul route gives differs from the call's
            lims, _, got_i = out.copy()
            out.free()
            got = np.repeat(np.arange(nq, dtype=np.int64), np.diff(lims).astype(np.int64)) << 40 | got_i
            mq, mr = matmul_mask(torch, rows, xq, t)
            ref = (mq << 40 | ids[mr]).cpu().numpy()
            point["matmul_hits_per_query"] = len(ref) / nq
            point["matmul_rows_differing"] = int(len(np.unique(np.setxor1d(got, ref) >> 40)))
            point["ratio_to_matmul"] = point["range_exact_ip_ms"][0] / point["matmul_mask_ms"][0]
            res[f"k{k}"] = point
            print(f"k = {k}: {json.dumps(point)}", file=sys.stderr, flush=True)
        # every record of 128 queries: every accumulator tile crowded, every survivor a hit
        m = min(nq, 128)
        everything = lambda: index.range_search_exact_ip_device(xq.data_ptr(), m, float("-inf")).free()  # noqa: E731
        everything()
        os.environ["VI_EXACT_TIMING"] = "1"
        everything()
        st = index.exact_ip_range_stats()
        del os.environ["VI_EXACT_TIMING"]
        res["minus_inf"] = {"nq": m, "ms": timed(everything, sync, args.repeats), "hits": st["hits"], "sweeps": st["sweeps"],
                            "phases": {f: st[f] for f in ("ms_prepare", "ms_sweep", "ms_place", "ms_sort", "ms_output", "ms_total")}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cmp-repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r35_exact_ip_range.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_exact_ip_range.py needs an MI355X")
    import bench
    import vector_indexer_py as vip
    dev = torch.device("cuda", 0)
    xb, xq = bench.make_dataset(args.n, args.d, args.nq, 1234, dev)
    res = {"shape": {"n": args.n, "d": args.d, "nlist": args.nlist, "nq": args.nq, "repeats": args.repeats, "cmp_repeats": args.cmp_repeats},
           "device": torch.cuda.get_device_name(0)}
    res["bench_data"] = measure(vip, torch, xb, xq, args, dev)
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    factor = torch.tensor([0.25, 1.0, 4.0], device=dev)[torch.randint(0, 3, (args.n, 1), generator=g, device=dev)]
    res["norm_spread"] = measure(vip, torch, (xb * factor).contiguous(), xq, args, dev)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
