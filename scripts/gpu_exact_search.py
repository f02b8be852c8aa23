#!/usr/bin/env python3
"""Measure the exact (flat) search on the bench index and write profiles/r30_exact_search.json.

On the benchmark's C2 shape (N = 1e6, D = 128, 4096 lists, 10 000 queries, k = 10; --n / --nq / --nlist shrink it) it records
  * search_exact_device: wall time (host clock around calls that end synchronised), and in a separate call under
    VI_EXACT_TIMING its three phases, survivors and candidates per query and the overflow rows;
  * what the tree offered before: search_device at n_probe = every list (the generic engine; --nq-generic queries, it
    takes seconds per handful) and bench.py's ground_truth (torch fp32 matmul + topk) on the same tensors — neither is
    touched by the exact search, so both can be measured with this script on any commit that has them;
  * how many of ground_truth's ids differ from the exact ones (near-ties of the matmul form), and whether the generic
    engine's ids and distance bits equal the exact ones.
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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq-generic", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_exact_search.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_exact_search.py needs an MI355X")
    import bench
    import vector_indexer_py as vip
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    xb, xq = bench.make_dataset(args.n, args.d, args.nq, 1234, dev)
    nq, k = args.nq, args.k
    res = {"shape": {"n": args.n, "d": args.d, "nlist": args.nlist, "nq": nq, "k": k}, "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as work:
        index = vip.build(xb.cpu().numpy(), work, nlist=args.nlist, now_secs=1_700_000_000)
        res["lists"] = index.num_centroids
        D = torch.empty((nq, k), dtype=torch.float32, device=dev)
        I = torch.empty((nq, k), dtype=torch.int64, device=dev)

        def exact():
            index.search_exact_device(xq.data_ptr(), nq, k, D.data_ptr(), I.data_ptr())

        exact()  # warm-up: code objects, workspace
        res["exact_ms"] = timed(exact, sync, args.repeats)
        os.environ["VI_EXACT_TIMING"] = "1"
        exact()
        st = index.exact_stats()
        del os.environ["VI_EXACT_TIMING"]
        res["exact_phases"] = {f: st[f] for f in ("ms_seed", "ms_sweep", "ms_finish", "ms_total")}
        res["exact_counts"] = {"survivors_per_query": st["survivors"] / nq, "candidates_per_query": st["candidates"] / nq,
                               "overflow_rows": st["overflow_rows"], "seed_probe": st["seed_probe"], "cand_cap": st["cand_cap"],
                               "query_tile": st["query_tile"], "block_splits": st["block_splits"]}
        # 2 N D multiply-adds' worth of flop per query and product; 3 bf16 products where the lists have lo planes, else 2
        res["sweep_mac_per_product"] = float(args.n) * args.d * nq
        Ie = I.clone()

        gt = bench.ground_truth(xb, xq, k)  # warm-up
        res["ground_truth_ms"] = timed(lambda: bench.ground_truth(xb, xq, k), sync, 3)
        differ = (gt != Ie).any(dim=1)
        res["ground_truth_rows_differing"] = int(differ.sum().item())
        res["ground_truth_ids_differing"] = int((gt != Ie).sum().item())

        g = min(args.nq_generic, nq)
        Dg = torch.empty((g, k), dtype=torch.float32, device=dev)
        Ig = torch.empty((g, k), dtype=torch.int64, device=dev)

        def generic():
            index.search_device(xq.data_ptr(), g, k, index.num_centroids, Dg.data_ptr(), Ig.data_ptr(), 0)

        generic()
        res["generic_all_lists"] = {"nq": g, "ms": timed(generic, sync, 2)}
        res["generic_equals_exact"] = bool((Ig == Ie[:g]).all().item() and
                                           (Dg.view(torch.int32) == D[:g].view(torch.int32)).all().item())
        per_q_generic = min(res["generic_all_lists"]["ms"]) / g
        per_q_exact = min(res["exact_ms"]) / nq
        res["per_query_ms"] = {"generic_all_lists": per_q_generic, "exact": per_q_exact, "ratio": per_q_generic / per_q_exact}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
