"""K2 neighbour lists against the dense join on one MI355X, in ONE process, resident inputs, alternating.

    python scripts/bench_mash_neighbors.py [--reps 9] [--calls 10] [--scale 1000000] [--out profiles/mash_neighbors_bench.json]

The configs[2] row block (12,500 x 100,000 sketches of 1000 hashes, bench_extra.family_sketches seed 0xC3):
  a      shared_counts_reuse_dev: the dense join against a prebuilt index (2.5 GB of counts written)
  index  index_build_dev alone -- neighbors_dev builds the block index inside every call
  b      neighbors_dev at min_shared = 1 (index build + join + CSR assembly + its host synchronisation)
  count  b without cols / shared / dist: first[] alone -- the walk and the flush's counting, no entry stored (what the
         FIRST pass of a two-pass CSR assembly -- count, scan, fill -- would cost; its second pass is another whole join)
  c      b with k = 10 and exclude_self
Every repeat runs a, index, b, c one after the other (--calls calls each, host clock around the calls and a device
synchronise); the spread is over the repeats.  "b_join_ms" = b - index, repeat by repeat: the neighbour join and assembly
on their own, the figure to hold against a.  It is DERIVED, not timed on its own (the ABI has no index-reuse form of the
list), and it still holds b's host synchronisation and 16-byte read-back, which a does not have; the kernel times
themselves are in profiles/mash_neighbors_kernel_stats.md (this script under rocprofv3 --kernel-trace --stats).
"two_pass_floor_ms" = 2 * (count - index): the least a two-pass assembly could cost, to hold against b_join_ms.
The scale leg (--scale N, 0 = skip): N x N sketches of 1000 hashes on one GPU, exclude_self, k = 10; recorded, not asserted.
Writes one JSON object to --out and prints it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1_000_000)
    ap.add_argument("--scale-min-shared", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mash_neighbors_bench.json"))
    args = ap.parse_args()
    import torch
    from poly_amd import bench_extra, mash
    if not torch.cuda.is_available():
        raise SystemExit("bench_mash_neighbors: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    nx, ny, s = 12_500, 100_000, 1000
    sk = bench_extra.family_sketches(dev, 1000, 100, 10_000, 21, s, seed=0xC3)
    X = sk[:nx]
    counts = torch.zeros((nx, ny), dtype=torch.int16, device=dev)
    work_a = torch.empty(mash.shared_counts_workspace_bytes(nx, s, ny, s), dtype=torch.uint8, device=dev)
    work_n = torch.empty(mash.neighbors_workspace_bytes(nx, s, ny, s), dtype=torch.uint8, device=dev)
    first = torch.zeros(nx + 1, dtype=torch.int64, device=dev)
    mash.neighbors_dev(X, sk, first, None, None, None, work_n)
    total = int(first[nx].item())
    cols = torch.zeros(total, dtype=torch.int32, device=dev)
    shared = torch.zeros(total, dtype=torch.int16, device=dev)
    dist = torch.zeros(total, dtype=torch.float64, device=dev)
    mash.index_build_dev(sk, work_a)
    info = {}

    def run_a():
        mash.shared_counts_reuse_dev(X, sk, counts, work_a)

    def run_i():
        mash.index_build_dev(sk, work_n)

    def run_b():
        mash.neighbors_dev(X, sk, first, cols, shared, dist, work_n, 1, 0)

    def run_n():
        mash.neighbors_dev(X, sk, first, None, None, None, work_n, 1, 0)

    def run_c():
        mash.neighbors_dev(X, sk, first, cols, shared, dist, work_n, 1, 10, True, 0)

    forms = {"a_dense_reuse": run_a, "index_build": run_i, "b_neighbors": run_b, "b_count_only": run_n,
             "c_neighbors_k10": run_c}
    for fn in forms.values():  # warm-up: every shape the timed window uses
        fn()
        fn()
    torch.cuda.synchronize()
    run_b()
    info["b"] = mash.neighbors_last_info()
    entries_b = int(first[nx].item())
    run_c()
    info["c"] = mash.neighbors_last_info()
    entries_c = int(first[nx].item())
    ms = {name: [] for name in forms}
    for _ in range(args.reps):
        for name, fn in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.calls)

    def stats(v):
        return {"min": min(v), "median": statistics.median(v), "max": max(v), "all": v}

    b_join = [b - i for b, i in zip(ms["b_neighbors"], ms["index_build"])]
    c_join = [c - i for c, i in zip(ms["c_neighbors_k10"], ms["index_build"])]
    n_join = [n - i for n, i in zip(ms["b_count_only"], ms["index_build"])]
    out = {
        "block": {"nx": nx, "ny": ny, "s": s, "reps": args.reps, "calls_per_rep": args.calls,
                  "timing": "host clock around the calls of one form and a device synchronise; ms per call"},
        "ms": {name: stats(v) for name, v in ms.items()},
        "b_join_ms": stats(b_join), "c_join_ms": stats(c_join), "count_only_join_ms": stats(n_join),
        "two_pass_floor_ms": 2 * statistics.median(n_join),
        "derived": "b_join / c_join / count_only_join = the call minus index_build of the same repeat; not timed alone",
        "a_spread_ms": max(ms["a_dense_reuse"]) - min(ms["a_dense_reuse"]),
        "b_join_minus_a_ms_median": statistics.median(b_join) - statistics.median(ms["a_dense_reuse"]),
        "entries": {"b": entries_b, "c": entries_c},
        "bytes_written": {"a": nx * ny * 2, "b": entries_b * 14 + (nx + 1) * 8, "c": entries_c * 14 + (nx + 1) * 8,
                          "b_temporary_list": entries_b * 6},
        "last_info": info,
    }
    del counts, work_a, work_n, cols, shared, dist
    torch.cuda.empty_cache()
    if args.scale:
        n = args.scale
        fam = max(1, n // 100)
        t0 = time.perf_counter()
        big = bench_extra.family_sketches(dev, fam, 100, 10_000, 21, s, seed=0xC3)
        n = big.shape[0]
        t_sketch = time.perf_counter() - t0
        work = torch.empty(mash.neighbors_workspace_bytes(n, s, n, s), dtype=torch.uint8, device=dev)
        first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        cols = torch.zeros(n * 10, dtype=torch.int32, device=dev)
        shared = torch.zeros(n * 10, dtype=torch.int16, device=dev)
        dist = torch.zeros(n * 10, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mash.neighbors_dev(big, big, first, cols, shared, dist, work, args.scale_min_shared, 10, True, 0)
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        out["scale"] = {"n": n, "s": s, "k": 10, "exclude_self": True, "min_shared": args.scale_min_shared,
                        "seconds": t, "seconds_generate_and_sketch": t_sketch, "workspace_bytes": work.numel(),
                        "entries": int(first[n].item()), "last_info": mash.neighbors_last_info(), "runs": 1}
    txt = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
