"""search/bwt with mismatches on one MI355X: polyhip_bwt_count_mismatch for k = 0..3 against the random-line read rate.

    python scripts/bench_bwt_mismatch.py [--sizes 5000000,100000000] [--npat 1000000] [--ks 0,1,2,3] [--reps 3] [--out FILE]

- genomes: the synthetic ones of scripts/bench_bwt.py (polyhip_synth_dna_dev, the same seeds);
- patterns: --npat 20-mers sampled from the genome, pattern i with i mod (k + 1) substitutions (each to another base);
- per k: wall time of one host-pointer polyhip_bwt_count_mismatch call (upload and read-back included; best of --reps
  after a warm-up call, or the warm-up call alone once it takes more than two seconds), patterns/s, and the library's own
  nodes and occ_lines (polyhip_bwt_mismatch_last_info) with lines/s = occ_lines / time;
- k = 0: polyhip_bwt_count (the exact path, host-pointer too) on the same patterns, timed the same way;
- bound: the rate of uniformly random 128-byte lines from a table the size of the occurrence structure, MEASURED by
  scripts/ubench/random_lines.hip in the same run; lines/s is set against it (share_of_random_line_rate), no fraction
  is fixed in advance.
Prints one JSON object (and writes it to --out, default profiles/bwt_mismatch_bench.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_bwt import random_line_rates  # noqa: E402


def wall(fn, reps):
    t0 = time.perf_counter()
    fn()
    best = time.perf_counter() - t0
    if best > 2.0:
        return best, 1
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best, reps


def sample(rng, g, npat, m, k):
    """npat m-mers of g, pattern i with i mod (k + 1) substitutions at distinct positions, each to another base"""
    st = rng.integers(0, len(g) - m, npat)
    pats = g[st[:, None] + np.arange(m)]
    code = np.zeros(256, np.uint8)
    code[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
    # k distinct positions per pattern: a random start, then steps of 7 (coprime to m = 20)
    where = (rng.integers(0, m, npat)[:, None] + 7 * np.arange(max(k, 1))) % m
    subs = np.arange(npat) % (k + 1)
    rows = np.arange(npat)
    for j in range(k):
        hit = subs > j
        col = where[hit, j]
        old = code[pats[rows[hit], col]]
        pats[rows[hit], col] = np.frombuffer(b"ACGT", np.uint8)[(old + rng.integers(1, 4, int(hit.sum()))) & 3]
    return np.ascontiguousarray(pats.reshape(-1)), np.arange(0, npat * m + 1, m, dtype=np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000000,100000000")
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--ks", default="0,1,2,3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bwt_mismatch_bench.json"))
    args = ap.parse_args()

    import torch
    from poly_amd import bwt, mash
    assert torch.cuda.is_available(), "bench_bwt_mismatch.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(12)
    out = {"device": torch.cuda.get_device_name(0), "npat": args.npat, "pattern_len": 20, "genomes": []}

    w = torch.empty(100_000, dtype=torch.uint8, device=dev)     # warm-up: code objects, the allocator
    mash.synth_dna_dev(1, w)
    bwt.new_dev(w).CountMismatchBatch([b"ACGTACGT"], 1)

    occ_bytes = []
    for n in [int(x) for x in args.sizes.split(",")]:
        g_t = torch.empty(n, dtype=torch.uint8, device=dev)
        mash.synth_dna_dev(0x5EED + n, g_t)
        idx = bwt.new_dev(g_t)
        torch.cuda.synchronize()
        lines = n // 448 + 2
        occ_bytes.append(lines * 128)
        g = g_t.cpu().numpy()
        del g_t
        gen = {"n": n, "layout": idx.Layout(), "occ_structure_bytes": lines * 128, "k": {}}
        for k in [int(x) for x in args.ks.split(",")]:
            buf, offs = sample(rng, g, args.npat, 20, k)
            t, reps = wall(lambda: idx.count_mismatch_packed(buf, offs, k), args.reps)
            info = idx.MismatchInfo()
            leg = {"s": t, "reps": reps, "patterns_per_s": args.npat / t, "nodes": info["nodes"], "occ_lines": info["occ_lines"],
                   "leaves": info["leaves"], "hits": info["hits"], "lines_per_s": info["occ_lines"] / t}
            if k == 0:
                te, _ = wall(lambda: idx.intervals_packed(buf, offs), args.reps)
                leg["exact_count_s"] = te
                leg["exact_count_patterns_per_s"] = args.npat / te
            gen["k"][str(k)] = leg
            print(f"n={n} k={k}: {json.dumps(leg)}", file=sys.stderr, flush=True)
        out["genomes"].append(gen)
        del idx
        torch.cuda.empty_cache()

    out["random_lines"] = random_line_rates(occ_bytes)
    for gen, rl in zip(out["genomes"], out["random_lines"]):
        for leg in gen["k"].values():
            leg["share_of_random_line_rate"] = leg["lines_per_s"] / rl["lines_per_s"]
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
