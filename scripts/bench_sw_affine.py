"""Smith-Waterman with affine gaps on one MI355X, against the linear path at the same shape in the same run.

    python scripts/bench_sw_affine.py [--shapes config4,pairs] [--reads 1000000] [--pairs 200000] [--reps 3] [--out FILE]

- config4: BASELINE config 4 -- --reads x 150 bp (poly_amd/workloads.py, 5 % substitutions, 1 % indels) against one 5 kb
  reference;  pairs: --pairs pairs of 150 x 150, each read against the clean window it was made from;
- NUC_4, gap_open = -5, gap_extend = -2 for polyhip_sw_affine_batch and polyhip_sw_affine_align_batch_packed; gap = -2
  for polyhip_sw_batch and polyhip_sw_align_batch_packed, the yardstick, measured here and not taken from elsewhere;
- per call: wall time of the host-pointer call (upload and read-back included; best of --reps after a warm-up call) and
  cell updates per second -- for the affine calls from polyhip_sw_affine_last_info (score pass cells, and the traceback
  windows' cells as well for the strings call), for the linear calls lenA x lenB summed over the pairs;
- ratio: affine wall time / linear wall time, for the score call and for the strings call;
- after the timing, eight pairs spread over each batch are compared with tests/sw_affine_oracle.py.
Prints one JSON object (and writes it to --out, default profiles/sw_affine_bench.json).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

GO, GE, LINEAR_GAP = -5, -2, -2


def wall(fn, reps):
    fn()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="config4,pairs")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sw_affine_bench.json"))
    args = ap.parse_args()

    import torch
    import sw_affine_oracle as ao
    from poly_amd import align, alphabet, matrix, workloads
    assert torch.cuda.is_available(), "bench_sw_affine.py measures on the GPU; there is no CPU path"
    ab = alphabet.NewAlphabet(list("-ACGT"))
    sc = align.NewScoring(matrix.NewSubstitutionMatrix(ab, ab, matrix.NUC_4), LINEAR_GAP)
    out = {"device": torch.cuda.get_device_name(0), "gap_open": GO, "gap_extend": GE, "linear_gap": LINEAR_GAP, "shapes": {}}
    align.SmithWatermanAffine("ACGTACGT", "ACGTTACGT", sc, GO, GE)      # warm-up: code objects, the allocator
    align.SmithWaterman("ACGTACGT", "ACGTTACGT", sc)

    for shape in args.shapes.split(","):
        if shape == "config4":
            ref, reads = workloads.config4_reads(args.reads)
            n, B, offB = args.reads, np.ascontiguousarray(ref), None
            cells = n * 150 * len(B)
        else:
            _, reads = workloads.config4_reads(args.pairs)
            _, clean = workloads.config4_reads(args.pairs, sub=0.0, indel=0.0)
            n, B = args.pairs, np.ascontiguousarray(clean.reshape(-1))
            offB = np.arange(0, n * 150 + 1, 150, dtype=np.uint64)
            cells = n * 150 * 150
        A = np.ascontiguousarray(reads.reshape(-1))
        offA = np.arange(0, n * 150 + 1, 150, dtype=np.uint64)
        leg = {"pairs": n, "lenA": 150, "lenB": int(len(B) if offB is None else 150), "cells": cells}
        t = wall(lambda: align.sw_affine_packed(sc, GO, GE, A, offA, B, offB), args.reps)
        info = align.sw_affine_last_info()
        leg["affine_score"] = {"s": t, "cells_per_s": info["cells"] / t, "info": info}
        t = wall(lambda: align.sw_affine_align_packed(sc, GO, GE, A, offA, B, offB), args.reps)
        info = align.sw_affine_last_info()
        leg["affine_strings"] = {"s": t, "cells_per_s": (info["cells"] + info["tb_cells"]) / t, "info": info}
        t = wall(lambda: align.sw_batch_packed(sc, A, offA, B, offB), args.reps)
        leg["linear_score"] = {"s": t, "cells_per_s": cells / t, "path": align.last_path()}
        t = wall(lambda: align.sw_align_strings_packed(sc, A, offA, B, offB), args.reps)
        leg["linear_strings"] = {"s": t, "cells_per_s": cells / t, "path": align.last_path(),
                                 "traceback_path": align.sw_traceback_last_path()}
        leg["ratio_score"] = leg["affine_score"]["s"] / leg["linear_score"]["s"]
        leg["ratio_strings"] = leg["affine_strings"]["s"] / leg["linear_strings"]["s"]
        # spot checks: eight pairs spread over the batch, both affine calls against the oracle
        got4 = align.sw_affine_packed(sc, GO, GE, A, offA, B, offB)
        got6 = align.sw_affine_align_packed(sc, GO, GE, A, offA, B, offB)
        for p in np.linspace(0, n - 1, 8).astype(int):
            b = bytes(B) if offB is None else bytes(B[int(offB[p]):int(offB[p + 1])])
            want = ao.align(bytes(A[int(offA[p]):int(offA[p + 1])]), b, ao.NUC_4, GO, GE)
            assert tuple(int(x[p]) for x in got4) == tuple(want[:4]), (shape, int(p))
            assert (int(got6[0][p]), int(got6[1][p]), int(got6[2][p]), int(got6[3][p]), got6[4][p], got6[5][p]) == tuple(want), (shape, int(p))
        leg["spot_checks"] = 8
        out["shapes"][shape] = leg
        print(f"{shape}: {json.dumps(leg)}", file=sys.stderr, flush=True)

    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
