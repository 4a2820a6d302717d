"""The paired-end read mapper on one MI355X, beside the single-read affine mapper on the same reads, in one run.

    python scripts/bench_map_pairs.py [--genome 5000000] [--pairs 500000] [--reps 3] [--out profiles/map_pairs_bench.json]

- workload: a synthetic genome with a few planted 300-bp repeats (five sequences, four copies each); pairs of 2 x 150 bp
  from fragments of 350 +- 50 bp (normal, cut to 200 .. 500), each mate with 5 % substitutions and 1 % indels as in
  scripts/bench_map.py; every second pair flipped (mate 1 is the reverse one); default parameters (mapper.MapParams),
  gaps (-5, -2), PairParams(200, 500);
- protocol: three calls alternate --reps times after one warm-up round: polyhip_map_pairs with rescue, without rescue,
  and polyhip_map_reads_affine on the same 2 x pairs reads interleaved (the yardstick: its code is the single-read
  mapper's); a host clock around each call, which ends in a stream synchronise and includes the copies of the reads in
  and of the arrays and strings out; medians and all times are reported;
- where the extra time goes: no_rescue - single is what the pair rule costs (the interleave, the pair-reduce and
  resolve kernels, tlen); rescue - no_rescue is what the rescue costs (its gather, its score pass, the wider windows of
  the traceback and the tracebacks of the mates it places);
- cells: the candidates' score pass sweeps 150 x (150 + 2 band .. 150 + 3 band) per candidate (bounds), a rescue attempt
  150 x (max_insert - min_insert + 150 + 2 band) unless the text's end clips it;
- placed: the share of pairs with both mates within 10 bp of where they came from (the forward mate's ref_start -
  read_start against the fragment's start, the reverse mate's ref_end + (150 - read_end) against its end), for the
  paired calls and for the single-read call;
- spot check: four pairs against tests/map_pairs_oracle.py.
Prints one JSON object (and writes it to --out).  Nothing here has a speed threshold.
"""
from __future__ import annotations

import argparse
import ctypes as C
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

FIELDS = ("score", "second", "flags", "votes", "ref_start", "ref_end", "read_start", "read_end", "err")


def make_pairs(rng, g, npairs, m=150, mean=350, sd=50, lo=200, hi=500, block=100_000):
    """-> (mate1, mate2: (npairs, m) uint8, start, end of every fragment, flipped)"""
    from bench_map import COMP, mutate_windows
    span = m + 20
    fwd, rev = np.empty((npairs, m), np.uint8), np.empty((npairs, m), np.uint8)
    insert = np.clip(np.rint(rng.normal(mean, sd, npairs)), lo, hi).astype(np.int64)
    start = rng.integers(0, len(g) - hi - span, npairs)
    end = start + insert
    for r0 in range(0, npairs, block):
        k = min(block, npairs - r0)
        cols = np.arange(span)
        fwd[r0:r0 + k] = mutate_windows(rng, g[start[r0:r0 + k, None] + cols], m)
        src = COMP[g[end[r0:r0 + k, None] - 1 - cols]]        # the fragment read from its end, on the other strand
        rev[r0:r0 + k] = mutate_windows(rng, src, m)
    flipped = np.arange(npairs) % 2 == 1
    m1, m2 = np.where(flipped[:, None], rev, fwd), np.where(flipped[:, None], fwd, rev)
    return m1, m2, start, end, flipped


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from poly_amd import _lib, align, alphabet, bwt, mapper, mash, matrix
    assert torch.cuda.is_available(), "bench_map_pairs.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(23)
    n, N, m = args.genome, args.pairs, 150
    P, PP, go, ge = mapper.MapParams(), mapper.PairParams(200, 500), -5, -2
    ab = alphabet.NewAlphabet(list("-ACGT"))
    sc = align.NewScoring(matrix.NewSubstitutionMatrix(ab, ab, matrix.NUC_4), -2)

    g_t = torch.empty(n, dtype=torch.uint8, device=dev)
    mash.synth_dna_dev(0x5EED + n, g_t)
    g = g_t.cpu().numpy()
    for _ in range(5):                                         # planted repeats
        rep = g[int(rng.integers(0, n - 300)):][:300].copy()
        for at in rng.integers(0, n - 300, 3):
            g[at:at + 300] = rep
    idx = bwt.new_dev(torch.from_numpy(g).to(dev))
    m1, m2, start, end, flipped = make_pairs(rng, g, N, m)
    inter = np.empty((2 * N, m), np.uint8)
    inter[0::2], inter[1::2] = m1, m2
    off1 = np.arange(0, N * m + 1, m, dtype=np.uint64)
    off2 = np.arange(0, 2 * N * m + 1, m, dtype=np.uint64)
    cap = 4 * N * m

    class Out:
        def __init__(self):
            R = 2 * N
            self.score, self.second = np.zeros(R, np.int64), np.zeros(R, np.int64)
            self.u32 = [np.zeros(R, np.uint32) for _ in range(7)]
            (self.flags, self.votes, self.ref_start, self.ref_end, self.read_start, self.read_end, self.err) = self.u32
            self.tlen = np.zeros(N, np.int64)
            self.alnA, self.alnB, self.off = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(R + 1, np.uint64)

        def mates(self):
            return (self.score.ctypes.data, self.second.ctypes.data, *[x.ctypes.data for x in self.u32])

        def strings(self):
            return (self.alnA.ctypes.data, self.alnB.ctypes.data, self.off.ctypes.data, cap)

        def aligned(self, i):
            o = self.off
            return self.alnA[int(o[i]):int(o[i + 1])].tobytes(), self.alnB[int(o[i]):int(o[i + 1])].tobytes()

    lib, p = _lib.lib(), P._c()
    pp = {"rescue": PP._c(), "no_rescue": dataclasses.replace(PP, rescue=False)._c()}
    head = (idx.handle(), sc.handle(), C.byref(p))
    res = {k: Out() for k in ("rescue", "no_rescue", "single")}

    def paired(k):
        o = res[k]
        return lambda: lib.polyhip_map_pairs(*head, C.byref(pp[k]), go, ge, m1.ctypes.data, off1.ctypes.data, m2.ctypes.data,
                                             off1.ctypes.data, N, m, 0, *o.mates(), o.tlen.ctypes.data, *o.strings())
    calls = {"rescue": paired("rescue"), "no_rescue": paired("no_rescue"),
             "single": lambda: lib.polyhip_map_reads_affine(*head, go, ge, inter.ctypes.data, off2.ctypes.data, 2 * N, m, 0,
                                                            *res["single"].mates(), *res["single"].strings())}
    infos = {"rescue": mapper.last_pairs_info, "no_rescue": mapper.last_pairs_info, "single": mapper.last_affine_info}
    times = {k: [] for k in calls}
    info = {}
    for rep in range(args.reps + 1):                           # round 0 warms up; the calls alternate
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(fn())
            dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt)
            else:
                info[name] = infos[name]()
    med = {k: float(np.median(v)) for k, v in times.items()}

    def placed(o):
        """both mates of a pair within 10 bp of the fragment's ends"""
        fl = o.flags.astype(np.int64)
        left = o.ref_start.astype(np.int64) - o.read_start.astype(np.int64)
        right = o.ref_end.astype(np.int64) + (m - o.read_end.astype(np.int64))
        rev = (fl >> 1) & 1
        want_rev = np.empty(2 * N, np.int64)
        want_rev[0::2], want_rev[1::2] = flipped, ~flipped
        where = np.where(want_rev == 1, np.repeat(end, 2), np.repeat(start, 2))
        ok = ((fl & 1) == 1) & (rev == want_rev) & (np.abs(np.where(rev == 1, right, left) - where) <= 10)
        return float((ok[0::2] & ok[1::2]).mean())

    # four pairs against the oracle
    import map_oracle as mo
    import map_pairs_oracle as mpo
    import sw_affine_oracle as ao
    T = g.tobytes()
    Po = mo.Params(**dataclasses.asdict(P))
    got, spot = res["rescue"], []
    for i in np.linspace(0, N - 1, 4).astype(int):
        r = mpo.map_pair(T, m1[i].tobytes(), m2[i].tobytes(), ao.NUC_4, go, ge, Po, mpo.PairParams(PP.min_insert, PP.max_insert, True), m)
        same = int(got.tlen[i]) == r.tlen
        for x, h in enumerate((r.h1, r.h2)):
            same = same and all(int(getattr(got, f)[2 * i + x]) == getattr(h, f) for f in FIELDS) and \
                got.aligned(2 * i + x) == (h.alignA, h.alignB)
        spot.append(bool(same))

    a = info["rescue"]
    cand = [a["pairs_aligned"] * m * (m + 2 * P.band), a["pairs_aligned"] * m * (m + 3 * P.band)]
    out = {"device": torch.cuda.get_device_name(0), "genome": n, "pairs": N, "read_len": m, "params": P.__dict__,
           "pair_params": PP.__dict__, "gaps": [go, ge], "reps": args.reps, "seconds": med, "seconds_all": times,
           "pairs_per_s": {k: N / v for k, v in med.items()}, "rescue_over_single": med["rescue"] / med["single"],
           "no_rescue_over_single": med["no_rescue"] / med["single"],
           "extra_seconds": {"pair_rule": med["no_rescue"] - med["single"], "rescue": med["rescue"] - med["no_rescue"]},
           "info": info, "candidate_cells_bounds": cand,
           "rescue_cells": a["rescue_attempts"] * m * (PP.max_insert - PP.min_insert + m + 2 * P.band),
           "placed": {k: placed(o) for k, o in res.items()}, "spot_check": spot}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    assert all(spot), "the paired mapper's results differ from the oracle's"


if __name__ == "__main__":
    main()
