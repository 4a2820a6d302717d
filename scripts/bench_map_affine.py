"""The read mapper with affine gaps on one MI355X, beside the linear one: reads/s of polyhip_map_reads (gap -2) and of
polyhip_map_reads_affine at (-5, -2) and at (-2, -2), through the host-pointer calls, in one run.

    python scripts/bench_map_affine.py [--genome 5000000] [--reads 1000000] [--reps 3] [--out profiles/map_affine_bench.json]

- workload: scripts/bench_map.py's -- a synthetic genome, reads of 150 bp sampled from it with 5 % substitutions and 1 %
  indels, every second one reverse-complemented; default parameters (mapper.MapParams);
- protocol: the calls alternate (linear, affine -5/-2, affine -2/-2) --reps times after one warm-up round; a host clock
  around each call, which ends in a stream synchronise and includes the copies of the reads in and of the arrays and
  strings out; medians are reported;
- tb_share: the traceback windows' cells (info.tb_cells) over the score pass's cells.  The score pass sweeps lenA x lenB
  per pair with lenB between m + 2 band and m + 3 band (window of the cluster; clipping at the text's ends aside), so the
  share is given against both bounds;
- affine_over_linear: the ratio of the medians; equal_gaps_same: the (-2, -2) call's arrays and strings equal the linear
  call's;
- spot check: eight reads against tests/map_affine_oracle.py at (-5, -2).
Prints one JSON object (and writes it to --out).  Nothing here has a speed threshold.
"""
from __future__ import annotations

import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from bench_map import make_reads
    from poly_amd import align, alphabet, bwt, mapper, mash, matrix
    assert torch.cuda.is_available(), "bench_map_affine.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(17)
    n, N, m = args.genome, args.reads, 150
    P = mapper.MapParams()
    ab = alphabet.NewAlphabet(list("-ACGT"))
    sc = align.NewScoring(matrix.NewSubstitutionMatrix(ab, ab, matrix.NUC_4), -2)

    g_t = torch.empty(n, dtype=torch.uint8, device=dev)
    mash.synth_dna_dev(0x5EED + n, g_t)
    idx = bwt.new_dev(g_t)
    g = g_t.cpu().numpy()
    reads = make_reads(rng, g, N, m)
    buf = reads.reshape(-1)
    offs = np.arange(0, N * m + 1, m, dtype=np.uint64)
    cap = 2 * N * m

    # the C calls themselves on preallocated host arrays (mapper.map_reads*_packed would add a Python list of 2 N strings)
    import ctypes as C
    from poly_amd import _lib
    lib, p = _lib.lib(), P._c()

    class Out:
        def __init__(self):
            self.score, self.second = np.zeros(N, np.int64), np.zeros(N, np.int64)
            self.u32 = [np.zeros(N, np.uint32) for _ in range(7)]
            (self.flags, self.votes, self.ref_start, self.ref_end, self.read_start, self.read_end, self.err) = self.u32
            self.alnA, self.alnB, self.off = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(N + 1, np.uint64)

        def tail(self):
            return (self.score.ctypes.data, self.second.ctypes.data, *[x.ctypes.data for x in self.u32], self.alnA.ctypes.data,
                    self.alnB.ctypes.data, self.off.ctypes.data, cap)

        def strings(self, i):
            o = self.off
            return self.alnA[int(o[i]):int(o[i + 1])].tobytes(), self.alnB[int(o[i]):int(o[i + 1])].tobytes()

    head = (idx.handle(), sc.handle(), C.byref(p))
    seqs = (buf.ctypes.data, offs.ctypes.data, N, m)
    res = {k: Out() for k in ("linear", "affine_5_2", "affine_2_2")}
    calls = {
        "linear": lambda: lib.polyhip_map_reads(*head, *seqs, *res["linear"].tail()),
        "affine_5_2": lambda: lib.polyhip_map_reads_affine(*head, -5, -2, *seqs, 0, *res["affine_5_2"].tail()),
        "affine_2_2": lambda: lib.polyhip_map_reads_affine(*head, -2, -2, *seqs, 0, *res["affine_2_2"].tail()),
    }
    infos = {"linear": mapper.last_info, "affine_5_2": mapper.last_affine_info, "affine_2_2": mapper.last_affine_info}
    times = {k: [] for k in calls}
    info = {}
    for rep in range(args.reps + 1):                       # round 0 warms up; the calls alternate
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

    lin, eq = res["linear"], res["affine_2_2"]
    used = int(lin.off[N])
    same = all((getattr(lin, f) == getattr(eq, f)).all() for f in FIELDS) and (lin.off == eq.off).all() and \
        (lin.alnA[:used] == eq.alnA[:used]).all() and (lin.alnB[:used] == eq.alnB[:used]).all()

    # eight reads against the oracle
    import map_affine_oracle as mao
    import map_oracle as mo
    import sw_affine_oracle as ao
    T = g.tobytes()
    Po = mo.Params(**dataclasses.asdict(P))
    got = res["affine_5_2"]
    spot = []
    for i in np.linspace(0, N - 1, 8).astype(int):
        counters = dict(seeds=0, seeds_over_max_occ=0, hits=0, clusters=0, pairs_aligned=0, reads_mapped=0)
        h = mao.map_read(T, reads[i].tobytes(), ao.NUC_4, -5, -2, Po, counters)
        spot.append(bool(all(int(getattr(got, f)[i]) == getattr(h, f) for f in FIELDS) and got.strings(i) == (h.alignA, h.alignB)))

    a = info["affine_5_2"]
    lo, hi = a["pairs_aligned"] * m * (m + 2 * P.band), a["pairs_aligned"] * m * (m + 3 * P.band)
    out = {"device": torch.cuda.get_device_name(0), "genome": n, "reads": N, "read_len": m, "params": P.__dict__, "reps": args.reps,
           "seconds": med, "seconds_all": times, "reads_per_s": {k: N / v for k, v in med.items()}, "info": info,
           "score_cells_bounds": [lo, hi], "tb_share": [a["tb_cells"] / hi, a["tb_cells"] / lo],
           "affine_over_linear": med["affine_5_2"] / med["linear"], "affine_equal_gaps_over_linear": med["affine_2_2"] / med["linear"],
           "equal_gaps_same": bool(same), "spot_check": spot}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    assert same and all(spot), "the affine mapper's results differ from the linear call's / the oracle's"


if __name__ == "__main__":
    main()
