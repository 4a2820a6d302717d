"""The read mapper on a reference of several contigs on one MI355X, beside the single-text calls on the same reads, in one run.

    python scripts/bench_map_refs.py [--genome 5000000] [--reads 1000000] [--pairs 500000] [--reps 3] [--only leg,leg] [--out profiles/map_refs_bench.json]

- workload: scripts/bench_map.py's (a synthetic genome, reads of 150 bp with 5 % substitutions and 1 % indels, half
  reverse-complemented; default parameters, gaps (-5, -2)) and scripts/bench_map_pairs.py's pairs (fragments of 350 +- 50,
  PairParams(200, 500)) on the same genome;
- legs, all through the host-pointer calls (copies of the reads in and of the arrays and strings out included):
  single      polyhip_map_reads_affine on the whole text: the yardstick
  refs_1      polyhip_map_reads_refs on the genome as one contig: what the refs path itself costs (the counting pass, the
              wider sort keys, the binary searches)
  refs_5kb    the genome cut into contigs of 5,000 bp (1,000 of them at 5 Mb)
  refs_100    the genome cut into contigs of 100 bp (50,000 of them)
  pairs_single / pairs_refs_1 / pairs_refs_5kb   polyhip_map_pairs on the whole text, polyhip_map_pairs_refs on one contig
              and on the 5 kb contigs
- protocol: the calls alternate --reps times after one warm-up round; a host clock around each call, which ends in a stream
  synchronise; medians and all times are reported;
- same_place: the share of entries whose flags and position in C (ref_start + start[rid]) equal the single-text call's;
- spot check: four reads of refs_5kb against tests/map_refs_oracle.py;
- --only: the legs to run (for a kernel trace of one leg in a run of its own); comparisons that need a missing leg are left out.
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

FIELDS = ("score", "second", "flags", "votes", "rid", "ref_start", "ref_end", "read_start", "read_end", "err")


class Out:
    """the output arrays of one leg: R entries, strings of `cap` bytes, tlen for pairs"""

    def __init__(self, R, cap, npairs=0):
        self.score, self.second = np.zeros(R, np.int64), np.zeros(R, np.int64)
        self.u32 = [np.zeros(R, np.uint32) for _ in range(7)]
        (self.flags, self.votes, self.ref_start, self.ref_end, self.read_start, self.read_end, self.err) = self.u32
        self.rid = np.zeros(R, np.uint32)
        self.tlen = np.zeros(max(npairs, 1), np.int64)
        self.alnA, self.alnB, self.off, self.cap = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(R + 1, np.uint64), cap

    def entries(self, refs: bool):
        u = [x.ctypes.data for x in self.u32]
        return (self.score.ctypes.data, self.second.ctypes.data, *u[:2], *([self.rid.ctypes.data] if refs else []), *u[2:])

    def strings(self):
        return (self.alnA.ctypes.data, self.alnB.ctypes.data, self.off.ctypes.data, self.cap)

    def aligned(self, i):
        o = self.off
        return self.alnA[int(o[i]):int(o[i + 1])].tobytes(), self.alnB[int(o[i]):int(o[i + 1])].tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from bench_map import make_reads
    from bench_map_pairs import make_pairs
    from poly_amd import _lib, align, alphabet, bwt, mapper, mash, matrix, refs
    assert torch.cuda.is_available(), "bench_map_refs.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(29)
    n, N, NP, m = args.genome, args.reads, args.pairs, 150
    P, PP, go, ge = mapper.MapParams(), mapper.PairParams(200, 500), -5, -2
    ab = alphabet.NewAlphabet(list("-ACGT"))
    sc = align.NewScoring(matrix.NewSubstitutionMatrix(ab, ab, matrix.NUC_4), -2)

    g_t = torch.empty(n, dtype=torch.uint8, device=dev)
    mash.synth_dna_dev(0x5EED + n, g_t)
    g = g_t.cpu().numpy()
    idx = bwt.new_dev(g_t)

    def cut(size):
        offs = np.append(np.arange(0, n, size, dtype=np.uint64), np.uint64(n))
        return refs.new_packed([f"c{i}" for i in range(len(offs) - 1)], g, offs)
    sets = {"refs_1": cut(n), "refs_5kb": cut(5_000), "refs_100": cut(100)}

    reads = make_reads(rng, g, N, m)
    off = np.arange(0, N * m + 1, m, dtype=np.uint64)
    m1, m2, _, _, _ = make_pairs(rng, g, NP, m)
    offp = np.arange(0, NP * m + 1, m, dtype=np.uint64)

    lib, p, pp = _lib.lib(), P._c(), PP._c()
    cap1, cap2 = int(1.3 * N * m), int(1.3 * 2 * NP * m)         # the strings are about 1.02 of the reads
    res = {"single": Out(N, cap1)}
    res.update({k: Out(N, cap1) for k in sets})
    res.update({k: Out(2 * NP, cap2, NP) for k in ("pairs_single", "pairs_refs_1", "pairs_refs_5kb")})

    def single_reads(h, name, fn, is_refs):
        o = res[name]
        return lambda: fn(h, sc.handle(), C.byref(p), go, ge, reads.ctypes.data, off.ctypes.data, N, m, 0, *o.entries(is_refs), *o.strings())

    def paired(h, name, fn, is_refs):
        o = res[name]
        return lambda: fn(h, sc.handle(), C.byref(p), C.byref(pp), go, ge, m1.ctypes.data, offp.ctypes.data, m2.ctypes.data,
                          offp.ctypes.data, NP, m, 0, *o.entries(is_refs), o.tlen.ctypes.data, *o.strings())
    calls = {"single": single_reads(idx.handle(), "single", lib.polyhip_map_reads_affine, False)}
    for k, s in sets.items():
        calls[k] = single_reads(s.handle(), k, lib.polyhip_map_reads_refs, True)
    calls["pairs_single"] = paired(idx.handle(), "pairs_single", lib.polyhip_map_pairs, False)
    calls["pairs_refs_1"] = paired(sets["refs_1"].handle(), "pairs_refs_1", lib.polyhip_map_pairs_refs, True)
    calls["pairs_refs_5kb"] = paired(sets["refs_5kb"].handle(), "pairs_refs_5kb", lib.polyhip_map_pairs_refs, True)

    if args.only:
        calls = {k: calls[k] for k in args.only.split(",")}
    times = {k: [] for k in calls}
    info, rinfo = {}, {}
    for rep in range(args.reps + 1):                           # round 0 warms up; the calls alternate
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(fn())
            dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt)
            else:
                info[name] = (mapper.last_pairs_info if name.startswith("pairs") else mapper.last_affine_info)()
                if "refs" in name:
                    rinfo[name] = mapper.last_refs_info()
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in times.items()}

    def same_place(name, base, s):
        o, b = res[name], res[base]
        at = o.ref_start.astype(np.int64) + s.starts[o.rid.astype(np.int64)]
        return float(((o.flags == b.flags) & (at == b.ref_start.astype(np.int64))).mean())
    same = {k: same_place(k, "single", sets[k]) for k in sets if k in calls and "single" in calls}
    for k in ("refs_1", "refs_5kb"):
        if "pairs_" + k in calls and "pairs_single" in calls:
            same["pairs_" + k] = same_place("pairs_" + k, "pairs_single", sets[k])
    one, base = res["refs_1"], res["single"]
    identical_one = "refs_1" not in calls or "single" not in calls or all((getattr(one, f) == getattr(base, f)).all() for f in FIELDS if f != "rid") and \
        (one.off == base.off).all() and (one.alnA[:int(one.off[N])] == base.alnA[:int(base.off[N])]).all()

    # four reads of the 5 kb set against the oracle
    import map_oracle as mo
    import map_refs_oracle as mro
    import sw_affine_oracle as ao
    s5 = sets["refs_5kb"]
    contigs = [g[int(a):int(b)].tobytes() for a, b in zip(s5.starts[:-1], s5.starts[1:])]
    Po = mo.Params(**dataclasses.asdict(P))
    got, spot = res["refs_5kb"], []
    for i in np.linspace(0, N - 1, 4).astype(int) if "refs_5kb" in calls else []:
        h = mro.map_read(contigs, reads[i].tobytes(), ao.NUC_4, go, ge, Po, mro.new_info(), m)
        spot.append(bool(all(int(getattr(got, f)[i]) == getattr(h, f) for f in FIELDS) and got.aligned(i) == (h.alignA, h.alignB)))

    out = {"device": torch.cuda.get_device_name(0), "genome": n, "reads": N, "pairs": NP, "read_len": m, "params": P.__dict__,
           "pair_params": PP.__dict__, "gaps": [go, ge], "reps": args.reps, "contigs": {k: len(s) for k, s in sets.items()},
           "seconds": med, "seconds_min": {k: min(v) for k, v in times.items()}, "seconds_all": times, "spread": spread,
           "over_single": {k: med[k] / med["single"] for k in sets if k in med and "single" in med},
           "pairs_over_single": {k: med[k] / med["pairs_single"] for k in ("pairs_refs_1", "pairs_refs_5kb")
                                 if k in med and "pairs_single" in med},
           "info": info, "refs_info": rinfo, "same_place": same, "one_contig_identical": bool(identical_one), "spot_check": spot}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    assert all(spot), "the refs mapper's results differ from the oracle's"
    assert identical_one, "one contig does not give the single-text call's outputs"


if __name__ == "__main__":
    main()
