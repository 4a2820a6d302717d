"""polyhip_pileup on one MI355X beside the two calls whose output it reads, through the host-pointer calls, in one run.

    python scripts/bench_pileup.py [--genome 5000000] [--reads 1000000] [--reps 3] [--out profiles/pileup_bench.json]

- workload: scripts/bench_map_affine.py's -- a synthetic genome, reads of 150 bp sampled from it with 5 % substitutions and
  1 % indels, every second one reverse-complemented; default parameters (mapper.MapParams), gaps (-5, -2);
- protocol: the reads are mapped once and the records made once; then polyhip_pileup over the whole text (min_mapq 20, sites
  at 500 permille of a depth of at least 4), polyhip_aln_records, polyhip_map_reads_affine and polyhip_pileup at a setting
  that reports a site wherever one read in about thirty disagrees alternate --reps times after one warm-up round; a host
  clock around each call, which ends in a stream synchronise and includes the copies in and out; medians are reported;
- bytes: what the pileup call copies to the device (the two strings, the text, the offsets, three per-entry arrays and mapq)
  and back (16 planes of counts, the consensus, err, the sites); atomic_adds: the adds its accumulate pass issues, i.e. the
  sum of all counts plus the events dropped at the text's start;
- the kernels' own time is not taken here: run the script under a kernel trace in a run of its own;
- spot check: a window of 2,000 positions -- counts, consensus and sites of the whole-text call, and of a call on that
  region alone, against tests/pileup_oracle.py on the entries that touch it -- and the info counters against numpy.
Prints one JSON object (and writes it to --out).  Nothing here has a speed threshold.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from bench_map import make_reads
    from poly_amd import _lib, align, alphabet, bwt, mapper, mash, matrix, pileup, sam
    assert torch.cuda.is_available(), "bench_pileup.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(17)
    n, N, m = args.genome, args.reads, 150
    P = mapper.MapParams()
    ab = alphabet.NewAlphabet(list("-ACGT"))
    sc = align.NewScoring(matrix.NewSubstitutionMatrix(ab, ab, matrix.NUC_4), -2)
    g_t = torch.empty(n, dtype=torch.uint8, device=dev)
    mash.synth_dna_dev(0x5EED + n, g_t)
    idx = bwt.new_dev(g_t)
    text = np.ascontiguousarray(g_t.cpu().numpy())
    reads = make_reads(rng, text, N, m)
    buf = reads.reshape(-1)
    offs = np.arange(0, N * m + 1, m, dtype=np.uint64)
    cap = 2 * N * m

    lib, p = _lib.lib(), P._c()
    score, second = np.zeros(N, np.int64), np.zeros(N, np.int64)
    u32 = [np.zeros(N, np.uint32) for _ in range(7)]
    flags, votes, ref_start, ref_end, read_start, read_end, err = u32
    alnA, alnB, aoff = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(N + 1, np.uint64)

    def map_call():
        return lib.polyhip_map_reads_affine(idx.handle(), sc.handle(), C.byref(p), -5, -2, buf.ctypes.data, offs.ctypes.data, N, m, 0,
                                            score.ctypes.data, second.ctypes.data, *[x.ctypes.data for x in u32], alnA.ctypes.data,
                                            alnB.ctypes.data, aoff.ctypes.data, cap)

    _lib.check(map_call())
    read_len = np.full(N, m, np.uint32)
    rp = sam._CParams(0, 0)
    coff, moff = np.zeros(N + 1, np.uint64), np.zeros(N + 1, np.uint64)
    nm, sf, rerr, mapq = np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint8)

    def rec_call(cigar, ccap, md, mcap):
        return lib.polyhip_aln_records(C.byref(rp), N, flags.ctypes.data, score.ctypes.data, second.ctypes.data, read_start.ctypes.data,
                                       read_end.ctypes.data, read_len.ctypes.data, alnA.ctypes.data, alnB.ctypes.data, aoff.ctypes.data,
                                       coff.ctypes.data, cigar.ctypes.data if cigar is not None else None, ccap, moff.ctypes.data,
                                       md.ctypes.data if md is not None else None, mcap, nm.ctypes.data, mapq.ctypes.data, sf.ctypes.data,
                                       rerr.ctypes.data)

    assert rec_call(None, 0, None, 0) in (_lib.OK, _lib.ERR_INVALID)          # the sizes
    nc, nb = int(coff[N]), int(moff[N])
    cigar, md = np.zeros(max(nc, 1), np.uint32), np.zeros(max(nb, 1), np.uint8)
    _lib.check(rec_call(cigar, nc, md, nb))                                  # mapq for the pileup

    settings = dict(min_mapq=20, min_depth=4, min_alt_count=2, min_alt_permille=500)
    perr, nsites = np.zeros(N, np.uint32), C.c_uint64(0)

    def pile_call(lo, hi, counts, consensus, sites, scap, st=settings):
        pp = pileup._CParams(lo, hi, st["min_mapq"], st["min_depth"], st["min_alt_count"], st["min_alt_permille"])
        return lib.polyhip_pileup(C.byref(pp), N, flags.ctypes.data, mapq.ctypes.data, ref_start.ctypes.data, ref_end.ctypes.data,
                                  alnA.ctypes.data, alnB.ctypes.data, aoff.ctypes.data, text.ctypes.data, n, counts.ctypes.data,
                                  consensus.ctypes.data, C.byref(nsites), sites.ctypes.data if sites is not None else None, scap,
                                  perr.ctypes.data)

    counts, consensus = np.zeros((pileup.CHANNELS, n), np.uint32), np.zeros(n, np.uint8)
    assert pile_call(0, n, counts, consensus, None, 0) in (_lib.OK, _lib.ERR_INVALID)   # the size
    ns = int(nsites.value)
    sites = np.zeros(max(ns, 1), pileup.SITE_DTYPE)
    # the reads' errors are independent, so the settings above find no site; a second setting reports nearly every read error
    loose = dict(min_mapq=0, min_depth=1, min_alt_count=1, min_alt_permille=30)
    assert pile_call(0, n, counts, consensus, None, 0, loose) in (_lib.OK, _lib.ERR_INVALID)
    ns_loose = int(nsites.value)
    sites_loose = np.zeros(max(ns_loose, 1), pileup.SITE_DTYPE)
    calls = {"pileup": lambda: pile_call(0, n, counts, consensus, sites, ns), "aln_records": lambda: rec_call(cigar, nc, md, nb),
             "map_reads_affine": map_call, "pileup_many_sites": lambda: pile_call(0, n, counts, consensus, sites_loose, ns_loose, loose)}
    times = {k: [] for k in calls}
    for rep in range(args.reps + 1):                       # round 0 warms up; the calls alternate
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(fn())
            dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt)
            if name == "pileup":
                info = pileup.last_info()                   # of this pileup call: the other calls keep their own
    med = {k: float(np.median(v)) for k, v in times.items()}
    _lib.check(calls["pileup"]())                           # untimed: the outputs that the checks below read

    # ---- the info counters against numpy, a window against the oracle
    mapped = (flags & 1) == 1
    skipped = mapped & (mapq < settings["min_mapq"])
    used = mapped & ~skipped & (perr == 0)
    cols = np.diff(aoff.astype(np.int64))
    counters_ok = info == dict(entries=N, used=int(used.sum()), skipped_mapq=int(skipped.sum()), bad=int((perr != 0).sum()),
                               columns=int(cols[used].sum()), edge_events=info["edge_events"], sites=ns)
    atomic_adds = int(counts.sum(dtype=np.uint64)) + info["edge_events"]
    import pileup_oracle as po
    lo, hi = n // 5, n // 5 + 2000
    near = np.nonzero(mapped & (ref_start <= hi) & (ref_end >= lo))[0]
    a_all, b_all = alnA.tobytes(), alnB.tobytes()
    sub_off = np.zeros(len(near) + 1, np.uint64)
    sub_off[1:] = np.cumsum(cols[near])
    want = po.pileup(flags[near], mapq[near], ref_start[near], ref_end[near], b"".join(a_all[int(aoff[i]):int(aoff[i + 1])] for i in near),
                     b"".join(b_all[int(aoff[i]):int(aoff[i + 1])] for i in near), sub_off, text.tobytes(), region=(lo, hi), **settings)
    in_window = sites[(sites["pos"] >= lo) & (sites["pos"] < hi)]
    spot = (counts[:, lo:hi] == want.counts).all() and (consensus[lo:hi] == want.consensus).all() and (in_window == want.sites).all()
    c2, k2, s2 = np.zeros((pileup.CHANNELS, hi - lo), np.uint32), np.zeros(hi - lo, np.uint8), np.zeros(max(len(want.sites), 1), pileup.SITE_DTYPE)
    _lib.check(pile_call(lo, hi, c2, k2, s2, len(want.sites)))
    spot = bool(spot and (c2 == want.counts).all() and (k2 == want.consensus).all() and (s2[:len(want.sites)] == want.sites).all())

    strings = int(aoff[N])
    bytes_in = 2 * strings + n + 8 * (N + 1) + N * (3 * 4 + 1)
    bytes_out = 4 * pileup.CHANNELS * n + n + 4 * N + 20 * ns
    depth = counts[0:6].sum(axis=0, dtype=np.uint64) + counts[8:14].sum(axis=0, dtype=np.uint64)
    kinds = {k: int((sites["kind"][:ns] == v).sum()) for k, v in (("snv", 1), ("ins", 2), ("del", 3))}
    out = {"device": torch.cuda.get_device_name(0), "genome": n, "reads": N, "read_len": m, "reps": args.reps, "settings": settings,
           "seconds": med, "seconds_all": times, "pileup_over_records": med["pileup"] / med["aln_records"],
           "pileup_over_mapping": med["pileup"] / med["map_reads_affine"], "info": info, "many_sites_settings": loose,
           "many_sites": ns_loose, "sites_by_kind": kinds,
           "mean_depth": float(depth.mean()), "max_depth": int(depth.max()), "atomic_adds": atomic_adds,
           "atomic_adds_per_column": atomic_adds / max(info["columns"], 1), "bytes_in": bytes_in, "bytes_out": bytes_out,
           "host_link_GBps": (bytes_in + bytes_out) / med["pileup"] / 1e9, "spot_check": spot, "spot_entries": int(len(near)),
           "counters_ok": bool(counters_ok)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    assert spot and counters_ok, "the pileup differs from the oracle's"


if __name__ == "__main__":
    main()
