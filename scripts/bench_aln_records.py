"""polyhip_aln_records on one MI355X beside the mapping call whose output it reads, through the host-pointer calls, in one run.

    python scripts/bench_aln_records.py [--genome 5000000] [--reads 1000000] [--reps 3] [--out profiles/aln_records_bench.json]

- workload: scripts/bench_map_affine.py's -- a synthetic genome, reads of 150 bp sampled from it with 5 % substitutions and
  1 % indels, every second one reverse-complemented; default parameters (mapper.MapParams), gaps (-5, -2);
- protocol: the reads are mapped once; then polyhip_aln_records on that result and polyhip_map_reads_affine itself alternate
  --reps times after one warm-up round; a host clock around each call, which ends in a stream synchronise and includes the
  copies in and out; medians are reported;
- bytes: what the records call copies to the device (the two strings, the offsets, six per-entry arrays) and back (the two
  scans, the CIGAR entries, the MD bytes, four per-entry arrays); kernel_bytes: what its two passes read and write on the
  device -- each pass reads both strings once;
- the kernels' own time is not taken here: run the script under a kernel trace in a run of its own;
- spot check: every 1000th entry, and the info counters, against tests/aln_records_oracle.py.
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
    from poly_amd import _lib, align, alphabet, bwt, mapper, mash, matrix, sam
    assert torch.cuda.is_available(), "bench_aln_records.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(17)
    n, N, m = args.genome, args.reads, 150
    P = mapper.MapParams()
    ab = alphabet.NewAlphabet(list("-ACGT"))
    sc = align.NewScoring(matrix.NewSubstitutionMatrix(ab, ab, matrix.NUC_4), -2)
    g_t = torch.empty(n, dtype=torch.uint8, device=dev)
    mash.synth_dna_dev(0x5EED + n, g_t)
    idx = bwt.new_dev(g_t)
    reads = make_reads(rng, g_t.cpu().numpy(), N, m)
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
    map_info = mapper.last_affine_info()
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
    calls = {"aln_records": lambda: rec_call(cigar, nc, md, nb), "map_reads_affine": map_call}
    times = {k: [] for k in calls}
    for rep in range(args.reps + 1):                       # round 0 warms up; the calls alternate
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(fn())
            dt = time.perf_counter() - t0
            if rep:
                times[name].append(dt)
    info = sam.last_info()                                  # of the last records call: the map call keeps its own
    med = {k: float(np.median(v)) for k, v in times.items()}

    import aln_records_oracle as aro
    pick = np.arange(0, N, 1000)
    a_all, b_all = alnA.tobytes(), alnB.tobytes()
    spot = True
    for i in pick:
        o0, o1 = int(aoff[i]), int(aoff[i + 1])
        e = aro.one(bool(flags[i] & 1), o1 - o0, a_all[o0:o1], b_all[o0:o1], int(read_start[i]), int(read_end[i]), m, int(score[i]),
                    int(second[i]), False)
        spot &= (e.err, e.nm, e.mapq) == (int(rerr[i]), int(nm[i]), int(mapq[i]))
        spot &= e.cigar == cigar[int(coff[i]):int(coff[i + 1])].tolist() and e.md == md[int(moff[i]):int(moff[i + 1])].tobytes()
    live = (sf & 4) == 0
    cols = np.diff(aoff.astype(np.int64))
    counters_ok = info == dict(entries=N, mapped=int(live.sum()), columns=int(cols[live].sum()), cigar_ops=nc, md_bytes=nb, bad=int((rerr != 0).sum()))

    strings = int(aoff[N])
    bytes_in = 2 * strings + 8 * (N + 1) + N * (4 * 4 + 2 * 8)
    bytes_out = 2 * 8 * (N + 1) + 4 * nc + nb + N * (3 * 4 + 1)
    out = {"device": torch.cuda.get_device_name(0), "genome": n, "reads": N, "read_len": m, "reps": args.reps, "seconds": med,
           "seconds_all": times, "records_over_mapping": med["aln_records"] / med["map_reads_affine"], "info": info,
           "map_info": map_info, "bytes_in": bytes_in, "bytes_out": bytes_out,
           "host_link_GBps": (bytes_in + bytes_out) / med["aln_records"] / 1e9,
           "kernel_bytes": 2 * 2 * info["columns"] + 4 * nc + nb, "spot_check": bool(spot), "counters_ok": bool(counters_ok)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    assert spot and counters_ok, "the records differ from the oracle's"


if __name__ == "__main__":
    main()
