"""The two base-quality calls on one MI355X, each beside the call it extends, in one run.

    python scripts/bench_base_qual.py [--genome 5000000] [--reads 1000000] [--records 200000] [--reps 5]
                                      [--only feeder|pileup] [--add-pass-ms T0,T20] [--out profiles/base_qual_bench.json]

- feeder: polyhip_fastq_pack_qual beside polyhip_fastq_pack on the README's image (--records records of 1 kb, one record
  repeated, 405 MB), through the host-pointer calls (the quality call has no device-resident flavour), alternating --reps
  times after a warm-up round; a host clock around each call, which includes the upload of the image, the device
  allocations and the copies back; medians;
- pileup: scripts/bench_pileup.py's workload and protocol -- a synthetic genome, reads of 150 bp with 5 % substitutions and
  1 % indels mapped once by polyhip_map_reads_affine, the records made once --, then polyhip_pileup (the parent's call,
  unchanged) and polyhip_pileup_qual at min_base_qual 0 and 20 over the whole text alternate --reps times after a warm-up
  round, through the host-pointer calls; medians.  Qualities: every read gets 150 bytes drawn so that about a tenth of the
  bases fall below 20 (Q 2..19 with probability 0.1, else 20..41);
- checks: at min_base_qual 0 counts, consensus, err and the shared info equal polyhip_pileup's; a window of 2,000 positions
  of the min_base_qual 20 call against tests/pileup_qual_oracle.py; the feeder's sequences and offsets equal
  polyhip_fastq_pack's and the quality bytes equal the image's;
- the kernels' own time is not taken here: run the script under a kernel trace in a run of its own (--only keeps the other
  half out of it).  --add-pass-ms hands the add pass's median time at min_base_qual 0 and 20 from such a trace back to a
  later run, which then writes the atomic adds per second beside M5's 8.0e10 (profiles/pileup_bench.json's workload);
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


def _alternate(calls, reps, sync):
    times = {k: [] for k in calls}
    for rep in range(reps + 1):                            # round 0 warms up; the calls alternate
        for name, fn in calls.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rep:
                times[name].append(time.perf_counter() - t0)
    return {k: float(np.median(v)) for k, v in times.items()}, times


def feeder(dev, records, reps):
    import torch
    from poly_amd import _lib
    rng = np.random.default_rng(1)
    L = 1000
    seq, qual = bytes(rng.choice(list(b"ACGT"), L).astype(np.uint8)), bytes(rng.integers(33, 74, L, dtype=np.uint8))
    rec = b"@r0000000 ch=1 start=2\n" + seq + b"\n+\n" + qual + b"\n"
    img = np.frombuffer(rec * records, np.uint8).copy()
    nb = len(img)
    most = nb // 7 + 1
    seqs, seqs_q, quals = (np.zeros(nb, np.uint8) for _ in range(3))
    offs, offs_q, qoffs = (np.zeros(most + 2, np.uint64) for _ in range(3))
    res, res_q = np.zeros(4, np.uint64), np.zeros(6, np.uint64)
    lib = _lib.lib()
    calls = {"fastq_pack": lambda: _lib.check(lib.polyhip_fastq_pack(img.ctypes.data, nb, seqs.ctypes.data, offs.ctypes.data, None, most,
                                                                     res.ctypes.data)),
             "fastq_pack_qual": lambda: _lib.check(lib.polyhip_fastq_pack_qual(img.ctypes.data, nb, seqs_q.ctypes.data, offs_q.ctypes.data,
                                                                               quals.ctypes.data, qoffs.ctypes.data, None, most,
                                                                               res_q.ctypes.data))}
    med, times = _alternate(calls, reps, torch.cuda.synchronize)
    r, rq = [int(x) for x in res], [int(x) for x in res_q]
    same = rq[:4] == r and rq[4:] == [records * L, 0] and bool((seqs_q[:r[3]] == seqs[:r[3]]).all()) and \
        bool((offs_q[:records + 1] == offs[:records + 1]).all()) and bool((qoffs[:records + 1] == offs[:records + 1]).all()) and \
        quals[:2 * L].tobytes() == qual * 2 and quals[rq[4] - L:rq[4]].tobytes() == qual
    bytes_plain, bytes_qual = nb + r[3] + 8 * (records + 1), nb + r[3] + rq[4] + 16 * (records + 1)
    return {"workload": f"FASTQ image of {records} records x {L} bp ({nb} B), host pointers", "seconds": med, "seconds_all": times,
            "qual_over_plain": med["fastq_pack_qual"] / med["fastq_pack"], "host_link_bytes_plain": bytes_plain,
            "host_link_bytes_qual": bytes_qual, "host_link_GBps_plain": bytes_plain / med["fastq_pack"] / 1e9,
            "host_link_GBps_qual": bytes_qual / med["fastq_pack_qual"] / 1e9, "result_plain": r, "result_qual": rq,
            "outputs_agree": bool(same)}


M5_ADDS_PER_SECOND = 8.0e10           # polyhip_pileup's add pass on this workload


def pile(dev, n, N, reps, add_pass_ms=None):
    import torch
    from bench_map import make_reads
    from poly_amd import _lib, align, alphabet, bwt, mapper, mash, matrix, pileup, sam
    import pileup_qual_oracle as qo
    rng = np.random.default_rng(17)
    m = 150
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
    _lib.check(lib.polyhip_map_reads_affine(idx.handle(), sc.handle(), C.byref(p), -5, -2, buf.ctypes.data, offs.ctypes.data, N, m, 0,
                                            score.ctypes.data, second.ctypes.data, *[x.ctypes.data for x in u32], alnA.ctypes.data,
                                            alnB.ctypes.data, aoff.ctypes.data, cap))
    read_len = np.full(N, m, np.uint32)
    rp = sam._CParams(0, 0)
    coff, moff = np.zeros(N + 1, np.uint64), np.zeros(N + 1, np.uint64)
    nm, sf, rerr, mapq = np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(N, np.uint8)
    rc = lib.polyhip_aln_records(C.byref(rp), N, flags.ctypes.data, score.ctypes.data, second.ctypes.data, read_start.ctypes.data,
                                 read_end.ctypes.data, read_len.ctypes.data, alnA.ctypes.data, alnB.ctypes.data, aoff.ctypes.data,
                                 coff.ctypes.data, None, 0, moff.ctypes.data, None, 0, nm.ctypes.data, mapq.ctypes.data, sf.ctypes.data,
                                 rerr.ctypes.data)                  # the sizes: mapq is filled either way
    assert rc in (_lib.OK, _lib.ERR_INVALID)
    # qualities of the reads as sequenced: about a tenth of the bases below 20
    qual = np.where(rng.random(N * m) < 0.1, rng.integers(2, 20, N * m), rng.integers(20, 42, N * m)).astype(np.uint8) + np.uint8(33)
    qoff = offs

    settings = dict(min_mapq=20, min_depth=4, min_alt_count=2, min_alt_permille=500)
    base = pileup._CParams(0, n, settings["min_mapq"], settings["min_depth"], settings["min_alt_count"], settings["min_alt_permille"])
    perr, qerr, nsites = np.zeros(N, np.uint32), np.zeros(N, np.uint32), C.c_uint64(0)
    counts, consensus = np.zeros((pileup.CHANNELS, n), np.uint32), np.zeros(n, np.uint8)
    qcounts, qsum, qcons = np.zeros((pileup.CHANNELS, n), np.uint32), np.zeros((pileup.QSUM_PLANES, n), np.uint32), np.zeros(n, np.uint8)
    scap = 1 << 20
    sites, qsites = np.zeros(scap, pileup.SITE_DTYPE), np.zeros(scap, pileup.SITE_DTYPE)

    def plain():
        _lib.check(lib.polyhip_pileup(C.byref(base), N, flags.ctypes.data, mapq.ctypes.data, ref_start.ctypes.data, ref_end.ctypes.data,
                                      alnA.ctypes.data, alnB.ctypes.data, aoff.ctypes.data, text.ctypes.data, n, counts.ctypes.data,
                                      consensus.ctypes.data, C.byref(nsites), sites.ctypes.data, scap, perr.ctypes.data))

    def with_qual(threshold, lo=0, hi=n, out=None):
        qp = pileup._CQualParams(pileup._CParams(lo, hi, *[settings[k] for k in ("min_mapq", "min_depth", "min_alt_count", "min_alt_permille")]),
                                 threshold, 33)
        c, s, k = out or (qcounts, qsum, qcons)
        _lib.check(lib.polyhip_pileup_qual(C.byref(qp), N, flags.ctypes.data, mapq.ctypes.data, ref_start.ctypes.data, ref_end.ctypes.data,
                                           read_start.ctypes.data, alnA.ctypes.data, alnB.ctypes.data, aoff.ctypes.data, qual.ctypes.data,
                                           qoff.ctypes.data, text.ctypes.data, n, c.ctypes.data, s.ctypes.data, k.ctypes.data,
                                           C.byref(nsites), qsites.ctypes.data, scap, qerr.ctypes.data))

    calls = {"pileup": plain, "pileup_qual_0": lambda: with_qual(0), "pileup_qual_20": lambda: with_qual(20)}
    med, times = _alternate(calls, reps, torch.cuda.synchronize)
    plain()
    info = pileup.last_info()
    with_qual(0)
    info0 = pileup.last_qual_info()
    identity = bool((qcounts == counts).all() and (qcons == consensus).all() and (qerr == perr).all() and
                    {k: info0[k] for k in info} == info and info0["filtered_bases"] == 0)
    adds0 = int(qcounts.sum(dtype=np.uint64)) + info0["edge_events"]
    qadds0 = int(qcounts[[0, 1, 2, 3, 8, 9, 10, 11]].sum(dtype=np.uint64))
    with_qual(20)
    info20 = pileup.last_qual_info()
    adds20 = int(qcounts.sum(dtype=np.uint64)) + info20["edge_events"]
    qadds20 = int(qcounts[[0, 1, 2, 3, 8, 9, 10, 11]].sum(dtype=np.uint64))
    # a window of the threshold-20 call against the oracle, on the entries that touch it
    lo, hi = n // 5, n // 5 + 2000
    mapped = (flags & 1) == 1
    near = np.nonzero(mapped & (ref_start <= hi) & (ref_end >= lo))[0]
    cols = np.diff(aoff.astype(np.int64))
    a_all, b_all, q_all = alnA.tobytes(), alnB.tobytes(), qual.tobytes()
    sub_off = np.zeros(len(near) + 1, np.uint64)
    sub_off[1:] = np.cumsum(cols[near])
    sub_q = np.arange(0, len(near) * m + 1, m, dtype=np.uint64)
    want = qo.pileup_qual(flags[near], mapq[near], ref_start[near], ref_end[near], read_start[near],
                          b"".join(a_all[int(aoff[i]):int(aoff[i + 1])] for i in near),
                          b"".join(b_all[int(aoff[i]):int(aoff[i + 1])] for i in near), sub_off,
                          b"".join(q_all[int(i) * m:(int(i) + 1) * m] for i in near), sub_q, text.tobytes(), region=(lo, hi), min_base_qual=20,
                          **settings)
    spot = bool((qcounts[:, lo:hi] == want.counts).all() and (qsum[:, lo:hi] == want.qsum).all() and (qcons[lo:hi] == want.consensus).all())
    strings = int(aoff[N])
    bytes_in = 2 * strings + n + 8 * (N + 1) + N * (3 * 4 + 1)
    bytes_out = 4 * pileup.CHANNELS * n + n + 4 * N
    more_in, more_out = N * m + 8 * (N + 1) + 4 * N, 4 * pileup.QSUM_PLANES * n
    rate = {}
    if add_pass_ms:
        rate = {"add_pass_ms_from_kernel_trace": {"pileup_qual_0": add_pass_ms[0], "pileup_qual_20": add_pass_ms[1]},
                "atomic_adds_per_second": {"pileup_qual_0": (adds0 + qadds0) / add_pass_ms[0] * 1e3,
                                           "pileup_qual_20": (adds20 + qadds20) / add_pass_ms[1] * 1e3, "pileup_M5": M5_ADDS_PER_SECOND}}
    return {**rate, "genome": n, "reads": N, "read_len": m, "settings": settings, "seconds": med, "seconds_all": times,
            "qual0_over_plain": med["pileup_qual_0"] / med["pileup"], "qual20_over_plain": med["pileup_qual_20"] / med["pileup"],
            "info_plain": info, "info_qual_0": info0, "info_qual_20": info20,
            "filtered_share_of_bases": info20["filtered_bases"] / max(adds0 - info0["edge_events"], 1),
            "atomic_adds": {"pileup": adds0, "pileup_qual_0": adds0 + qadds0, "pileup_qual_20": adds20 + qadds20},
            "bytes_in_plain": bytes_in, "bytes_out_plain": bytes_out, "bytes_in_qual": bytes_in + more_in, "bytes_out_qual": bytes_out + more_out,
            "host_link_GBps_plain": (bytes_in + bytes_out) / med["pileup"] / 1e9,
            "host_link_GBps_qual_0": (bytes_in + bytes_out + more_in + more_out) / med["pileup_qual_0"] / 1e9,
            "identity_at_0": identity, "spot_check_at_20": spot, "spot_entries": int(len(near))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--records", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("feeder", "pileup"), default=None)
    ap.add_argument("--add-pass-ms", default=None, help="T0,T20: the add pass's time in a kernel trace of a run of its own")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    add_pass_ms = [float(x) for x in args.add_pass_ms.split(",")] if args.add_pass_ms else None
    import torch
    assert torch.cuda.is_available(), "bench_base_qual.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    if args.only != "pileup":
        out["feeder"] = feeder(dev, args.records, args.reps)
    if args.only != "feeder":
        out["pileup"] = pile(dev, args.genome, args.reads, args.reps, add_pass_ms)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    assert out.get("feeder", {}).get("outputs_agree", True), "the feeder's outputs differ"
    assert out.get("pileup", {}).get("identity_at_0", True) and out.get("pileup", {}).get("spot_check_at_20", True), "the pileup differs"


if __name__ == "__main__":
    main()
