"""The demultiplexer on one MI355X: polyhip_demux_reads beside polyhip_trim_reads on the same reads, and polyhip_demux_pairs with
dual barcodes, in one run.

    python scripts/bench_demux.py [--reads 1000000] [--pairs 500000] [--genome 5000000] [--reps 5] [--only reads|pairs]
                                  [--out profiles/demux_bench.json]
    python scripts/bench_demux.py --kernel-trace KERNEL_TRACE.csv --into profiles/demux_bench.json      (no GPU needed)

- reads: --reads reads of 150 bp with qualities, each an 8-byte barcode of a set of 384 (pairwise Hamming distance >= 3) followed
  by 142 random bases; a tenth of the reads have one substitution in the barcode, a hundredth carry no barcode (150 random
  bases).  polyhip_demux_reads with max_shift 0 and with max_shift 3 (max_mismatches 1, min_margin 1, clip 1) and
  polyhip_trim_reads on the same packed batch (bench_trim.py's settings: both quality cut-offs at 20, one adapter, min_len 20)
  alternate --reps times after a warm-up round, through the host-pointer calls: a host clock around each call, which includes
  the copies in, the device allocations and the copies back; medians.  The ratio reported is demux over trim in this run;
- pairs: scripts/bench_map_pairs.py's pairs (2 x 150 bp from a synthetic genome) with one of 96 barcodes of 8 bytes in front
  of each mate and a 96 x 96 table that names a sample for every combination (9216 samples), polyhip_demux_pairs with max_shift
  0, --reps times after a warm-up;
- checks: the decisions for the first 1,000 reads and the first 500 pairs against tests/demux_oracle.py, the sample of every
  tagged read against the barcode it was given, and the grouped batch against the input permuted by `order`;
- the kernels' own time is not taken here: run the script under a kernel trace in a run of its own (rocprofv3 --kernel-trace
  --stats, csv output) and fold the trace's kernel_trace.csv into the JSON with the second form above.
Prints one JSON object (and writes it to --out).  Nothing here has a speed threshold.
"""
from __future__ import annotations

import argparse
import csv
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

ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
ACGT = np.frombuffer(b"ACGT", np.uint8)
NONE = 0xFFFFFFFF
KERNELS = ("match_kernel", "assign_kernel", "radix_hist_kernel", "radix_scatter_kernel", "starts_kernel", "place_kernel", "scan_apply_kernel",
           "scan_reduce_kernel", "gather_kernel")


def _alternate(calls, reps):
    times = {k: [] for k in calls}
    for rep in range(reps + 1):                            # round 0 warms up; the calls alternate; every call ends synchronised
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                times[name].append(time.perf_counter() - t0)
    return {k: float(np.median(v)) for k, v in times.items()}, times


def barcode_set(rng, n, length=8, min_dist=3):
    """n barcodes as rows of letter codes 0..3, pairwise at Hamming distance >= min_dist: greedy over a shuffle of all strings"""
    every = rng.permutation(4 ** length)
    codes = (every[:, None] >> (2 * np.arange(length))[None, :] & 3).astype(np.uint8)
    chosen = np.empty((n, length), np.uint8)
    k = 0
    for c in codes:
        if k == 0 or ((chosen[:k] != c).sum(axis=1) >= min_dist).all():
            chosen[k] = c
            k += 1
            if k == n:
                return chosen
    raise RuntimeError(f"only {k} of {n} barcodes of {length} bytes at distance {min_dist}")


def _tag(rng, body, codes, subst_share, none_share):
    """body with barcode which[i] of `codes` in front of row i; -> (reads, which, substituted), which = -1: no barcode"""
    n, p = len(body), codes.shape[1]
    which = rng.integers(0, len(codes), n)
    tags = codes[which].copy()
    x = rng.random(n)
    subst = x < subst_share
    rows = np.nonzero(subst)[0]
    cols = rng.integers(0, p, len(rows))
    tags[rows, cols] = (tags[rows, cols] + rng.integers(1, 4, len(rows))) & 3
    none = (x >= subst_share) & (x < subst_share + none_share)
    tags[none] = rng.integers(0, 4, (int(none.sum()), p))
    which[none] = -1
    return np.ascontiguousarray(np.concatenate([ACGT[tags], body], axis=1)), which, subst


def _packed_set(codes):
    return np.ascontiguousarray(ACGT[codes]).reshape(-1), np.arange(0, codes.size + 1, codes.shape[1], dtype=np.uint32)


def _params(nsamples, **kw):
    from poly_amd import demux
    return demux.DemuxParams(**kw)._c(nsamples)


def _permuted(reads, out, ooff, order, cut):
    """the grouped batch is the input permuted by order, input read i without its first cut[i] bytes"""
    m = reads.shape[1]
    lens = np.diff(ooff.astype(np.int64))
    if not (lens == m - cut[order]).all():
        return False
    at, got, cols = ooff[:-1].astype(np.int64), np.append(out[:int(ooff[-1])], np.zeros(m, np.uint8)), np.arange(m)
    for j0 in range(0, len(order), 100_000):               # a block of output reads at a time: their bytes by their offsets
        sl = slice(j0, j0 + 100_000)
        rows, c = reads[order[sl]], cut[order[sl]][:, None]
        src = np.take_along_axis(rows, np.minimum(c + cols, m - 1), axis=1)
        if not ((got[at[sl][:, None] + cols] == src) | (cols >= m - c)).all():
            return False
    return True


def _cuts(sample_of_entry, bstart, p):
    """what the clip takes off every entry: the barcode's start and length where the read (pair) is assigned"""
    return np.where(sample_of_entry != NONE, bstart.astype(np.int64) + p, 0)


def bench_reads(N, reps):
    from poly_amd import _lib, demux, trim
    import demux_oracle as do
    rng = np.random.default_rng(41)
    m, p, nbc = 150, 8, 384
    codes = barcode_set(rng, nbc, p, 3)
    reads, which, subst = _tag(rng, rng.choice(ACGT, (N, m - p)), codes, 0.1, 0.01)
    quals = (rng.integers(20, 42, (N, m)) + 33).astype(np.uint8)
    off = np.arange(0, N * m + 1, m, dtype=np.uint64)
    bc, bcoff = _packed_set(codes)
    lib = _lib.lib()
    barcode, bstart, mism, flags, err, sample, order = (np.zeros(N, np.uint32) for _ in range(7))
    starts = np.zeros(nbc + 2, np.uint64)
    out, outq, ooff = np.zeros(N * m, np.uint8), np.zeros(N * m, np.uint8), np.zeros(N + 1, np.uint64)
    tp = trim.TrimParams(min_qual_3p=20, min_qual_5p=20, adapter_err_pct=10, min_overlap=3, min_len=20)._c()
    ad, adoff = np.frombuffer(ADAPTER, np.uint8).copy(), np.array([0, len(ADAPTER)], np.uint32)
    t_start, t_end, t_flags, t_err = (np.zeros(N, np.uint32) for _ in range(4))

    def split(shift):
        prm = _params(nbc, max_shift=shift, max_mismatches=1, min_margin=1, clip=1)
        _lib.check(lib.polyhip_demux_reads(C.byref(prm), bc.ctypes.data, bcoff.ctypes.data, nbc, reads.ctypes.data, off.ctypes.data,
                                           quals.ctypes.data, off.ctypes.data, N, barcode.ctypes.data, bstart.ctypes.data, mism.ctypes.data,
                                           flags.ctypes.data, err.ctypes.data, sample.ctypes.data, order.ctypes.data, starts.ctypes.data,
                                           out.ctypes.data, outq.ctypes.data, ooff.ctypes.data))

    def cut():
        _lib.check(lib.polyhip_trim_reads(C.byref(tp), ad.ctypes.data, adoff.ctypes.data, 1, reads.ctypes.data, off.ctypes.data, quals.ctypes.data,
                                          off.ctypes.data, N, t_start.ctypes.data, t_end.ctypes.data, t_flags.ctypes.data, t_err.ctypes.data,
                                          out.ctypes.data, outq.ctypes.data, ooff.ctypes.data))

    med, times = _alternate({"trim_reads": cut, "demux_reads_shift0": lambda: split(0), "demux_reads_shift3": lambda: split(3)}, reps)
    k = min(N, 1000)
    rows = [reads[i].tobytes() for i in range(k)]
    barcodes = [ACGT[c].tobytes() for c in codes]
    infos, agree, right, grouped = {}, {}, {}, {}
    for shift in (0, 3):
        split(shift)
        name = f"demux_reads_shift{shift}"
        infos[name] = demux.last_info()
        want = do.demux_reads(rows, barcodes, None, max_shift=shift, max_mismatches=1, min_margin=1)
        agree[name] = bool(all((x[:k] == getattr(want, f)).all() for f, x in (("barcode", barcode), ("bstart", bstart), ("mism", mism),
                                                                            ("flags", flags), ("err", err), ("sample", sample))))
        tagged = which >= 0
        right[name] = float((sample[tagged] == which[tagged]).mean())
        grouped[name] = _permuted(reads, out, ooff, order, _cuts(sample, bstart, p)) and bool((np.sort(order) == np.arange(N)).all()) and int(starts[-1]) == N
    return {"workload": f"{N} reads x {m} bp with qualities, {nbc} barcodes of {p} bytes at pairwise distance >= 3, "
                        f"{int(subst.sum())} reads with one barcode substitution, {int((which < 0).sum())} without a barcode",
            "settings": {"max_mismatches": 1, "min_margin": 1, "clip": 1, "max_shift": [0, 3]}, "seconds": med, "seconds_all": times,
            "demux_over_trim": {kk: med[kk] / med["trim_reads"] for kk in med if kk != "trim_reads"},
            "reads_per_s": {kk: N / v for kk, v in med.items()}, "info": infos,
            "host_link_bytes_in": 2 * N * m + 16 * (N + 1), "tagged_reads_in_their_sample": right, "grouped_batch_is_the_input_permuted": grouped,
            "agrees_with_oracle": agree, "oracle_reads": k}


def bench_pairs(N, n, reps):
    import torch
    from bench_map_pairs import make_pairs
    from poly_amd import _lib, demux, mash
    import demux_oracle as do
    rng = np.random.default_rng(43)
    m, p, nbc = 150, 8, 96
    g_t = torch.empty(n, dtype=torch.uint8, device=torch.device("cuda:0"))
    mash.synth_dna_dev(0x5EED + n, g_t)
    g = g_t.cpu().numpy()
    del g_t
    m1, m2, _, _, _ = make_pairs(rng, g, N, m)
    codes1, codes2 = barcode_set(rng, nbc, p, 3), barcode_set(rng, nbc, p, 3)
    m1, which1, _ = _tag(rng, m1, codes1, 0.1, 0.01)
    m2, which2, _ = _tag(rng, m2, codes2, 0.1, 0.01)
    L = m + p
    q1, q2 = (rng.integers(20, 42, (N, L)) + 33).astype(np.uint8), (rng.integers(20, 42, (N, L)) + 33).astype(np.uint8)
    off = np.arange(0, N * L + 1, L, dtype=np.uint64)
    (bc1, bo1), (bc2, bo2) = _packed_set(codes1), _packed_set(codes2)
    table = np.arange(nbc * nbc, dtype=np.uint32)
    nsamples = nbc * nbc
    lib = _lib.lib()
    barcode, bstart, mism, flags, err = (np.zeros(2 * N, np.uint32) for _ in range(5))
    sample, order, starts = np.zeros(N, np.uint32), np.zeros(N, np.uint32), np.zeros(nsamples + 2, np.uint64)
    o1, oq1, oo1 = np.zeros(N * L, np.uint8), np.zeros(N * L, np.uint8), np.zeros(N + 1, np.uint64)
    o2, oq2, oo2 = np.zeros(N * L, np.uint8), np.zeros(N * L, np.uint8), np.zeros(N + 1, np.uint64)
    prm = _params(nsamples, max_shift=0, max_mismatches=1, min_margin=1, clip=1)

    def split():
        _lib.check(lib.polyhip_demux_pairs(C.byref(prm), bc1.ctypes.data, bo1.ctypes.data, nbc, bc2.ctypes.data, bo2.ctypes.data, nbc,
                                           table.ctypes.data, m1.ctypes.data, off.ctypes.data, q1.ctypes.data, off.ctypes.data, m2.ctypes.data,
                                           off.ctypes.data, q2.ctypes.data, off.ctypes.data, N, barcode.ctypes.data, bstart.ctypes.data,
                                           mism.ctypes.data, flags.ctypes.data, err.ctypes.data, sample.ctypes.data, order.ctypes.data,
                                           starts.ctypes.data, o1.ctypes.data, oq1.ctypes.data, oo1.ctypes.data, o2.ctypes.data, oq2.ctypes.data,
                                           oo2.ctypes.data))

    med, times = _alternate({"demux_pairs": split}, reps)
    info = demux.last_info()
    k = min(N, 500)
    want = do.demux_pairs([m1[i].tobytes() for i in range(k)], [m2[i].tobytes() for i in range(k)], [ACGT[c].tobytes() for c in codes1],
                          [ACGT[c].tobytes() for c in codes2], table.tolist(), nsamples, max_shift=0, max_mismatches=1, min_margin=1)
    agree = bool(all((x[:len(getattr(want, f))] == getattr(want, f)).all() for f, x in (("barcode", barcode), ("bstart", bstart), ("mism", mism),
                                                                                         ("flags", flags), ("err", err), ("sample", sample))))
    tagged = (which1 >= 0) & (which2 >= 0)
    right = float((sample[tagged] == (which1[tagged] * nbc + which2[tagged])).mean())
    grouped = (_permuted(m1, o1, oo1, order, _cuts(sample, bstart[0::2], p)) and _permuted(m2, o2, oo2, order, _cuts(sample, bstart[1::2], p))
               and int(starts[-1]) == N)
    return {"workload": f"{N} pairs of 2 x ({p} + {m}) bp with qualities, {nbc} x {nbc} dual barcodes of {p} bytes, {nsamples} samples by table",
            "settings": {"max_shift": 0, "max_mismatches": 1, "min_margin": 1, "clip": 1}, "seconds": med, "seconds_all": times,
            "pairs_per_s": N / med["demux_pairs"], "info": info, "host_link_bytes_in": 4 * N * L + 32 * (N + 1) + 4 * nsamples,
            "tagged_pairs_in_their_sample": right, "grouped_batch_is_the_input_permuted": grouped, "agrees_with_oracle": agree, "oracle_pairs": k}


def fold_kernel_trace(trace_csv, into):
    """The demultiplexer's dispatches of a rocprofv3 kernel_trace.csv, grouped into calls, into the benchmark's JSON: per call kind
    the median time of each kernel (summed over the call's dispatches of it).  A call runs from its first match_kernel to as many
    gather_kernels as it had match_kernels (one: polyhip_demux_reads, whose two settings alternate as in bench_reads; two:
    polyhip_demux_pairs); what is dispatched outside a call (the trimmer's kernels, the genome) is left out."""
    with open(into) as f:
        out = json.load(f)
    calls, open_call = [], None
    with open(trace_csv, newline="") as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"])):
            name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if name is None:
                continue
            if name == "match_kernel" and (open_call is None or "assign_kernel" in open_call):
                open_call = {}
                calls.append(open_call)
            if open_call is None:
                continue
            open_call[name] = open_call.get(name, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            open_call["n_" + name] = open_call.get("n_" + name, 0) + 1
            if open_call.get("n_gather_kernel", 0) == open_call["n_match_kernel"]:
                open_call = None
    reads = [c for c in calls if c["n_match_kernel"] == 1]
    kinds = {"demux_reads_shift0": reads[0::2], "demux_reads_shift3": reads[1::2], "demux_pairs": [c for c in calls if c["n_match_kernel"] == 2]}
    table = {}
    for kind, cs in kinds.items():
        if cs:
            table[kind] = {"calls": len(cs), "median_us": {k: float(np.median([c.get(k, 0.0) for c in cs])) for k in KERNELS}}
            table[kind]["median_us"]["all_kernels"] = float(np.median([sum(c.get(k, 0.0) for k in KERNELS) for c in cs]))
    trace = {"source": "rocprofv3 --kernel-trace --stats, the script in a run of its own (--reps 2)", "per_call": table}
    for kind, key in (("demux_reads_shift0", "reads"), ("demux_reads_shift3", "reads"), ("demux_pairs", "pairs")):
        if kind in table and key in out:
            wall = out[key]["seconds"][kind] * 1e6
            table[kind]["kernels_share_of_the_call"] = table[kind]["median_us"]["all_kernels"] / wall
    out["kernel_trace"] = trace
    with open(into, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(trace))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("reads", "pairs"), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 kernel_trace.csv of a traced run of this script")
    ap.add_argument("--into", default=None, help="with --kernel-trace: the JSON of an untraced run to fold the kernel times into")
    args = ap.parse_args()
    if args.kernel_trace:
        fold_kernel_trace(args.kernel_trace, args.into)
        return
    import torch
    assert torch.cuda.is_available(), "bench_demux.py measures on the GPU; there is no CPU path"
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    if args.only != "pairs":
        out["reads"] = bench_reads(args.reads, args.reps)
    if args.only != "reads":
        out["pairs"] = bench_pairs(args.pairs, args.genome, args.reps)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    assert all(out.get("reads", {}).get("agrees_with_oracle", {}).values()), "polyhip_demux_reads differs from the oracle"
    assert out.get("pairs", {}).get("agrees_with_oracle", True), "polyhip_demux_pairs differs from the oracle"


if __name__ == "__main__":
    main()
