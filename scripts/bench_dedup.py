"""polyhip_mark_duplicates and polyhip_coord_order on one MI355X beside the calls whose output they read, through the
host-pointer calls, in one run.

    python scripts/bench_dedup.py [--genome 5000000] [--reads 1000000] [--pairs 500000] [--reps 5] [--out profiles/dedup_bench.json]

- workloads: scripts/bench_map_affine.py's reads (150 bp sampled from a synthetic genome with 5 % substitutions and 1 % indels,
  every second one reverse-complemented, gaps (-5, -2)) and scripts/bench_map_pairs.py's pairs (2 x 150 bp, inserts 200..500),
  with a fifth of the reads (pairs) overwritten by exact copies of other reads (pairs), errors included, so that they land on
  their originals' ends; 150 quality bytes per read, Phred 2..40;
- protocol: each batch is mapped once and its records made once; then polyhip_mark_duplicates with the weights computed from
  the qualities (weight_mode 1, min_weight_qual 15), the same call with no weights at all (weight_mode 0), polyhip_coord_order,
  polyhip_aln_records and the mapping call alternate --reps times after one warm-up round; a host clock around each call, which
  ends in a stream synchronise and includes the copies in and out; medians are reported;
- key_passes: the 8-bit radix passes the call's sorts take on this batch, from the ranges of its sort words (restated here from
  the header's definition of the keys); sorted_keys = entries x passes of the end sort + pairs x passes of the pair sort;
  keys_per_s_of_the_call divides that by the WHOLE call's time, copies included, so it is a lower bound of the sort's own rate;
- the kernels' own time is not taken here: run the script under a kernel trace in a run of its own;
- check: dup, rep, weight, err and the info counters of the timed calls against tests/dedup_oracle.py on the whole batch (the
  weights it is handed are numpy's sums of the qualities), and the order against numpy's stable lexsort.
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


def _bits(lo, hi):
    return 0 if hi <= lo else int(hi - lo).bit_length()


def _passes(words):
    """8-bit passes of one sort: a word whose values are all the same costs none"""
    return sum((_bits(int(w.min()), int(w.max())) + 7) // 8 for w in words if len(w))


def _top(span, outsiders):
    """passes of the most significant word: the elements that take no part sort one past the largest key of the others"""
    top = span + 1 if outsiders else span
    return (top.bit_length() + 7) // 8


def key_passes(flags, err, w, ref_start, ref_end, read_start, read_end, read_len, paired):
    cand = ((flags & 1) == 1) & (err == 0)
    s = (flags >> 1 & 1).astype(np.int64)
    u = np.where(s == 1, ref_end.astype(np.int64) - 1 + read_len.astype(np.int64) - read_end, ref_start.astype(np.int64) - read_start)
    us = (u + (1 << 32)) << 1 | s
    pair = cand & cand[np.arange(len(cand)) ^ 1] if paired else np.zeros(len(cand), bool)
    A = ((cand & ~pair).astype(np.int64) << 32) | (0xFFFFFFFF - w.astype(np.int64))
    ends = _passes([A[cand], us[cand]]) + _top(0, int((~cand).sum()))          # no contigs here: the last word is one value
    pairs = 0
    if paired:
        p = pair[0::2]
        W = 0x1FFFFFFFF - (w[0::2].astype(np.int64) + w[1::2].astype(np.int64))
        odd = us[1::2] < us[0::2]
        lo, hi = np.where(odd, us[1::2], us[0::2]), np.where(odd, us[0::2], us[1::2])
        pairs = _passes([W[p], hi[p], lo[p]]) + _top(0, int((~p).sum()))
    return ends, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, default=500_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from bench_map import make_reads
    from bench_map_pairs import make_pairs
    from poly_amd import _lib, align, alphabet, bwt, dedup, mapper, mash, matrix, sam
    import dedup_oracle as do
    assert torch.cuda.is_available(), "bench_dedup.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(29)
    n, m = args.genome, 150
    P, PP = mapper.MapParams(), mapper.PairParams(200, 500)
    ab = alphabet.NewAlphabet(list("-ACGT"))
    sc = align.NewScoring(matrix.NewSubstitutionMatrix(ab, ab, matrix.NUC_4), -2)
    g_t = torch.empty(n, dtype=torch.uint8, device=dev)
    mash.synth_dna_dev(0x5EED + n, g_t)
    idx = bwt.new_dev(g_t)
    text = np.ascontiguousarray(g_t.cpu().numpy())
    lib, p, pp = _lib.lib(), P._c(), PP._c()

    def run(name, R, paired, map_call, out):
        """R entries; out: the arrays the mapping call filled"""
        flags, ref_start, ref_end, read_start, read_end = (out[k] for k in ("flags", "ref_start", "ref_end", "read_start", "read_end"))
        read_len = np.full(R, m, np.uint32)
        qual = rng.integers(33 + 2, 33 + 41, R * m).astype(np.uint8)
        qoff = np.arange(0, R * m + 1, m, dtype=np.uint64)
        rp = sam._CParams(0, int(paired))
        coff, moff = np.zeros(R + 1, np.uint64), np.zeros(R + 1, np.uint64)
        nm, sf, rerr, mapq = np.zeros(R, np.uint32), np.zeros(R, np.uint32), np.zeros(R, np.uint32), np.zeros(R, np.uint8)

        def rec_call(cigar, ccap, md, mcap):
            return lib.polyhip_aln_records(C.byref(rp), R, flags.ctypes.data, out["score"].ctypes.data, out["second"].ctypes.data,
                                           read_start.ctypes.data, read_end.ctypes.data, read_len.ctypes.data, out["alnA"].ctypes.data,
                                           out["alnB"].ctypes.data, out["aoff"].ctypes.data, coff.ctypes.data,
                                           cigar.ctypes.data if cigar is not None else None, ccap, moff.ctypes.data,
                                           md.ctypes.data if md is not None else None, mcap, nm.ctypes.data, mapq.ctypes.data, sf.ctypes.data,
                                           rerr.ctypes.data)

        assert rec_call(None, 0, None, 0) in (_lib.OK, _lib.ERR_INVALID)          # the sizes
        nc, nb = int(coff[R]), int(moff[R])
        cigar, md = np.zeros(max(nc, 1), np.uint32), np.zeros(max(nb, 1), np.uint8)
        res = {k: (np.zeros(R, np.uint8), np.zeros(R, np.uint32), np.zeros(R, np.uint32), np.zeros(R, np.uint32)) for k in ("qual", "plain")}
        order = np.zeros(R, np.uint32)

        def mark_call(k):
            dp = dedup._CParams(int(paired), 1 if k == "qual" else 0, 15, 33)
            d, r, w, e = res[k]
            return lambda: lib.polyhip_mark_duplicates(C.byref(dp), R, flags.ctypes.data, None, ref_start.ctypes.data, ref_end.ctypes.data,
                                                       read_start.ctypes.data, read_end.ctypes.data, read_len.ctypes.data, None,
                                                       qual.ctypes.data if k == "qual" else None, qoff.ctypes.data if k == "qual" else None,
                                                       w.ctypes.data, d.ctypes.data, r.ctypes.data, e.ctypes.data)

        calls = {"mark_duplicates": mark_call("qual"), "mark_duplicates_no_weights": mark_call("plain"),
                 "coord_order": lambda: lib.polyhip_coord_order(R, int(paired), sf.ctypes.data, None, ref_start.ctypes.data, order.ctypes.data),
                 "aln_records": lambda: rec_call(cigar, nc, md, nb), "mapping": map_call}
        times, infos = {k: [] for k in calls}, {}
        for rep in range(args.reps + 1):                       # round 0 warms up; the calls alternate
            for k, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _lib.check(fn())
                dt = time.perf_counter() - t0
                if rep:
                    times[k].append(dt)
                if k.startswith("mark"):
                    infos[k] = dedup.last_info()
        med = {k: float(np.median(v)) for k, v in times.items()}
        # ---- the whole batch against the oracle
        same = True
        q = qual.reshape(R, m).astype(np.int64) - 33             # every string is in range: the weights by numpy, the rest by the oracle
        by_numpy = np.where(q >= 15, q, 0).sum(axis=1).astype(np.uint32)
        for k in ("qual", "plain"):
            want = do.mark(flags, ref_start, ref_end, read_start, read_end, read_len, paired=paired, weight=by_numpy if k == "qual" else None)
            d, r, w, e = res[k]
            same = same and all((x == y).all() for x, y in zip((d, r, w, e), (want.dup, want.rep, want.weight, want.err)))
            same = same and infos["mark_duplicates" if k == "qual" else "mark_duplicates_no_weights"] == want.info
        live = (sf & 4) == 0
        at = np.arange(R)
        if paired:
            at = np.where(~live & live[at ^ 1], at ^ 1, at)
        placed = live[at]
        want_order = np.lexsort((np.arange(R), np.where(placed, ref_start[at], 0), ~placed))
        same = bool(same and (order == want_order).all())
        ends, pairs = key_passes(flags, res["qual"][3], res["qual"][2], ref_start, ref_end, read_start, read_end, read_len, paired)
        keys = R * ends + (R // 2) * pairs
        return {"entries": R, "paired": paired, "seconds": med, "seconds_all": times, "info": infos["mark_duplicates"],
                "info_no_weights": infos["mark_duplicates_no_weights"], "mark_over_records": med["mark_duplicates"] / med["aln_records"],
                "mark_over_mapping": med["mark_duplicates"] / med["mapping"], "order_over_records": med["coord_order"] / med["aln_records"],
                "order_over_mapping": med["coord_order"] / med["mapping"], "key_passes_end_sort": ends, "key_passes_pair_sort": pairs,
                "sorted_keys": keys, "keys_per_s_of_the_call": keys / med["mark_duplicates"],
                "bytes_in": R * (6 * 4 + m + 8) + 8, "bytes_out": R * (1 + 3 * 4), "equals_oracle": same}

    def outputs(R, cap):
        o = {k: np.zeros(R, np.int64) for k in ("score", "second")}
        o.update({k: np.zeros(R, np.uint32) for k in ("flags", "votes", "ref_start", "ref_end", "read_start", "read_end", "err")})
        o.update(alnA=np.zeros(cap, np.uint8), alnB=np.zeros(cap, np.uint8), aoff=np.zeros(R + 1, np.uint64))
        return o

    u32 = ("flags", "votes", "ref_start", "ref_end", "read_start", "read_end", "err")
    # ---- single reads
    N = args.reads
    reads = make_reads(rng, text, N, m)
    copies = rng.choice(N, N // 5, replace=False)
    keep = np.setdiff1d(np.arange(N), copies)
    reads[copies] = reads[rng.choice(keep, len(copies))]
    buf, offs, cap = reads.reshape(-1), np.arange(0, N * m + 1, m, dtype=np.uint64), 2 * N * m
    o1 = outputs(N, cap)

    def map_reads():
        return lib.polyhip_map_reads_affine(idx.handle(), sc.handle(), C.byref(p), -5, -2, buf.ctypes.data, offs.ctypes.data, N, m, 0,
                                            o1["score"].ctypes.data, o1["second"].ctypes.data, *[o1[k].ctypes.data for k in u32],
                                            o1["alnA"].ctypes.data, o1["alnB"].ctypes.data, o1["aoff"].ctypes.data, cap)

    _lib.check(map_reads())
    single = run("reads", N, False, map_reads, o1)
    # ---- pairs
    M = args.pairs
    m1, m2, _, _, _ = make_pairs(rng, text, M, m)
    copies = rng.choice(M, M // 5, replace=False)
    keep = np.setdiff1d(np.arange(M), copies)
    src = rng.choice(keep, len(copies))
    m1[copies], m2[copies] = m1[src], m2[src]
    off1, cap2 = np.arange(0, M * m + 1, m, dtype=np.uint64), 4 * M * m
    o2 = outputs(2 * M, cap2)
    tlen = np.zeros(M, np.int64)

    def map_pairs():
        return lib.polyhip_map_pairs(idx.handle(), sc.handle(), C.byref(p), C.byref(pp), -5, -2, m1.ctypes.data, off1.ctypes.data,
                                     m2.ctypes.data, off1.ctypes.data, M, m, 0, o2["score"].ctypes.data, o2["second"].ctypes.data,
                                     *[o2[k].ctypes.data for k in u32], tlen.ctypes.data, o2["alnA"].ctypes.data, o2["alnB"].ctypes.data,
                                     o2["aoff"].ctypes.data, cap2)

    _lib.check(map_pairs())
    pairs = run("pairs", 2 * M, True, map_pairs, o2)

    yard = {}
    try:
        with open(os.path.join(ROOT, "profiles", "bwt_bench.json")) as f:
            big = json.load(f)["genomes"][-1]
        # the file holds no rate of the sort alone: the whole build of polyhip_bwt_create, whose doubling rounds each end in
        # one radix_sort of n keys among other kernels
        yard = {"bwt_create_n": big["n"], "bwt_create_build_s": big["build_s"], "bwt_create_doubling_rounds": big["doubling_rounds"],
                "bwt_create_positions_per_s": big["n"] / big["build_s"]}
    except (OSError, KeyError, ValueError):
        pass
    out = {"device": torch.cuda.get_device_name(0), "genome": n, "read_len": m, "reps": args.reps, "copies": 0.2, "reads": single,
           "pairs": pairs, "yardstick": yard}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    assert single["equals_oracle"] and pairs["equals_oracle"], "the marks or the order differ from the oracle's"


if __name__ == "__main__":
    main()
