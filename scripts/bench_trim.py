"""The read trimmer on one MI355X: polyhip_trim_reads beside polyhip_fastq_pack_qual, and polyhip_trim_pairs, in one run.

    python scripts/bench_trim.py [--reads 1000000] [--pairs 500000] [--genome 5000000] [--reps 5] [--only reads|pairs]
                                 [--out profiles/trim_bench.json]
    python scripts/bench_trim.py --kernel-trace KERNEL_TRACE.csv --into profiles/trim_bench.json      (no GPU needed)

- reads: --reads reads of 150 bp with qualities (Q 2..19 with probability 0.1, else 20..41: a tenth of the bases below 20); a
  third of the reads end in 5..60 bytes of adapter (the 33-byte adapter, then noise); parameters min_qual_3p = min_qual_5p =
  20, one adapter, adapter_err_pct 10, min_overlap 3, min_len 20.  polyhip_fastq_pack_qual on the FASTQ image of these reads
  and polyhip_trim_reads on the packed batch alternate --reps times after a warm-up round, through the host-pointer calls: a
  host clock around each call, which includes the copies in, the device allocations and the copies back; medians;
- pairs: scripts/bench_map_pairs.py's pairs (2 x 150 bp, 5 % substitutions, 1 % indels, every second pair flipped) from
  fragments of 120 +- 40 bp (cut to 40 .. 300) instead of 350 +- 50: past the fragment's end a mate runs into its adapter and
  then into noise.  polyhip_trim_pairs with both adapters known (the adapter search finds the short inserts, step P the few
  it leaves), and with no adapter (step P alone), pair_min_overlap 20, pair_err_pct 10, alternate in the same way;
- checks: the first 1,000 reads and the first 200 pairs against tests/trim_oracle.py;
- bytes: what crosses the host link per call, and the device floor of a call: one read of the sequence and quality bytes plus
  one write of the kept ones;
- the kernels' own time is not taken here: run the script under a kernel trace in a run of its own (rocprofv3 --kernel-trace
  --stats, csv output) and fold the trace's kernel_trace.csv into the JSON with the second form above, which also sets the
  reads call's kernels against the floor at 8 TB/s.
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
ADAPTER2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"
HBM_BYTES_PER_S = 8e12
KERNELS = ("decide_kernel", "pair_kernel", "finish_kernel", "gather_kernel", "scan_apply_kernel", "scan_reduce_kernel")


def _alternate(calls, reps):
    times = {k: [] for k in calls}
    for rep in range(reps + 1):                            # round 0 warms up; the calls alternate; every call ends synchronised
        for name, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                times[name].append(time.perf_counter() - t0)
    return {k: float(np.median(v)) for k, v in times.items()}, times


def _quals(rng, shape):
    return (np.where(rng.random(shape) < 0.1, rng.integers(2, 20, shape), rng.integers(20, 42, shape)) + 33).astype(np.uint8)


def _adapter_tails(rng, reads, keep, adapter):
    """row i keeps its first keep[i] bytes; behind them come the adapter and then noise"""
    n, m = reads.shape
    ad = np.frombuffer(adapter, np.uint8)
    rel = np.arange(m)[None, :] - np.asarray(keep)[:, None]
    noise = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n, m))
    tail = np.where(rel < len(ad), ad[np.clip(rel, 0, len(ad) - 1)], noise)
    return np.where(rel >= 0, tail, reads)


def _params(**kw):
    from poly_amd import trim
    return trim.TrimParams(**kw)._c()


def _oracle_rows(reads, quals, k):
    return [reads[i].tobytes() for i in range(k)], [quals[i].tobytes() for i in range(k)]


def bench_reads(N, reps):
    from poly_amd import _lib, trim
    import trim_oracle as to
    rng = np.random.default_rng(31)
    m = 150
    reads = rng.choice(np.frombuffer(b"ACGT", np.uint8), (N, m))
    with_ad = np.nonzero(rng.random(N) < 1 / 3)[0]
    reads[with_ad] = _adapter_tails(rng, reads[with_ad], m - rng.integers(5, 61, len(with_ad)), ADAPTER)
    quals = _quals(rng, (N, m))
    head, plus, nl = (np.broadcast_to(np.frombuffer(x, np.uint8), (N, len(x))) for x in (b"@r x=1\n", b"\n+\n", b"\n"))
    img = np.ascontiguousarray(np.concatenate([head, reads, plus, quals, nl], axis=1)).reshape(-1)
    nb = len(img)
    most = nb // 7 + 1
    seqs, q = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)
    offs, qoffs = np.zeros(most + 2, np.uint64), np.zeros(most + 2, np.uint64)
    res = np.zeros(6, np.uint64)
    lib = _lib.lib()
    settings = dict(min_qual_3p=20, min_qual_5p=20, adapter_err_pct=10, min_overlap=3, min_len=20)
    p = _params(**settings)
    ad = np.frombuffer(ADAPTER, np.uint8).copy()
    adoff = np.array([0, len(ADAPTER)], np.uint32)
    start, end, flags, err = (np.zeros(N, np.uint32) for _ in range(4))
    out, outq, ooff = np.zeros(N * m, np.uint8), np.zeros(N * m, np.uint8), np.zeros(N + 1, np.uint64)

    def pack():
        _lib.check(lib.polyhip_fastq_pack_qual(img.ctypes.data, nb, seqs.ctypes.data, offs.ctypes.data, q.ctypes.data, qoffs.ctypes.data, None,
                                               most, res.ctypes.data))

    def cut():
        _lib.check(lib.polyhip_trim_reads(C.byref(p), ad.ctypes.data, adoff.ctypes.data, 1, seqs.ctypes.data, offs.ctypes.data, q.ctypes.data,
                                          qoffs.ctypes.data, N, start.ctypes.data, end.ctypes.data, flags.ctypes.data, err.ctypes.data,
                                          out.ctypes.data, outq.ctypes.data, ooff.ctypes.data))

    med, times = _alternate({"fastq_pack_qual": pack, "trim_reads": cut}, reps)
    info = trim.last_info()
    k = min(N, 1000)
    want = to.trim_reads(*_oracle_rows(reads, quals, k), [ADAPTER], **settings)
    kept = int(want.offsets[k])
    agree = bool(int(res[0]) == N and (start[:k] == want.start).all() and (end[:k] == want.end).all() and (flags[:k] == want.flags).all() and
                 (err[:k] == want.err).all() and (ooff[:k + 1] == want.offsets).all() and out[:kept].tobytes() == want.seqs.tobytes() and
                 outq[:kept].tobytes() == want.quals.tobytes())
    link_in, link_out = 2 * N * m + 16 * (N + 1), 2 * info["bytes_out"] + 8 * (N + 1) + 16 * N
    floor = 2 * info["bytes_in"] + 2 * info["bytes_out"]
    return {"workload": f"{N} reads x {m} bp with qualities, a tenth of the bases below Q 20, {len(with_ad)} reads ending in 5..60 adapter bytes",
            "settings": settings, "adapters": 1, "seconds": med, "seconds_all": times, "trim_over_pack_qual": med["trim_reads"] / med["fastq_pack_qual"],
            "reads_per_s": N / med["trim_reads"], "info": info, "fastq_image_bytes": nb, "host_link_bytes": {"in": link_in, "out": link_out},
            "host_link_GBps": (link_in + link_out) / med["trim_reads"] / 1e9, "device_floor_bytes": floor,
            "device_floor_us_at_8TBps": floor / HBM_BYTES_PER_S * 1e6, "agrees_with_oracle": agree, "oracle_reads": k}


def bench_pairs(N, n, reps):
    import torch
    from bench_map_pairs import make_pairs
    from poly_amd import _lib, mash, trim
    import trim_oracle as to
    rng = np.random.default_rng(37)
    m = 150
    g_t = torch.empty(n, dtype=torch.uint8, device=torch.device("cuda:0"))
    mash.synth_dna_dev(0x5EED + n, g_t)
    g = g_t.cpu().numpy()
    del g_t
    m1, m2, frag_start, frag_end, flipped = make_pairs(rng, g, N, m, mean=120, sd=40, lo=40, hi=300)
    insert = frag_end - frag_start
    keep = np.minimum(insert, m)                           # past the fragment's end: the adapter, then noise
    m1, m2 = np.ascontiguousarray(_adapter_tails(rng, m1, keep, ADAPTER)), np.ascontiguousarray(_adapter_tails(rng, m2, keep, ADAPTER2))
    q1, q2 = _quals(rng, (N, m)), _quals(rng, (N, m))
    off = np.arange(0, N * m + 1, m, dtype=np.uint64)
    lib = _lib.lib()
    settings = dict(min_qual_3p=20, adapter_err_pct=10, min_overlap=3, min_len=20, pair_min_overlap=20, pair_err_pct=10)
    p = _params(**settings)
    ad = np.frombuffer(ADAPTER + ADAPTER2, np.uint8).copy()
    adoff = np.array([0, len(ADAPTER), len(ADAPTER) + len(ADAPTER2)], np.uint32)
    start, end, flags, err = (np.zeros(2 * N, np.uint32) for _ in range(4))
    o1, oq1, oo1 = np.zeros(N * m, np.uint8), np.zeros(N * m, np.uint8), np.zeros(N + 1, np.uint64)
    o2, oq2, oo2 = np.zeros(N * m, np.uint8), np.zeros(N * m, np.uint8), np.zeros(N + 1, np.uint64)

    def cut(nad):
        _lib.check(lib.polyhip_trim_pairs(C.byref(p), ad.ctypes.data, adoff.ctypes.data, nad, m1.ctypes.data, off.ctypes.data, q1.ctypes.data,
                                          off.ctypes.data, m2.ctypes.data, off.ctypes.data, q2.ctypes.data, off.ctypes.data, N,
                                          start.ctypes.data, end.ctypes.data, flags.ctypes.data, err.ctypes.data, o1.ctypes.data, oq1.ctypes.data,
                                          oo1.ctypes.data, o2.ctypes.data, oq2.ctypes.data, oo2.ctypes.data))

    med, times = _alternate({"trim_pairs_adapters_and_overlap": lambda: cut(2), "trim_pairs_overlap_only": lambda: cut(0)}, reps)
    k = min(N, 200)
    (r1, qq1), (r2, qq2) = _oracle_rows(m1, q1, k), _oracle_rows(m2, q2, k)
    infos, agree, exact = {}, {}, {}
    for name, nad in (("trim_pairs_adapters_and_overlap", 2), ("trim_pairs_overlap_only", 0)):
        cut(nad)
        infos[name] = trim.last_info()
        want = to.trim_pairs(r1, r2, qq1, qq2, [ADAPTER, ADAPTER2][:nad], **settings)
        agree[name] = bool((start[:2 * k] == want.start).all() and (end[:2 * k] == want.end).all() and (flags[:2 * k] == want.flags).all() and
                           (oo1[:k + 1] == want.offsets[0]).all() and (oo2[:k + 1] == want.offsets[1]).all())
        short = insert < m - 2                              # a mate with indels reaches the fragment's end a few bytes off
        near = (np.abs(end[0::2].astype(np.int64) - insert) <= 3) & (np.abs(end[1::2].astype(np.int64) - insert) <= 3)
        exact[name] = float(near[short].mean())
    link_in = 4 * N * m + 8 * (N + 1)
    floor = {k_: 2 * v["bytes_in"] + 2 * v["bytes_out"] for k_, v in infos.items()}
    return {"workload": f"{N} pairs of 2 x {m} bp, fragments of 120 +- 40 bp (40 .. 300), {int((insert < m).sum())} shorter than the reads",
            "settings": settings, "seconds": med, "seconds_all": times, "pairs_per_s": {k_: N / v for k_, v in med.items()}, "info": infos,
            "host_link_bytes_in": link_in, "host_link_bytes_out": {k_: 2 * v["bytes_out"] + 16 * (N + 1) + 32 * N for k_, v in infos.items()},
            "device_floor_bytes": floor, "device_floor_us_at_8TBps": {k_: v / HBM_BYTES_PER_S * 1e6 for k_, v in floor.items()},
            "short_inserts_cut_within_3_bytes": exact, "agrees_with_oracle": agree, "oracle_pairs": k}


def fold_kernel_trace(trace_csv, into):
    """The trim kernels' dispatches of a rocprofv3 kernel_trace.csv, grouped into calls, into the benchmark's JSON: per call
    kind the median time of each kernel (summed over the call's dispatches of it), and the reads call's against its floor.
    A call starts at a decide_kernel that follows a gather_kernel; one decide_kernel means polyhip_trim_reads, two
    polyhip_trim_pairs, whose two settings alternate as in bench_pairs."""
    with open(into) as f:
        out = json.load(f)
    calls = []
    with open(trace_csv, newline="") as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"])):
            name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if name is None or "fq::" in r["Kernel_Name"] or (name.startswith("scan") and "unsigned long>" not in r["Kernel_Name"]):
                continue
            if name == "decide_kernel" and (not calls or "gather_kernel" in calls[-1]):
                calls.append({})
            if calls:
                calls[-1][name] = calls[-1].get(name, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                calls[-1]["n_" + name] = calls[-1].get("n_" + name, 0) + 1
    kinds = {"trim_reads": [c for c in calls if c["n_decide_kernel"] == 1]}
    pairs = [c for c in calls if c["n_decide_kernel"] == 2]
    kinds["trim_pairs_adapters_and_overlap"], kinds["trim_pairs_overlap_only"] = pairs[0::2], pairs[1::2]
    table = {}
    for kind, cs in kinds.items():
        if cs:
            table[kind] = {"calls": len(cs), "median_us": {k: float(np.median([c.get(k, 0.0) for c in cs])) for k in KERNELS}}
            table[kind]["median_us"]["all_kernels"] = float(np.median([sum(c.get(k, 0.0) for k in KERNELS) for c in cs]))
    trace = {"source": "rocprofv3 --kernel-trace --stats, the script in a run of its own (--reps 2)", "per_call": table}
    if "reads" in out and "trim_reads" in table:
        floor = out["reads"]["device_floor_us_at_8TBps"]
        us = table["trim_reads"]["median_us"]
        trace["reads_call_over_floor"] = {"floor_us": floor, "decide_kernel": us["decide_kernel"] / floor, "all_kernels": us["all_kernels"] / floor}
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
    assert torch.cuda.is_available(), "bench_trim.py measures on the GPU; there is no CPU path"
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    if args.only != "pairs":
        out["reads"] = bench_reads(args.reads, args.reps)
    if args.only != "reads":
        out["pairs"] = bench_pairs(args.pairs, args.genome, args.reps)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    assert out.get("reads", {}).get("agrees_with_oracle", True), "polyhip_trim_reads differs from the oracle"
    assert all(out.get("pairs", {}).get("agrees_with_oracle", {}).values()), "polyhip_trim_pairs differs from the oracle"


if __name__ == "__main__":
    main()
