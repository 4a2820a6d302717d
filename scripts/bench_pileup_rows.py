"""polyhip_pileup_rows on one MI355X beside polyhip_pileup_qual, in one run.

    python scripts/bench_pileup_rows.py [--genome 5000000] [--reads 1000000] [--reps 5] [--only-rows]
                                        [--out profiles/pileup_rows_bench.json]
    python scripts/bench_pileup_rows.py --summarise-db x_results.db > profiles/pileup_rows_kernel_stats.md  (no GPU)
    python scripts/bench_pileup_rows.py --merge-trace profiles/pileup_rows_kernel_stats.md --out profiles/pileup_rows_bench.json

- workload: scripts/bench_base_qual.py's pileup half, built the same way -- a synthetic genome, reads of 150 bp with 5 %
  substitutions and 1 % indels mapped once by polyhip_map_reads_affine, the records made once, 150 quality bytes per read
  with about a tenth of the bases below 20 --, then polyhip_pileup_qual at min_base_qual 0 and polyhip_pileup_rows (with
  the qualities, min_mapq 20, entry order, rows for the covered positions) over the whole text alternate --reps times after
  a warm-up round, through the host-pointer calls; a host clock around each call, which includes the uploads, the device
  allocations and the copies back; medians.  The text buffer has the exact size, asked for once before the clock starts;
- checks: the depth column of every row equals polyhip_pileup's depth at min_mapq 20; a window of 2,000 positions, run as a
  region of its own, equals tests/pileup_rows_oracle.py byte for byte; the whole text parses with poly_amd.pileup_text;
- the kernels' own time is not taken here: run the script under a kernel trace in a run of its own (--only-rows --reps 1
  keeps the other call out of it), summarise its database with --summarise-db and hand the table back with --merge-trace,
  which adds the kernels' time per call and its share of the call to the JSON of the timing run.
Prints one JSON object (and writes it to --out).  Nothing here has a speed threshold.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

ROWS_KERNELS = ("order_kernel", "walk_kernel", "count_kernel", "item_kernel", "gather_kernel", "rowsize_kernel",
                "header_kernel", "token_kernel", "radix_hist_kernel", "radix_scatter_kernel")      # and the scan_* kernels


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


def run(dev, n, N, reps, only_rows):
    import torch
    from bench_map import make_reads
    from poly_amd import _lib, align, alphabet, bwt, mapper, mash, matrix, pileup, pileup_text, sam
    import pileup_rows_oracle as ro
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
    qual = np.where(rng.random(N * m) < 0.1, rng.integers(2, 20, N * m), rng.integers(20, 42, N * m)).astype(np.uint8) + np.uint8(33)
    qoff = offs
    settings = dict(min_mapq=20, min_depth=4, min_alt_count=2, min_alt_permille=500)
    name = np.frombuffer(b"genome", np.uint8)

    qerr, nsites = np.zeros(N, np.uint32), C.c_uint64(0)
    qcounts, qsum, qcons = np.zeros((pileup.CHANNELS, n), np.uint32), np.zeros((pileup.QSUM_PLANES, n), np.uint32), np.zeros(n, np.uint8)
    scap = 1 << 20
    qsites = np.zeros(scap, pileup.SITE_DTYPE)

    def with_qual():
        qp = pileup._CQualParams(pileup._CParams(0, n, *[settings[k] for k in ("min_mapq", "min_depth", "min_alt_count", "min_alt_permille")]), 0, 33)
        _lib.check(lib.polyhip_pileup_qual(C.byref(qp), N, flags.ctypes.data, mapq.ctypes.data, ref_start.ctypes.data, ref_end.ctypes.data,
                                           read_start.ctypes.data, alnA.ctypes.data, alnB.ctypes.data, aoff.ctypes.data, qual.ctypes.data,
                                           qoff.ctypes.data, text.ctypes.data, n, qcounts.ctypes.data, qsum.ctypes.data, qcons.ctypes.data,
                                           C.byref(nsites), qsites.ctypes.data, scap, qerr.ctypes.data))

    rerr2, ntext = np.zeros(N, np.uint32), C.c_uint64(0)

    def rows_call(lo, hi, out, out_cap, row_off):
        cp = pileup._CRowsParams(lo, hi, 0, settings["min_mapq"], 33, 0, 0)
        return lib.polyhip_pileup_rows(C.byref(cp), N, flags.ctypes.data, mapq.ctypes.data, ref_start.ctypes.data, ref_end.ctypes.data,
                                       read_start.ctypes.data, alnA.ctypes.data, alnB.ctypes.data, aoff.ctypes.data, qual.ctypes.data,
                                       qoff.ctypes.data, text.ctypes.data, n, None, name.ctypes.data, len(name), C.byref(ntext),
                                       None if out is None else out.ctypes.data, out_cap, None if row_off is None else row_off.ctypes.data,
                                       rerr2.ctypes.data)

    assert rows_call(0, n, None, 0, None) in (_lib.OK, _lib.ERR_INVALID)          # the size
    nt = int(ntext.value)
    out, row_off = np.zeros(max(nt, 1), np.uint8), np.zeros(n + 1, np.uint64)
    calls = {"pileup_rows": lambda: _lib.check(rows_call(0, n, out, nt, row_off))}
    if not only_rows:
        calls = {"pileup_qual_0": with_qual, **calls}
    med, times = _alternate(calls, reps, torch.cuda.synchronize)
    info = pileup.last_rows_info()
    result = {"genome": n, "reads": N, "read_len": m, "settings": dict(min_mapq=settings["min_mapq"], all_positions=0, order=None, qualities=True),
              "seconds": med, "seconds_all": times, "info": info, "text_bytes": nt, "tokens": info["tokens"],
              "sort_passes": (max(n - 1, 1).bit_length() + 7) // 8, "sort_key_bits": max(n - 1, 1).bit_length()}
    strings = int(aoff[N])
    bytes_in = 2 * strings + n + 8 * (N + 1) + N * (3 * 4 + 1) + N * m + 8 * (N + 1) + 4 * N
    result.update(bytes_in=bytes_in, bytes_out=nt + 8 * (n + 1) + 4 * N,
                  host_link_GBps=(bytes_in + nt + 8 * (n + 1) + 4 * N) / med["pileup_rows"] / 1e9)
    if only_rows:
        return result
    result["rows_over_pileup_qual"] = med["pileup_rows"] / med["pileup_qual_0"]
    # every row's depth column against the counts
    with_qual()
    depth = qcounts[0:6].sum(axis=0, dtype=np.uint64) + qcounts[8:14].sum(axis=0, dtype=np.uint64)
    lens = np.diff(row_off.astype(np.int64))
    result["rows_where_depth"] = bool(((lens > 0) == (depth > 0)).all()) and info["rows"] == int((depth > 0).sum())
    result["tokens_equal_depth_sum"] = info["tokens"] == int(depth.sum())
    sample = np.nonzero(depth)[0][:: max(1, n // 5000)]
    blob = out.tobytes()
    result["depth_column"] = all(int(blob[int(row_off[j]):int(row_off[j + 1])].split(b"\t")[3]) == int(depth[j]) for j in sample)
    head = blob[:int(row_off[min(n, 20000)])]
    parsed = pileup_text.parse(head)
    result["parses"] = len(parsed) == int((depth[:min(n, 20000)] > 0).sum()) and all(len(x.quality) == x.read_count for x in parsed)
    # a window, run as a region of its own, against the oracle on the entries that touch it
    lo, hi = n // 5, n // 5 + 2000
    near = np.nonzero(((flags & 1) == 1) & (ref_start <= hi) & (ref_end >= lo))[0]
    cols = np.diff(aoff.astype(np.int64))
    a_all, b_all, q_all = alnA.tobytes(), alnB.tobytes(), qual.tobytes()
    sub_off = np.zeros(len(near) + 1, np.uint64)
    sub_off[1:] = np.cumsum(cols[near])
    sub_q = np.arange(0, len(near) * m + 1, m, dtype=np.uint64)
    want = ro.pileup_rows(flags[near], mapq[near], ref_start[near], ref_end[near], read_start[near],
                          b"".join(a_all[int(aoff[i]):int(aoff[i + 1])] for i in near),
                          b"".join(b_all[int(aoff[i]):int(aoff[i + 1])] for i in near), sub_off,
                          b"".join(q_all[int(i) * m:(int(i) + 1) * m] for i in near), sub_q, text.tobytes(), b"genome", region=(lo, hi),
                          min_mapq=settings["min_mapq"])
    win = np.zeros(len(want.text) + 1, np.uint8)
    _lib.check(rows_call(lo, hi, win, len(win), None))
    result["spot_check"] = int(ntext.value) == len(want.text) and win[:len(want.text)].tobytes() == want.text and \
        blob[int(row_off[lo]):int(row_off[hi])] == want.text
    result["spot_entries"] = int(len(near))
    return result


def merge_trace(stats_path, out_path):
    """adds the kernels' time per polyhip_pileup_rows call, from the markdown table scripts/rocpd_summary.py wrote for a run of
    --only-rows, to the JSON of the timing run"""
    with open(out_path) as f:
        out = json.load(f)
    kernels, total_ms = {}, 0.0
    with open(stats_path) as f:
        for line in f:
            mt = re.match(r"\| `([^`]+)` \| (\d+) \| ([0-9.]+) \| ([0-9.]+) \|", line)
            base = mt.group(1).split("::")[-1].split("<")[0] if mt else ""
            if mt and (base in ROWS_KERNELS or base.startswith("scan_")):
                kernels[mt.group(1)] = {"calls": int(mt.group(2)), "total_ms": float(mt.group(3))}
                total_ms += float(mt.group(3))
    item = next((v["calls"] for k, v in kernels.items() if "item_kernel" in k), 0)
    assert item, "the table holds no item_kernel: it is not a trace of polyhip_pileup_rows"
    # an upper bound: the sort and scan kernels of the run's set-up (index build, mapping) carry the same names and are
    # counted in, and so is the size call, which runs everything but the two emit kernels
    per_call = total_ms / item
    out["rows"]["kernel_trace"] = {"source": os.path.basename(stats_path), "calls_traced": item, "kernels": kernels,
                                   "kernel_ms_per_call_upper_bound": per_call,
                                   "kernel_share_of_call": per_call / 1e3 / out["rows"]["seconds"]["pileup_rows"]}
    with open(out_path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["rows"]["kernel_trace"]))


def summarise_db(path, title):
    """the per-kernel table of a rocprofv3 kernel trace (rocpd format), kernels of anonymous namespaces under their own names"""
    import sqlite3
    cur = sqlite3.connect(path).cursor()
    print(f"# {title}\n\n| kernel | calls | total ms | mean ms | % |\n|---|---:|---:|---:|---:|")
    for name, calls, total, avg, pct in cur.execute("select name,total_calls,total_duration,average,percentage from top_kernels"):
        short = name.replace("(anonymous namespace)::", "").split("(")[0][:110]
        print(f"| `{short}` | {calls} | {total / 1e3:.3f} | {avg / 1e3:.4f} | {pct:.2f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-rows", action="store_true", help="polyhip_pileup_rows alone and no checks: for a kernel trace")
    ap.add_argument("--merge-trace", default=None, help="a table of scripts/rocpd_summary.py to add to --out; runs nothing")
    ap.add_argument("--summarise-db", default=None, help="a rocprofv3 results.db: prints its kernel table; runs nothing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise_db:
        return summarise_db(args.summarise_db, "polyhip_pileup_rows alone (--only-rows --reps 1), kernel trace of a run of its own")
    if args.merge_trace:
        return merge_trace(args.merge_trace, args.out)
    import torch
    assert torch.cuda.is_available(), "bench_pileup_rows.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "workloads_measured": 1,
           "rows": run(dev, args.genome, args.reads, args.reps, args.only_rows)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    r = out["rows"]
    assert all(r.get(k, True) for k in ("rows_where_depth", "tokens_equal_depth_sum", "depth_column", "parses", "spot_check")), "the rows differ"


if __name__ == "__main__":
    main()
