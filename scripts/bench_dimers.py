"""The primer-dimer screen on one MI355X: polyhip_primer_dimer_screen on a pool and polyhip_primer_dimer_matrix on a block of it.

    python scripts/bench_dimers.py [--pool 20000] [--block 4096] [--reps 5] [--out profiles/dimers_bench.json]
    python scripts/bench_dimers.py --kernel-trace KERNEL_TRACE.csv --into profiles/dimers_bench.json         (no GPU needed)
    python scripts/bench_dimers.py --counters COUNTER_COLLECTION.csv --into profiles/dimers_bench.json       (no GPU needed)

- the pool: --pool primers of 18..30 bytes cut at random places from the K4 workload's genome (poly_amd/workloads.py's synthetic
  DNA, seed 0xC5, 5 Mb), table at 37 degrees Celsius;
- screen: the pool against itself (pool mode), thresholds -6000 / -4000 cal/mol, --reps times after a warm-up, through the
  host-pointer call: a host clock around each call, which includes the copies in, the device allocation and the copies back;
- matrix: the first --block primers against themselves, both planes, the same way;
- rates: ordered pairs per second and shift evaluations per second (polyhip_primer_dimer_last_info's shifts: the sum of m + n - 1
  over the pairs), and the bytes that cross the host link;
- checks: the screen of the block against the numpy reduction of the matrix call's planes, 2,000 random cells of the matrix and
  the shift, pos and pairs of 200 rows against tests/dimers_oracle.py;
- the kernels' own time and their instruction counts are not taken here: run the script under a kernel trace (rocprofv3
  --kernel-trace --stats, csv output) and under a counter collection (rocprofv3 --pmc SQ_INSTS_VALU, csv output), each in a run
  of its own, and fold kernel_trace.csv / counter_collection.csv into the JSON with the second and third form above; the
  counter fold sets the count against the issue cost of the loop's instruction mix (LOOP_MIX below).
Prints one JSON object (and writes it to --out).  Nothing here has a speed threshold.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KERNELS = ("prepare_kernel", "pair_kernel", "detail_kernel")
ANY_T, END_T = -6000, -4000
SIMDS = 256 * 4                                                # 256 CUs x 4 SIMDs
NOMINAL_GHZ = 2.4                                              # the clock during the kernel is not measured here
# The VALU instructions of pair_kernel<screen>'s shift loop as hipcc compiles it for gfx950, counted in the assembly and priced
# with the issue rates of DESIGN.md section 2 (add / sub / and / or / xor / lshr: 2 cycles per wave64, everything else 4):
# (2-cycle, 4-cycle) instructions once per walked shift (the four masks, M & M >> 1, the 3' run) and per turn of the run loop
LOOP_MIX = {"per_walked_shift": (16, 12), "per_run_loop_turn": (11, 13)}


def make_pool(n, genome=5_000_000):
    from poly_amd import workloads
    g = workloads.synth_dna(0xC5, genome)
    rng = np.random.default_rng(2030)
    lens = rng.integers(18, 31, n)
    starts = rng.integers(0, genome - 30, n)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    buf = np.concatenate([g[s:s + l] for s, l in zip(starts, lens)])
    return np.ascontiguousarray(buf), offs


def _timed(fn, reps):
    fn()                                                       # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def bench(npool, nblock, reps):
    from poly_amd import dimers
    import dimers_oracle as do
    buf, offs = make_pool(npool)
    nblock = min(nblock, npool)
    boffs = offs[:nblock + 1]
    out = {}

    res = {}
    t, times = _timed(lambda: res.__setitem__("s", dimers.screen_packed(buf, offs, any_threshold=ANY_T, end_threshold=END_T)), reps)
    info = dimers.last_info()
    s = res["s"]
    out["screen"] = {"workload": f"{npool} primers of 18..30 bytes against themselves, thresholds {ANY_T} / {END_T} cal/mol at 37 C",
                     "seconds": t, "seconds_all": times, "info": info, "pairs_per_s": info["pairs"] / t,
                     "shift_evaluations_per_s": info["shifts"] / t,
                     "host_link_bytes": {"in": int(len(buf) + 8 * (npool + 1) + 64), "out": int(12 * 4 * npool)},
                     "rows_with_a_partner_at_the_any_threshold": int((s.any_count > 0).sum()),
                     "rows_with_a_partner_at_the_end_threshold": int((s.end_count > 0).sum())}

    t, times = _timed(lambda: res.__setitem__("m", dimers.matrix_packed(buf, boffs)), reps)
    info = dimers.last_info()
    m = res["m"]
    out["matrix"] = {"workload": f"the first {nblock} primers against themselves, both planes", "seconds": t, "seconds_all": times,
                     "info": info, "pairs_per_s": info["pairs"] / t, "shift_evaluations_per_s": info["shifts"] / t,
                     "host_link_bytes": {"in": int(boffs[-1] + 8 * (nblock + 1) + 64), "out": int(2 * 4 * nblock * nblock + 4 * nblock)}}

    # checks
    sb = dimers.screen_packed(buf, boffs, any_threshold=ANY_T, end_threshold=END_T)
    red = do.screen_from_matrix(m.dg_any, m.dg_end, m.errX, m.errY, ANY_T, END_T)
    prim = [buf[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nblock)]
    rng = np.random.default_rng(7)
    cells = rng.integers(0, nblock, (2000, 2))
    cells_ok = all((int(m.dg_any[i, j]), int(m.dg_end[i, j])) == (lambda p: (p.dg_any, p.dg_end))(do.pair(prim[i], prim[j])) for i, j in cells)
    rows_ok = True
    for i in range(min(200, nblock)):
        pa = do.pair(prim[i], prim[int(sb.any_partner[i])]) if sb.any_partner[i] != do.NONE else do.Pair()
        pe = do.pair(prim[i], prim[int(sb.end_partner[i])]) if sb.end_partner[i] != do.NONE else do.Pair()
        rows_ok &= (int(sb.any_shift[i]), int(sb.any_pos[i]), int(sb.any_pairs[i])) == (pa.any_shift, pa.any_pos, pa.any_pairs)
        rows_ok &= (int(sb.end_shift[i]), int(sb.end_pairs[i])) == (pe.end_shift, pe.end_pairs)
    out["checks"] = {"screen_equals_the_reduction_of_the_matrix": bool(all((getattr(sb, f) == v).all() for f, v in red.items())),
                     "matrix_cells_equal_the_oracle": bool(cells_ok), "cells": len(cells), "screen_rows_equal_the_oracle": bool(rows_ok),
                     "rows": min(200, nblock)}
    return out


def _load(into):
    with open(into) as f:
        return json.load(f)


def _store(into, out):
    with open(into, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


def fold_kernel_trace(trace_csv, into):
    """The unit's dispatches of a rocprofv3 kernel_trace.csv into the benchmark's JSON: per kernel the dispatches and the summed
    and median time; the screen's pair_kernel dispatches (the long ones: template argument true) against the screen call's wall
    time of the untraced run."""
    out = _load(into)
    per = {k: [] for k in KERNELS}
    screen_pair = []
    with open(trace_csv, newline="") as f:
        for r in csv.DictReader(f):
            name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if name is None or "polyhip" not in r["Kernel_Name"]:
                continue
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            per[name].append(us)
            if name == "pair_kernel" and ("<true>" in r["Kernel_Name"] or "ILb1E" in r["Kernel_Name"]):
                screen_pair.append(us)
    trace = {"source": "rocprofv3 --kernel-trace --stats, the script in a run of its own",
             "per_kernel_us": {k: {"dispatches": len(v), "sum": float(np.sum(v)), "median": float(np.median(v))} for k, v in per.items() if v}}
    if screen_pair and "screen" in out:
        big = float(np.median([u for u in screen_pair if u >= 0.5 * max(screen_pair)]))
        trace["screen_pair_kernel_us"] = big
        trace["screen_pair_kernel_share_of_the_call"] = big / (out["screen"]["seconds"] * 1e6)
        trace["screen_shift_evaluations_per_s_in_the_kernel"] = out["screen"]["info"]["shifts"] / (big / 1e6)
    out["kernel_trace"] = trace
    _store(into, out)
    print(json.dumps(trace))


def walked_shifts(npool):
    """what the screen's waves walk on the pool of this size: a wave of 64 consecutive y runs the shifts of its longest y, so a
    lane walks m + nmax - 1 shifts where polyhip_primer_dimer_last_info counts m + n - 1"""
    _, offs = make_pool(npool)
    lens = np.diff(offs.astype(np.int64))
    pad = np.zeros(-(-npool // 64) * 64, np.int64)
    pad[:npool] = lens
    nmax = np.repeat(pad.reshape(-1, 64).max(axis=1), 64)[:npool]
    return int(npool * lens.sum() + npool * nmax.sum() - npool * npool)


def fold_counters(counter_csv, into):
    """SQ_INSTS_VALU of a rocprofv3 counter_collection.csv: the VALU wave-instructions of the largest pair_kernel dispatch (the
    screen's) per shift evaluation, and with the traced kernel time the cycles a SIMD spends per VALU instruction at the nominal
    clock, set against what the loop's instruction mix costs to issue (LOOP_MIX; the number of run-loop turns per walked shift
    follows from the count): the share of the VALU issue ceiling."""
    out = _load(into)
    best = 0.0
    with open(counter_csv, newline="") as f:
        for r in csv.DictReader(f):
            if "pair_kernel" in r["Kernel_Name"] and r["Counter_Name"] == "SQ_INSTS_VALU":
                best = max(best, float(r["Counter_Value"]))
    info = out["screen"]["info"]
    walked = walked_shifts(info["primers"])
    per_walked = best * 64.0 / walked
    (a2, a4), (b2, b4) = LOOP_MIX["per_walked_shift"], LOOP_MIX["per_run_loop_turn"]
    turns = (per_walked - (a2 + a4)) / (b2 + b4)
    priced = (2 * a2 + 4 * a4 + turns * (2 * b2 + 4 * b4)) / per_walked
    c = {"source": "rocprofv3 --pmc SQ_INSTS_VALU, the script in a run of its own", "screen_pair_kernel_SQ_INSTS_VALU": best,
         "valu_instructions_per_shift_evaluation": best * 64.0 / info["shifts"], "shifts_walked_by_the_waves": walked,
         "valu_instructions_per_walked_shift": per_walked, "loop_mix_2_and_4_cycle": LOOP_MIX,
         "run_loop_turns_per_walked_shift_from_the_count": turns, "issue_cycles_per_instruction_by_the_mix": priced}
    us = out.get("kernel_trace", {}).get("screen_pair_kernel_us")
    if us:
        spent = us * 1e3 * NOMINAL_GHZ * SIMDS / best
        c["cycles_per_instruction_and_simd_at_the_nominal_clock"] = spent
        c["share_of_the_valu_issue_ceiling"] = priced / spent
        c["note"] = (f"{NOMINAL_GHZ} GHz is nominal: the clock during the kernel was not measured, a lower one raises the share; priced flat at 4 "
                     f"cycles as K3's row is, the share would be {4 / spent:.2f}, at 2 cycles {2 / spent:.2f}")
    out["counters"] = c
    _store(into, out)
    print(json.dumps(c))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool", type=int, default=20_000)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None, help="a rocprofv3 kernel_trace.csv of a traced run of this script")
    ap.add_argument("--counters", default=None, help="a rocprofv3 counter_collection.csv of a --pmc SQ_INSTS_VALU run of this script")
    ap.add_argument("--into", default=None, help="with --kernel-trace / --counters: the JSON of an untraced run to fold into")
    args = ap.parse_args()
    if args.kernel_trace:
        fold_kernel_trace(args.kernel_trace, args.into)
        return
    if args.counters:
        fold_counters(args.counters, args.into)
        return
    import torch
    assert torch.cuda.is_available(), "bench_dimers.py measures on the GPU; there is no CPU path"
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, **bench(args.pool, args.block, args.reps)}
    print(json.dumps(out))
    if args.out:
        _store(args.out, out)
    assert all(v for k, v in out["checks"].items() if isinstance(v, bool)), "the dimer calls differ from the oracle"


if __name__ == "__main__":
    main()
