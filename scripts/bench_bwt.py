"""search/bwt on one MI355X: index build, batched Count and Locate, against the random-line read rate.

    python scripts/bench_bwt.py [--sizes 5000000,100000000] [--npat 1000000] [--reps 5] [--out FILE]

- build: polyhip_bwt_create_dev on a synthetic genome (polyhip_synth_dna_dev), wall time of the (synchronous) call;
- Count: 1M x 32-mers, half sampled from the genome and half with two random substitutions, one count_dev call
  (device events, best of --reps after a warm-up); reported as patterns/s and LF steps/s, where the steps are the
  ones the search really takes (a lane stops once its range is empty: counted here from the intervals of every
  suffix of the pattern, i.e. from the library's own answers);
- Locate: 1M x 20-mers sampled from the genome: locate_dev on their intervals (events, best of --reps);
- roofline: an LF step of the nucleotide layout reads one 128-byte line per range end, 256 B per step; the rate of
  uniformly random 128-byte lines from a table the size of the occurrence structure is MEASURED by
  scripts/ubench/random_lines.hip in the same run (compiled here with hipcc), not estimated.
Prints one JSON object (and writes it to --out).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def random_line_rates(table_bytes):
    src = os.path.join(ROOT, "scripts", "ubench", "random_lines.hip")
    exe = os.path.join(ROOT, "scripts", "ubench", "random_lines")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        from poly_amd import build
        subprocess.run([build._hipcc(), "--offload-arch=gfx950", "-O3", "-o", exe, src], check=True)
    res = subprocess.run([exe] + [str(int(b)) for b in table_bytes], capture_output=True, text=True, timeout=300)
    if res.returncode:
        raise RuntimeError(res.stdout + res.stderr)
    return [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="5000000,100000000")
    ap.add_argument("--npat", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from poly_amd import bwt, mash
    assert torch.cuda.is_available(), "bench_bwt.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    out = {"device": torch.cuda.get_device_name(0), "npat": args.npat, "genomes": []}

    # warm-up: code objects, the allocator
    w = torch.empty(100_000, dtype=torch.uint8, device=dev)
    mash.synth_dna_dev(1, w)
    bwt.new_dev(w)

    occ_bytes = []
    for n in [int(x) for x in args.sizes.split(",")]:
        g_t = torch.empty(n, dtype=torch.uint8, device=dev)
        mash.synth_dna_dev(0x5EED + n, g_t)
        work = torch.empty(bwt.workspace_bytes(n), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx = bwt.new_dev(g_t, work)
        t_build = time.perf_counter() - t0
        del work
        lines = n // 448 + 2
        occ_bytes.append(lines * 128)
        g = g_t.cpu().numpy()

        # Count: 1M x 32-mers, half exact, half with two substitutions
        m = 32
        st = rng.integers(0, n - m, args.npat)
        pats = g[st[:, None] + np.arange(m)]
        half = pats[args.npat // 2:]
        for _ in range(2):
            half[np.arange(len(half)), rng.integers(0, m, len(half))] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(half))]
        p_t = torch.from_numpy(pats.reshape(-1).copy()).to(dev)
        o_t = torch.arange(0, pats.size + 1, m, dtype=torch.int64, device=dev)
        s_t = torch.empty(args.npat, dtype=torch.int32, device=dev)
        e_t, err_t = torch.empty_like(s_t), torch.empty_like(s_t)
        t_count = timed(lambda: bwt.count_dev(idx, p_t, o_t, s_t, e_t, err_t), args.reps)
        # LF steps really taken: a pattern takes one step per symbol until its range is empty, i.e. 1 + the length of
        # its longest matching suffix (capped at m): the counts of the suffixes p[m-k:] say where that is
        steps = np.zeros(args.npat, np.int64)
        alive = np.ones(args.npat, bool)
        for k in range(1, m + 1):
            suf = pats[:, m - k:]
            sp = torch.from_numpy(suf.reshape(-1).copy()).to(dev)
            so = torch.arange(0, suf.size + 1, k, dtype=torch.int64, device=dev)
            bwt.count_dev(idx, sp, so, s_t, e_t, err_t)
            c = (e_t.cpu().numpy().view(np.uint32) > s_t.cpu().numpy().view(np.uint32))
            steps += alive
            alive &= c
        lf_steps = int(steps.sum())

        # Locate: 1M x 20-mers from the genome
        m2 = 20
        st2 = rng.integers(0, n - m2, args.npat)
        pats2 = g[st2[:, None] + np.arange(m2)]
        p2 = torch.from_numpy(pats2.reshape(-1).copy()).to(dev)
        o2 = torch.arange(0, pats2.size + 1, m2, dtype=torch.int64, device=dev)
        s2, e2, r2 = (torch.empty(args.npat, dtype=torch.int32, device=dev) for _ in range(3))
        bwt.count_dev(idx, p2, o2, s2, e2, r2)
        total = int((e2.cpu().numpy().view(np.uint32).astype(np.int64) - s2.cpu().numpy().view(np.uint32)).sum())
        first = torch.empty(args.npat + 1, dtype=torch.int64, device=dev)
        loc = torch.empty(total, dtype=torch.int32, device=dev)
        lw = torch.empty(max(bwt.locate_workspace_bytes(args.npat), 1), dtype=torch.uint8, device=dev)
        t_locate = timed(lambda: bwt.locate_dev(idx, s2, e2, first, loc, lw), args.reps)
        t_c2 = timed(lambda: bwt.count_dev(idx, p2, o2, s2, e2, r2), args.reps)
        out["genomes"].append({
            "n": n, "layout": idx.Layout(), "doubling_rounds": idx.Rounds(), "build_s": round(t_build, 4),
            "occ_structure_bytes": lines * 128,
            "count32": {"s": t_count, "patterns_per_s": args.npat / t_count, "lf_steps": lf_steps,
                        "lf_steps_per_s": lf_steps / t_count, "line_reads_per_s": 2 * lf_steps / t_count},
            "locate20": {"s": t_locate, "count_s": t_c2, "offsets": total, "patterns_per_s": args.npat / t_locate,
                         "offsets_per_s": total / t_locate},
        })
        del idx
        torch.cuda.empty_cache()

    out["random_lines"] = random_line_rates(occ_bytes)
    for gen, rl in zip(out["genomes"], out["random_lines"]):
        gen["count32"]["share_of_random_line_rate"] = gen["count32"]["line_reads_per_s"] / rl["lines_per_s"]
    txt = json.dumps(out)
    print(txt)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
