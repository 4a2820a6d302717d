"""The read mapper on one MI355X: reads/s of polyhip_map_reads_dev, and what its two borrowed halves cost alone.

    python scripts/bench_map.py [--genome 5000000] [--reads 1000000] [--reps 10] [--out profiles/map_bench.json]

- workload: a synthetic genome (polyhip_synth_dna_dev), reads of 150 bp sampled from it with 5 % substitutions and 1 % indels
  (half insertions, half deletions), every second one reverse-complemented; default parameters (mapper.MapParams);
- protocol: everything device-resident, one warm-up call, then --reps timed calls between device events (the call
  synchronises its stream itself: it reads two counts per chunk back); median and best are reported;
- parts, from the same process: polyhip_bwt_count_dev alone on the same seeds (every seed of both strands as a packed
  pattern batch) and polyhip_sw_align_batch_dev alone on candidate pairs rebuilt from the mapper's answers -- one pair per
  mapped read, its strand-oriented read against the window [ref_start - read_start - band, + m + 2 band) of the genome.  That
  is the chosen candidate's window up to its diagonal spread; the mapper's other kept candidates (pairs_aligned -
  reads_mapped of them) are not in this batch, which the JSON says in align_pairs;
- whole_over_parts = the mapper's time over the sum of the two parts.
Prints one JSON object (and writes it to --out).  Nothing here has a speed threshold.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


def mutate_windows(rng, src, m, sub=0.05, indel=0.01):
    """(k, span) uint8 windows -> (k, m): substitutions, deleted bases and inserted ones, then the first m bytes of each"""
    k, span = src.shape
    hit = rng.random(src.shape) < sub
    src[hit] = ACGT[(np.searchsorted(ACGT, src[hit]) + rng.integers(1, 4, int(hit.sum()))) & 3]
    u = rng.random(src.shape)
    copies = np.where(u < indel / 2, 0, np.where(u < indel, 2, 1))          # deleted / an inserted base in front / kept
    flat = np.repeat(src.reshape(-1), copies.reshape(-1))
    row = np.repeat(np.repeat(np.arange(k), span), copies.reshape(-1))
    first = np.concatenate([[0], np.cumsum(copies.sum(1))[:-1]])
    rank = np.arange(len(flat)) - first[row]
    ins = np.zeros(len(flat), bool)
    ins[np.nonzero(np.repeat(copies.reshape(-1), copies.reshape(-1)) == 2)[0][::2]] = True
    flat[ins] = ACGT[rng.integers(0, 4, int(ins.sum()))]
    keep = rank < m
    return flat[keep].reshape(k, m)


def make_reads(rng, g, nreads, m=150, sub=0.05, indel=0.01, block=100_000):
    """(nreads, m) uint8: windows of g with errors, odd rows reverse-complemented"""
    out = np.empty((nreads, m), np.uint8)
    span = m + 20
    for r0 in range(0, nreads, block):
        k = min(block, nreads - r0)
        src = g[rng.integers(0, len(g) - span, k)[:, None] + np.arange(span)]
        out[r0:r0 + k] = mutate_windows(rng, src, m, sub, indel)
    out[1::2] = COMP[out[1::2, ::-1]]
    return out


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from poly_amd import align, alphabet, bwt, mapper, mash, matrix
    assert torch.cuda.is_available(), "bench_map.py measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(17)
    n, N, m = args.genome, args.reads, 150
    P = mapper.MapParams()
    ab = alphabet.NewAlphabet(list("-ACGT"))
    sc = align.NewScoring(matrix.NewSubstitutionMatrix(ab, ab, matrix.NUC_4), -2)

    g_t = torch.empty(n, dtype=torch.uint8, device=dev)
    mash.synth_dna_dev(0x5EED + n, g_t)
    idx = bwt.new_dev(g_t)
    g = g_t.cpu().numpy()
    reads = make_reads(rng, g, N, m)
    r_t = torch.from_numpy(reads.reshape(-1)).to(dev)
    o_t = torch.arange(0, N * m + 1, m, dtype=torch.int64, device=dev)
    i64 = [torch.empty(N, dtype=torch.int64, device=dev) for _ in range(2)]
    i32 = [torch.empty(N, dtype=torch.int32, device=dev) for _ in range(7)]
    cap = 2 * N * m
    sa, sb = (torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(2))
    so = torch.empty(N + 1, dtype=torch.int64, device=dev)
    wb = mapper.workspace_bytes(idx, sc, P, N, m)
    work = torch.empty(wb, dtype=torch.uint8, device=dev)
    t_map, t_map_best = timed(lambda: mapper.map_reads_dev(idx, sc, r_t, o_t, m, P, *i64, *i32, sa, sb, so, work), args.reps)
    info = mapper.last_info()
    flags, rs, qs = (i32[k].cpu().numpy().view(np.uint32) for k in (0, 2, 4))
    del work, sa, sb
    torch.cuda.empty_cache()

    # part 1: Count alone on the same seeds
    offs = np.arange(0, m - P.seed_len + 1, P.seed_stride)
    both = np.stack([reads, COMP[reads[:, ::-1]]], 1) if P.both_strands else reads[:, None, :]
    seeds = both[:, :, offs[:, None] + np.arange(P.seed_len)]                    # (N, strands, seeds, L)
    nseeds = seeds.size // P.seed_len
    p_t = torch.from_numpy(np.ascontiguousarray(seeds).reshape(-1)).to(dev)
    po_t = torch.arange(0, seeds.size + 1, P.seed_len, dtype=torch.int64, device=dev)
    s_t, e_t, x_t = (torch.empty(nseeds, dtype=torch.int32, device=dev) for _ in range(3))
    t_count, _ = timed(lambda: bwt.count_dev(idx, p_t, po_t, s_t, e_t, x_t), args.reps)
    del p_t, po_t, s_t, e_t, x_t, seeds

    # part 2: the aligner alone on one pair per mapped read
    mp = np.nonzero(flags & 1)[0]
    q = np.where((flags[mp, None] & 2) != 0, both[mp, -1], reads[mp])
    lo = np.maximum(0, rs[mp].astype(np.int64) - qs[mp] - P.band)
    hi = np.minimum(n, lo + m + 2 * P.band)
    lenB = int((hi - lo).max())
    offB = np.concatenate([[0], np.cumsum(hi - lo)])
    B = np.concatenate([g[a:b] for a, b in zip(lo, hi)])
    npairs = len(mp)
    A_t = torch.from_numpy(np.ascontiguousarray(q).reshape(-1)).to(dev)
    oA_t = torch.arange(0, npairs * m + 1, m, dtype=torch.int64, device=dev)
    B_t = torch.from_numpy(np.concatenate([B, np.zeros(64, np.uint8)])).to(dev)
    oB_t = torch.from_numpy(offB.astype(np.int64)).to(dev)
    stride = align.sw_traceback_stride(sc, m, lenB)
    score_t = torch.empty(npairs, dtype=torch.int64, device=dev)
    ea, eb, er, al = (torch.empty(npairs, dtype=torch.int32, device=dev) for _ in range(4))
    alnA, alnB = (torch.empty((npairs, stride), dtype=torch.uint8, device=dev) for _ in range(2))
    w1 = torch.empty(max(align.sw_workspace_bytes(sc, npairs, m, lenB, shared=False), 256), dtype=torch.uint8, device=dev)
    w2 = torch.empty(align.sw_traceback_workspace_bytes(sc, min(npairs, 131072), m, lenB), dtype=torch.uint8, device=dev)
    t_align, _ = timed(lambda: align.sw_align_dev(sc, A_t, oA_t, m, B_t, oB_t, lenB, score_t, ea, eb, er, alnA, alnB, al, w1, w2),
                       args.reps)

    out = {"device": torch.cuda.get_device_name(0), "genome": n, "reads": N, "read_len": m, "params": P.__dict__,
           "workspace_bytes": wb, "reps": args.reps,
           "map_s": t_map, "map_s_best": t_map_best, "reads_per_s": N / t_map, "info": info,
           "count_alone_s": t_count, "count_patterns": nseeds,
           "align_alone_s": t_align, "align_pairs": npairs, "align_paths": [align.last_path(), align.sw_traceback_last_path()],
           "whole_over_parts": t_map / (t_count + t_align)}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
