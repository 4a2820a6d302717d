"""CPU oracle of the read mapper with affine gaps: the definition above polyhip_map_reads_affine in include/polyhip.h, i.e.
tests/map_oracle.py's map_read with tests/sw_affine_oracle.py's align in step 5.  Steps 1-4 are map_oracle's, line for line;
Params, Hit and occurrences are its own.  `mat` is a sw_affine_oracle.Mat."""
from __future__ import annotations

import map_oracle as mo
import oracle
import sw_affine_oracle as ao


def map_read(T: bytes, r: bytes, mat, go: int, ge: int, P: mo.Params, info: dict) -> mo.Hit:
    n, m, h = len(T), len(r), mo.Hit()
    clusters = []
    for s in range(2 if P.both_strands else 1):
        q = oracle.reverse_complement(r) if s else bytes(r)
        diags = []
        for o in range(0, m - P.seed_len + 1, P.seed_stride):
            info["seeds"] += 1
            occ = mo.occurrences(T, q[o:o + P.seed_len])
            if len(occ) > P.max_occ:
                info["seeds_over_max_occ"] += 1
                h.over += 1
                continue
            diags += [p - o for p in occ]
        info["hits"] += len(diags)
        diags.sort()
        i = 0
        while i < len(diags):
            j = i
            while j < len(diags) and diags[j] <= diags[i] + P.band:
                j += 1
            clusters.append((-(j - i), s, diags[i], diags[j - 1], q))
            i = j
    info["clusters"] += len(clusters)
    h.clusters = len(clusters)
    clusters.sort(key=lambda c: c[:3])
    results = []
    for nv, s, d0, dmax, q in clusters[:P.max_cand]:
        info["pairs_aligned"] += 1
        lo, hi = max(0, d0 - P.band), min(n, dmax + m + P.band)
        res = ao.align(q, T[lo:hi], mat, go, ge)
        results.append((res.score, res.alignA, res.alignB, res.endA, res.endB, res.err))
        h.cands.append((-nv, s, d0, dmax, lo, hi, res.score))
    for res in results:
        if res[5]:
            h.err = res[5]
            return h
    if not results:
        return h
    best = max(range(len(results)), key=lambda k: (results[k][0], -k))
    h.best_rank = best
    score, aa, ab, ea, eb, _ = results[best]
    if score < P.min_score:
        return h
    votes, s, _, _, lo, _, _ = h.cands[best]
    info["reads_mapped"] += 1
    h.score, h.flags, h.votes = score, 1 | (s << 1), votes
    h.second = max([x[0] for k, x in enumerate(results) if k != best], default=0)
    h.ref_end = lo + eb
    h.ref_start = h.ref_end - sum(1 for c in ab if c != 0x2D)
    h.read_end = ea
    h.read_start = ea - sum(1 for c in aa if c != 0x2D)
    h.alignA, h.alignB = aa, ab
    return h


def map_reads(T: bytes, reads, mat, go: int, ge: int, P: mo.Params):
    """-> (list of Hit, info dict with the six counters polyhip_map_affine_info shares with polyhip_map_info)"""
    info = dict(seeds=0, seeds_over_max_occ=0, hits=0, clusters=0, pairs_aligned=0, reads_mapped=0)
    return [map_read(bytes(T), bytes(r), mat, go, ge, P, info) for r in reads], info
