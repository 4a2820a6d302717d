"""CPU oracle of the read mapper: the definition in include/polyhip.h (polyhip_map_reads) restated in plain Python on
the two oracles the project already trusts -- bytes.find for the seeds (tests/bwt_oracle.py's Locate gives the same
sets), oracle.smith_waterman and oracle.reverse_complement for the extension.  It is the only definition the GPU is
compared with."""
from __future__ import annotations

from dataclasses import dataclass, field

import oracle


@dataclass
class Params:
    seed_len: int = 20
    seed_stride: int = 10
    max_occ: int = 32
    band: int = 24
    max_cand: int = 4
    both_strands: bool = True
    min_score: int = 1


@dataclass
class Hit:
    score: int = 0
    second: int = 0
    flags: int = 0
    votes: int = 0
    ref_start: int = 0
    ref_end: int = 0
    read_start: int = 0
    read_end: int = 0
    err: int = 0
    alignA: bytes = b""
    alignB: bytes = b""
    # what the tests' input conditions look at (not outputs of the mapper)
    over: int = 0          # seeds dropped for max_occ
    clusters: int = 0      # before the cut to max_cand
    cands: list = field(default_factory=list)   # (votes, strand, d0, dmax, lo, hi, score) by rank
    best_rank: int = -1


def occurrences(T: bytes, seed: bytes):
    if b"$" in seed:
        return []
    out, p = [], T.find(seed)
    while p >= 0:
        out.append(p)
        p = T.find(seed, p + 1)
    return out


def map_read(T: bytes, r: bytes, mat, gap: int, P: Params, info: dict) -> Hit:
    n, m, h = len(T), len(r), Hit()
    clusters = []
    for s in range(2 if P.both_strands else 1):
        q = oracle.reverse_complement(r) if s else bytes(r)
        diags = []
        for o in range(0, m - P.seed_len + 1, P.seed_stride):
            info["seeds"] += 1
            occ = occurrences(T, q[o:o + P.seed_len])
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
        try:
            score, aa, ab, ea, eb = oracle.smith_waterman(q, T[lo:hi], mat, gap)
            e = 0
        except oracle.AlphabetError as ex:
            score, aa, ab, ea, eb, e = 0, "", "", 0, 0, (ex.side << 8) | ex.symbol
        results.append((score, aa.encode("latin-1"), ab.encode("latin-1"), ea, eb, e))
        h.cands.append((-nv, s, d0, dmax, lo, hi, score))
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


def map_reads(T: bytes, reads, mat, gap: int, P: Params):
    """-> (list of Hit, info dict with the counters of polyhip_map_info but `chunks`)"""
    info = dict(seeds=0, seeds_over_max_occ=0, hits=0, clusters=0, pairs_aligned=0, reads_mapped=0)
    return [map_read(bytes(T), bytes(r), mat, gap, P, info) for r in reads], info
