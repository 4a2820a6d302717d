"""CPU oracle of the paired-end read mapper: the definition above polyhip_map_pairs in include/polyhip.h in plain Python.
Steps 1-4 of a mate (strands, seeds, clusters, ranks) are tests/map_oracle.py's, line for line, as tests/map_affine_oracle.py
restates them; every alignment is tests/sw_affine_oracle.py's align.  One pair in, both mates' Hits out, plus proper, tlen,
the counters and which of the definition's cases applied.  It is the only definition the GPU is compared with."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import map_oracle as mo
import oracle
import sw_affine_oracle as ao

FLAG_PROPER, FLAG_RESCUED = 4, 8
COUNTERS = ("seeds", "seeds_over_max_occ", "hits", "clusters", "pairs_aligned", "reads_mapped", "proper_pairs", "rescue_attempts",
            "rescued")


@dataclass
class PairParams:
    min_insert: int
    max_insert: int
    rescue: bool = True


@dataclass
class Cand:
    votes: int
    strand: int
    lo: int
    hi: int
    q: bytes
    res: ao.Result


@dataclass
class Attempt:
    """one rescue window: the mate that anchors it (1 or 2), the unclipped and the clipped window, what came of it"""
    anchor: int
    raw: tuple
    wlo: int
    whi: int
    strand: int = 0
    res: ao.Result | None = None
    insert: int = -1          # >= 0: the attempt succeeded
    total: int = 0


@dataclass
class PairResult:
    h1: mo.Hit
    h2: mo.Hit
    proper: bool = False
    tlen: int = 0
    case: str = "fallback"    # "pair" (step 3), "rescue" (step 4) or "fallback" (step 5)
    ranks: tuple = (-1, -1)   # the candidates' ranks of the mates (-1: unmapped or rescued)
    combos: int = 0           # combinations (k1, k2) step 3 looked at: nc1 * nc2 when both mates are free of errors
    proper_combos: list = field(default_factory=list)   # (sum, k1, k2, insert) of every proper one
    attempts: list = field(default_factory=list)
    anchor: int = 0           # the mate that anchored the rescue that won (1 or 2)
    info: dict = field(default_factory=dict)


@functools.lru_cache(maxsize=None)
def _align(q: bytes, window: bytes, mat, go: int, ge: int):
    return ao.align(q, window, mat, go, ge)


def candidates(T: bytes, r: bytes, mat, go: int, ge: int, P: mo.Params, max_len: int, info: dict):
    """steps 1-5 of polyhip_map_reads_affine for one mate -> (kept candidates by rank, err of the mate)"""
    n, m = len(T), len(r)
    if m > max_len:
        return [], 0xFFFFFFFF
    clusters = []
    for s in range(2 if P.both_strands else 1):
        q = oracle.reverse_complement(r) if s else bytes(r)
        diags = []
        for o in range(0, m - P.seed_len + 1, P.seed_stride):
            info["seeds"] += 1
            occ = mo.occurrences(T, q[o:o + P.seed_len])
            if len(occ) > P.max_occ:
                info["seeds_over_max_occ"] += 1
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
    clusters.sort(key=lambda c: c[:3])
    out = []
    for nv, s, d0, dmax, q in clusters[:P.max_cand]:
        info["pairs_aligned"] += 1
        lo, hi = max(0, d0 - P.band), min(n, dmax + m + P.band)
        out.append(Cand(-nv, s, lo, hi, q, _align(q, T[lo:hi], mat, go, ge)))
    err = next((c.res.err for c in out if c.res.err), 0)
    return out, err


def proper_insert(sa: int, la: int, ma: int, sb: int, lb: int, mb: int, PP: PairParams) -> int:
    """step 2: the insert when (strand, left, length) a and b are a proper combination, else -1"""
    if sa == sb:
        return -1
    (lf, mf), (lr, mr) = ((la, ma), (lb, mb)) if sa == 0 else ((lb, mb), (la, ma))
    ins = lr + mr - lf
    return ins if lf <= lr and lf + mf <= lr + mr and PP.min_insert <= ins <= PP.max_insert else -1


def _left(c: Cand) -> int:
    return c.lo + c.res.endB - c.res.endA


def _place(h: mo.Hit, res, strand: int, lo: int, votes: int, extra: int):
    h.score, h.flags, h.votes = res.score, 1 | (strand << 1) | extra, votes
    h.ref_end = lo + res.endB
    h.ref_start = h.ref_end - sum(1 for c in res.alignB if c != 0x2D)
    h.read_end = res.endA
    h.read_start = res.endA - sum(1 for c in res.alignA if c != 0x2D)
    h.alignA, h.alignB = res.alignA, res.alignB


def map_pair(T: bytes, r1: bytes, r2: bytes, mat, go: int, ge: int, P: mo.Params, PP: PairParams, max_len: int) -> PairResult:
    T, reads = bytes(T), (bytes(r1), bytes(r2))
    n, W = len(T), P.band
    info = dict.fromkeys(COUNTERS, 0)
    out = PairResult(mo.Hit(), mo.Hit(), info=info)
    hits = (out.h1, out.h2)
    cands, errs = [], []
    for x in range(2):
        c, e = candidates(T, reads[x], mat, go, ge, P, max_len, info)
        cands.append(c)
        errs.append(e)
        hits[x].err = e
        hits[x].cands = [(k.votes, k.strand, None, None, k.lo, k.hi, k.res.score) for k in c]
    usable = [[errs[x] == 0 and c.res.score >= P.min_score for c in cands[x]] for x in range(2)]
    # step 6's winner of each mate on its own: the anchor of a rescue, and the fallback
    single = []
    for x in range(2):
        best = max(range(len(cands[x])), key=lambda k: (cands[x][k].res.score, -k), default=-1)
        single.append(best if best >= 0 and usable[x][best] else -1)
        hits[x].best_rank = best if errs[x] == 0 else -1
    chosen = [-1, -1]          # rank of the chosen candidate; -2: the rescue window
    rescued = None
    # step 3
    if errs[0] == 0 and errs[1] == 0:
        out.combos = len(cands[0]) * len(cands[1])
    for k1, a in enumerate(cands[0]):
        for k2, b in enumerate(cands[1]):
            if usable[0][k1] and usable[1][k2]:
                ins = proper_insert(a.strand, _left(a), len(reads[0]), b.strand, _left(b), len(reads[1]), PP)
                if ins >= 0:
                    out.proper_combos.append((a.res.score + b.res.score, k1, k2, ins))
    if out.proper_combos:
        _, k1, k2, ins = max(out.proper_combos, key=lambda c: (c[0], -c[1], -c[2]))
        chosen, out.proper, out.tlen, out.case = [k1, k2], True, ins, "pair"
    elif PP.rescue:
        # step 4
        for x in range(2):
            y = 1 - x
            if single[x] < 0 or errs[y] != 0 or len(reads[y]) < 1:
                continue
            a, my = cands[x][single[x]], len(reads[y])
            la = _left(a)
            ra = la + len(reads[x])
            raw = (la + PP.min_insert - my - W, la + PP.max_insert + W) if a.strand == 0 else \
                (ra - PP.max_insert - W, ra - PP.min_insert + my + W)
            wlo, whi = max(raw[0], 0), min(raw[1], n)
            at = Attempt(x + 1, raw, wlo, whi, strand=1 - a.strand)
            out.attempts.append(at)
            if wlo >= whi:
                continue
            info["rescue_attempts"] += 1
            q = oracle.reverse_complement(reads[y]) if at.strand else reads[y]
            at.res = _align(q, T[wlo:whi], mat, go, ge)
            if at.res.err == 0 and at.res.score >= P.min_score:
                at.insert = proper_insert(a.strand, la, len(reads[x]), at.strand, wlo + at.res.endB - at.res.endA, my, PP)
                at.total = a.res.score + at.res.score
        good = [at for at in out.attempts if at.insert >= 0]
        if good:
            rescued = max(good, key=lambda at: (at.total, -at.anchor))
            x = rescued.anchor - 1
            chosen[x], chosen[1 - x] = single[x], -2
            out.proper, out.tlen, out.case, out.anchor = True, rescued.insert, "rescue", rescued.anchor
            info["rescued"] += 1
    if out.case == "fallback":
        chosen = single
    extra = FLAG_PROPER if out.proper else 0
    for x in range(2):
        scores = [c.res.score for c in cands[x]]
        if chosen[x] == -2:
            _place(hits[x], rescued.res, rescued.strand, rescued.wlo, 0, extra | FLAG_RESCUED)
            hits[x].second = max(scores, default=0)
        elif chosen[x] >= 0:
            c = cands[x][chosen[x]]
            _place(hits[x], c.res, c.strand, c.lo, c.votes, extra)
            hits[x].second = max([s for k, s in enumerate(scores) if k != chosen[x]], default=0)
        info["reads_mapped"] += hits[x].flags & 1
    out.ranks = tuple(k if k >= 0 else -1 for k in chosen)
    info["proper_pairs"] += out.proper
    return out


def map_pairs(T: bytes, reads1, reads2, mat, go: int, ge: int, P: mo.Params, PP: PairParams, max_len: int | None = None):
    """-> (list of PairResult, the counters summed)"""
    if max_len is None:
        max_len = max((len(r) for r in list(reads1) + list(reads2)), default=0)
    res = [map_pair(T, a, b, mat, go, ge, P, PP, max_len) for a, b in zip(reads1, reads2)]
    return res, {k: sum(r.info[k] for r in res) for k in COUNTERS}
