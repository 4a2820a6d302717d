"""CPU oracle of the read mapper on a reference of several contigs: the definition above polyhip_map_reads_refs in
include/polyhip.h in plain Python.  It is tests/map_affine_oracle.py's map_read and tests/map_pairs_oracle.py's map_pair with
the changes that comment names: a seed is counted on the concatenation C and located per contig (bytes.find on each), clusters
are per (strand, contig), windows end at the contig's ends, a proper pair lies on one contig, a rescue window inside the
anchor's.  Hit, Cand, Params, PairParams, proper_insert and every alignment (tests/sw_affine_oracle.py) are the existing
oracles' own.  It is the only definition the GPU is compared with."""
from __future__ import annotations

from dataclasses import dataclass

import map_oracle as mo
import map_pairs_oracle as mpo
import oracle

COUNTERS = ("seeds", "seeds_over_max_occ", "hits", "clusters", "pairs_aligned", "reads_mapped")
PAIR_COUNTERS = mpo.COUNTERS
REFS_COUNTERS = ("straddling",)


@dataclass
class RHit(mo.Hit):
    rid: int = 0


@dataclass
class RCand(mpo.Cand):
    rid: int = 0


def new_info(pairs: bool = False) -> dict:
    return dict.fromkeys((PAIR_COUNTERS if pairs else COUNTERS) + REFS_COUNTERS, 0)


def candidates(contigs, r: bytes, mat, go: int, ge: int, P: mo.Params, max_len: int, info: dict):
    """steps 1-5 for one read -> (kept candidates by rank, err of the read, clusters before the cut, seeds over max_occ)"""
    m = len(r)
    if m > max_len:
        return [], 0xFFFFFFFF, 0, 0
    C = b"".join(contigs)
    clusters, over = [], 0
    for s in range(2 if P.both_strands else 1):
        q = oracle.reverse_complement(r) if s else bytes(r)
        diags = [[] for _ in contigs]
        for o in range(0, m - P.seed_len + 1, P.seed_stride):
            info["seeds"] += 1
            seed = q[o:o + P.seed_len]
            count = len(mo.occurrences(C, seed))          # judged on C: the straddling occurrences count
            if count > P.max_occ:
                info["seeds_over_max_occ"] += 1
                over += 1
                continue
            kept = 0
            for c, Tc in enumerate(contigs):
                occ = mo.occurrences(Tc, seed)
                diags[c] += [p - o for p in occ]
                kept += len(occ)
            info["hits"] += kept
            info["straddling"] += count - kept
        for c, dc in enumerate(diags):
            dc.sort()
            i = 0
            while i < len(dc):
                j = i
                while j < len(dc) and dc[j] <= dc[i] + P.band:
                    j += 1
                clusters.append((-(j - i), s, c, dc[i], dc[j - 1], q))
                i = j
    info["clusters"] += len(clusters)
    clusters.sort(key=lambda c: c[:4])
    out = []
    for nv, s, c, d0, dmax, q in clusters[:P.max_cand]:
        info["pairs_aligned"] += 1
        lo, hi = max(0, d0 - P.band), min(len(contigs[c]), dmax + m + P.band)
        out.append(RCand(-nv, s, lo, hi, q, mpo._align(q, contigs[c][lo:hi], mat, go, ge), c))
    err = next((c.res.err for c in out if c.res.err), 0)
    return out, err, len(clusters), over


def _place(h: RHit, res, strand: int, lo: int, votes: int, extra: int, rid: int):
    mpo._place(h, res, strand, lo, votes, extra)
    h.rid = rid


def map_read(contigs, r: bytes, mat, go: int, ge: int, P: mo.Params, info: dict, max_len: int | None = None) -> RHit:
    contigs = [bytes(t) for t in contigs]
    h = RHit()
    cands, h.err, h.clusters, h.over = candidates(contigs, bytes(r), mat, go, ge, P, len(r) if max_len is None else max_len, info)
    h.cands = [(k.votes, k.strand, k.rid, None, k.lo, k.hi, k.res.score) for k in cands]
    if h.err or not cands:
        return h
    best = max(range(len(cands)), key=lambda k: (cands[k].res.score, -k))
    h.best_rank = best
    c = cands[best]
    if c.res.score < P.min_score:
        return h
    info["reads_mapped"] += 1
    _place(h, c.res, c.strand, c.lo, c.votes, 0, c.rid)
    h.second = max([x.res.score for k, x in enumerate(cands) if k != best], default=0)
    return h


def map_reads(contigs, reads, mat, go: int, ge: int, P: mo.Params, max_len: int | None = None):
    """-> (list of RHit, the counters summed)"""
    if max_len is None:
        max_len = max((len(r) for r in reads), default=0)
    info = new_info()
    return [map_read(contigs, r, mat, go, ge, P, info, max_len) for r in reads], info


def _left(c) -> int:
    return c.lo + c.res.endB - c.res.endA


def map_pair(contigs, r1: bytes, r2: bytes, mat, go: int, ge: int, P: mo.Params, PP: mpo.PairParams, max_len: int) -> mpo.PairResult:
    contigs, reads = [bytes(t) for t in contigs], (bytes(r1), bytes(r2))
    W = P.band
    info = new_info(True)
    out = mpo.PairResult(RHit(), RHit(), info=info)
    hits = (out.h1, out.h2)
    cands, errs = [], []
    for x in range(2):
        c, e, _, _ = candidates(contigs, reads[x], mat, go, ge, P, max_len, info)
        cands.append(c)
        errs.append(e)
        hits[x].err = e
        hits[x].cands = [(k.votes, k.strand, k.rid, None, k.lo, k.hi, k.res.score) for k in c]
    usable = [[errs[x] == 0 and c.res.score >= P.min_score for c in cands[x]] for x in range(2)]
    single = []
    for x in range(2):
        best = max(range(len(cands[x])), key=lambda k: (cands[x][k].res.score, -k), default=-1)
        single.append(best if best >= 0 and usable[x][best] else -1)
        hits[x].best_rank = best if errs[x] == 0 else -1
    chosen = [-1, -1]          # rank of the chosen candidate; -2: the rescue window
    rescued = None
    if errs[0] == 0 and errs[1] == 0:
        out.combos = len(cands[0]) * len(cands[1])
    for k1, a in enumerate(cands[0]):
        for k2, b in enumerate(cands[1]):
            if usable[0][k1] and usable[1][k2] and a.rid == b.rid:                     # one contig: left and right are local
                ins = mpo.proper_insert(a.strand, _left(a), len(reads[0]), b.strand, _left(b), len(reads[1]), PP)
                if ins >= 0:
                    out.proper_combos.append((a.res.score + b.res.score, k1, k2, ins))
    if out.proper_combos:
        _, k1, k2, ins = max(out.proper_combos, key=lambda c: (c[0], -c[1], -c[2]))
        chosen, out.proper, out.tlen, out.case = [k1, k2], True, ins, "pair"
    elif PP.rescue:
        for x in range(2):
            y = 1 - x
            if single[x] < 0 or errs[y] != 0 or len(reads[y]) < 1:
                continue
            a, my = cands[x][single[x]], len(reads[y])
            Tc = contigs[a.rid]
            la = _left(a)
            ra = la + len(reads[x])
            raw = (la + PP.min_insert - my - W, la + PP.max_insert + W) if a.strand == 0 else \
                (ra - PP.max_insert - W, ra - PP.min_insert + my + W)
            wlo, whi = max(raw[0], 0), min(raw[1], len(Tc))                              # the anchor's contig
            at = mpo.Attempt(x + 1, raw, wlo, whi, strand=1 - a.strand)
            out.attempts.append(at)
            if wlo >= whi:
                continue
            info["rescue_attempts"] += 1
            q = oracle.reverse_complement(reads[y]) if at.strand else reads[y]
            at.res = mpo._align(q, Tc[wlo:whi], mat, go, ge)
            if at.res.err == 0 and at.res.score >= P.min_score:
                at.insert = mpo.proper_insert(a.strand, la, len(reads[x]), at.strand, wlo + at.res.endB - at.res.endA, my, PP)
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
    extra = mpo.FLAG_PROPER if out.proper else 0
    for x in range(2):
        scores = [c.res.score for c in cands[x]]
        if chosen[x] == -2:
            anchor = cands[1 - x][chosen[1 - x]]
            _place(hits[x], rescued.res, rescued.strand, rescued.wlo, 0, extra | mpo.FLAG_RESCUED, anchor.rid)
            hits[x].second = max(scores, default=0)
        elif chosen[x] >= 0:
            c = cands[x][chosen[x]]
            _place(hits[x], c.res, c.strand, c.lo, c.votes, extra, c.rid)
            hits[x].second = max([s for k, s in enumerate(scores) if k != chosen[x]], default=0)
        info["reads_mapped"] += hits[x].flags & 1
    out.ranks = tuple(k if k >= 0 else -1 for k in chosen)
    info["proper_pairs"] += out.proper
    return out


def map_pairs(contigs, reads1, reads2, mat, go: int, ge: int, P: mo.Params, PP: mpo.PairParams, max_len: int | None = None):
    """-> (list of PairResult, the counters summed)"""
    if max_len is None:
        max_len = max((len(r) for r in list(reads1) + list(reads2)), default=0)
    res = [map_pair(contigs, a, b, mat, go, ge, P, PP, max_len) for a, b in zip(reads1, reads2)]
    return res, {k: sum(r.info[k] for r in res) for k in PAIR_COUNTERS + REFS_COUNTERS}
