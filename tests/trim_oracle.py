"""polyhip_trim_reads / polyhip_trim_pairs in plain Python loops: the definition in the comment above the calls in
include/polyhip.h, step by step, one byte at a time.  Nothing here is vectorised; numpy only holds the results."""
from types import SimpleNamespace

import numpy as np

F_QUAL_3P, F_QUAL_5P, F_ADAPTER, F_SHORT, F_OVERLAP = 1, 2, 4, 8, 16
INFO_FIELDS = ("reads", "bytes_in", "bytes_out", "cut_3p", "cut_5p", "adapter_hits", "overlap_cut", "too_short", "bad")
DEFAULTS = dict(qual_offset=33, min_qual_5p=0, min_qual_3p=0, adapter_err_pct=10, min_overlap=3, min_len=0, pair_min_overlap=0,
                pair_err_pct=10)
COMP = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}


def upper(c):
    return c - 32 if ord("a") <= c <= ord("z") else c


def judge(m, q, qual_offset):
    """step 1: err of a read of m bytes with quality string q (None: no qualities)"""
    if q is None:
        return 0
    if len(q) != m:
        return 1
    for c in q:
        if c < qual_offset or c > qual_offset + 93:
            return 2
    return 0


def walk(Q, cutoff):
    """step 2, one end: Q in walking order.  How many bytes the end loses"""
    s, best, ncut = 0, 0, 0
    for j in range(len(Q)):
        s += cutoff - Q[j]
        if s < 0:
            break
        if s > best:
            best, ncut = s, j + 1
    return ncut


def quality_ends(q, qual_offset, min_qual_5p, min_qual_3p, m):
    """step 2: (a, b, flags)"""
    a, b = 0, m
    if min_qual_3p > 0:
        b = m - walk([q[k] - qual_offset for k in range(m - 1, -1, -1)], min_qual_3p)
    if min_qual_5p > 0:
        a = walk([q[k] - qual_offset for k in range(m)], min_qual_5p)
    if a >= b:
        a = b = 0
    return a, b, (F_QUAL_3P if b < m else 0) | (F_QUAL_5P if a > 0 else 0)


def mismatches(r, s, t, L):
    n = 0
    for k in range(L):
        if upper(r[s + k]) != t[k]:          # t is upper-case ACGT: every other read byte differs from it
            n += 1
    return n


def find_adapter(r, a, b, adapters, adapter_err_pct, min_overlap):
    """step 3: (s, adapter index) of the hit, or None"""
    for s in range(a, b):
        for t in range(len(adapters)):
            L = min(len(adapters[t]), b - s)
            if L >= min_overlap and 100 * mismatches(r, s, adapters[t], L) <= adapter_err_pct * L:
                return s, t
    return None


def find_insert(r1, r2, pair_min_overlap, pair_err_pct):
    """step P: the greatest qualifying I, or None"""
    for I in range(min(len(r1), len(r2)), pair_min_overlap - 1, -1):
        if I < 1:
            break
        mism = 0
        for k in range(I):
            if COMP.get(upper(r2[I - 1 - k]), -1) != upper(r1[k]):
                mism += 1
        if 100 * mism <= pair_err_pct * I:
            return I
    return None


def _steps_1_to_3(r, q, adapters, P):
    m = len(r)
    err = judge(m, q, P["qual_offset"])
    if err:
        return 0, 0, 0, err
    a, b, flags = quality_ends(q, P["qual_offset"], P["min_qual_5p"], P["min_qual_3p"], m) if q is not None else (0, m, 0)
    hit = find_adapter(r, a, b, adapters, P["adapter_err_pct"], P["min_overlap"])
    if hit is not None:
        b = hit[0]
        flags |= F_ADAPTER | hit[1] << 8
    return a, b, flags, 0


def _params(kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def _finish(entries, reads, quals, P, nbatch):
    """step 4 and 5 for the decided entries [(a, b, flags, err)] in entry order; reads / quals: per batch, lists of bytes"""
    n = len(entries)
    start, end, flags, err = (np.zeros(n, np.uint32) for _ in range(4))
    out = [dict(seqs=bytearray(), quals=bytearray() if quals[q] is not None else None, offsets=[0]) for q in range(nbatch)]
    info = dict.fromkeys(INFO_FIELDS, 0)
    info["reads"] = n
    for e, (a, b, f, er) in enumerate(entries):
        q, i = e % nbatch, e // nbatch
        keep = not er
        if not er and b - a < P["min_len"]:
            f |= F_SHORT
            keep = False
        start[e], end[e], flags[e], err[e] = a, b, f, er
        o = out[q]
        if keep:
            o["seqs"] += reads[q][i][a:b]
            if o["quals"] is not None:
                o["quals"] += quals[q][i][a:b]
        o["offsets"].append(len(o["seqs"]))
        info["bytes_in"] += len(reads[q][i])
        info["cut_3p"] += bool(f & F_QUAL_3P)
        info["cut_5p"] += bool(f & F_QUAL_5P)
        info["adapter_hits"] += bool(f & F_ADAPTER)
        info["overlap_cut"] += bool(f & F_OVERLAP)
        info["too_short"] += bool(f & F_SHORT)
        info["bad"] += bool(er)
    info["bytes_out"] = sum(len(o["seqs"]) for o in out)
    conv = [(np.frombuffer(bytes(o["seqs"]), np.uint8), np.array(o["offsets"], np.uint64),
             None if o["quals"] is None else np.frombuffer(bytes(o["quals"]), np.uint8)) for o in out]
    return start, end, flags, err, conv, info


def trim_reads(reads, quals=None, adapters=(), **kw):
    """reads: list of bytes; quals: list of bytes or None -> the fields of trim.Trimmed, and info"""
    P = _params(kw)
    adapters = [bytes(a) for a in adapters]
    entries = [_steps_1_to_3(reads[i], None if quals is None else quals[i], adapters, P) for i in range(len(reads))]
    start, end, flags, err, conv, info = _finish(entries, [reads], [quals], P, 1)
    return SimpleNamespace(seqs=conv[0][0], offsets=conv[0][1], quals=conv[0][2], start=start, end=end, flags=flags, err=err, info=info)


def trim_pairs(reads1, reads2, quals1=None, quals2=None, adapters=(), **kw):
    P = _params(kw)
    adapters = [bytes(a) for a in adapters]
    assert len(reads1) == len(reads2)
    entries = []
    for i in range(len(reads1)):
        mates = [list(_steps_1_to_3(reads1[i], None if quals1 is None else quals1[i], adapters, P)),
                 list(_steps_1_to_3(reads2[i], None if quals2 is None else quals2[i], adapters, P))]
        if P["pair_min_overlap"] > 0 and not mates[0][3] and not mates[1][3] and not (mates[0][2] | mates[1][2]) & F_ADAPTER:
            I = find_insert(reads1[i], reads2[i], P["pair_min_overlap"], P["pair_err_pct"])
            if I is not None:
                for x in mates:
                    if I < x[1]:
                        x[1] = I
                        x[2] |= F_OVERLAP
                        if x[0] >= x[1]:
                            x[0] = x[1] = 0
        entries += [tuple(mates[0]), tuple(mates[1])]
    start, end, flags, err, conv, info = _finish(entries, [reads1, reads2], [quals1, quals2], P, 2)
    return SimpleNamespace(seqs=(conv[0][0], conv[1][0]), offsets=(conv[0][1], conv[1][1]), quals=(conv[0][2], conv[1][2]), start=start,
                           end=end, flags=flags, err=err, info=info)
