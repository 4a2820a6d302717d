"""polyhip_mark_duplicates and polyhip_coord_order in plain Python: a direct restatement of the comment above the two calls in
include/polyhip.h, with dicts and ``sorted``.  It shares no code with the product (poly_amd/csrc/dedup.hip sorts packed words
with a radix sort and never builds a dict)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

INFO_FIELDS = ("entries", "candidates", "bad", "pairs", "fragments", "dup_pairs", "dup_fragments", "pair_sets", "end_sets")


@dataclass
class Marked:
    dup: np.ndarray
    rep: np.ndarray
    weight: np.ndarray
    err: np.ndarray
    info: dict


def entry_err(mapped, ref_start, ref_end, read_start, read_end, read_len, q, min_weight_qual, qual_offset):
    """(err, the mode-1 weight); q: the entry's quality string, None with weight_mode 0"""
    if not mapped:
        return 0, 0
    if read_start > read_end or read_end > read_len or ref_start > ref_end:
        return 2, 0
    if q is None:
        return 0, 0
    if len(q) != read_len:
        return 6, 0
    if any(b < qual_offset or b > qual_offset + 93 for b in q):
        return 7, 0
    return 0, sum(b - qual_offset for b in q if b - qual_offset >= min_weight_qual)


def end_key(rid, strand, ref_start, ref_end, read_start, read_end, read_len):
    """E = (rid, u, s): u is the text position of the 5' end with the clips added back"""
    u = ref_end - 1 + (read_len - read_end) if strand else ref_start - read_start
    return (rid, u, strand)


def mark(flags, ref_start, ref_end, read_start, read_end, read_len, rid=None, paired=False, weight=None, qual=None, qual_off=None,
         min_weight_qual=15, qual_offset=33) -> Marked:
    n = len(flags)
    I = lambda x: [int(v) for v in x]                                       # noqa: E731,E741
    flags, ref_start, ref_end, read_start, read_end = I(flags), I(ref_start), I(ref_end), I(read_start), I(read_end)
    read_len = [int(read_len)] * n if np.ndim(read_len) == 0 else I(read_len)
    rid = [0] * n if rid is None else I(rid)
    mode1 = qual_off is not None
    if mode1:
        qual, qual_off = bytes(bytearray(qual)) if qual is not None else b"", I(qual_off)
    assert not paired or n % 2 == 0
    err, w, cand, E = [0] * n, [0] * n, [False] * n, [None] * n
    for i in range(n):
        q = qual[qual_off[i]:qual_off[i + 1]] if mode1 else None
        err[i], wq = entry_err(flags[i] & 1, ref_start[i], ref_end[i], read_start[i], read_end[i], read_len[i], q, min_weight_qual,
                               qual_offset)
        cand[i] = bool(flags[i] & 1) and err[i] == 0
        if cand[i]:
            w[i] = wq if mode1 else 0 if weight is None else int(weight[i])
            E[i] = end_key(rid[i], flags[i] >> 1 & 1, ref_start[i], ref_end[i], read_start[i], read_end[i], read_len[i])
    dup, rep = [0] * n, list(range(n))
    is_pair = [paired and cand[i] and cand[i ^ 1] for i in range(n)]
    fragment = [cand[i] and not is_pair[i] for i in range(n)]
    # pair sets
    pair_sets = {}
    lo_of = {}
    for p in range(n // 2 if paired else 0):
        if is_pair[2 * p]:
            lo, hi = sorted((2 * p, 2 * p + 1), key=lambda i: (E[i], i))
            lo_of[p] = (lo, hi)
            pair_sets.setdefault((E[lo], E[hi]), []).append(p)
    dup_pairs = 0
    for members in pair_sets.values():
        best = sorted(members, key=lambda p: (-(w[2 * p] + w[2 * p + 1]), p))[0]
        for p in members:
            if p != best:
                dup_pairs += 1
                for mine, theirs in zip(lo_of[p], lo_of[best]):
                    dup[mine], rep[mine] = 1, theirs
    # end sets
    end_sets = {}
    for i in range(n):
        if cand[i]:
            end_sets.setdefault(E[i], []).append(i)
    dup_fragments = 0
    for members in end_sets.values():
        head = sorted(members, key=lambda i: (fragment[i], -w[i], i))[0]
        for i in members:
            if fragment[i] and i != head:
                dup_fragments += 1
                dup[i], rep[i] = 1, head
    info = dict(entries=n, candidates=sum(cand), bad=sum(1 for e in err if e), pairs=sum(is_pair) // 2, fragments=sum(fragment),
                dup_pairs=dup_pairs, dup_fragments=dup_fragments, pair_sets=len(pair_sets), end_sets=len(end_sets))
    return Marked(np.array(dup, np.uint8), np.array(rep, np.uint32), np.array(w, np.uint32), np.array(err, np.uint32), info)


def coord_order(sam_flag, ref_start, rid=None, paired=False) -> np.ndarray:
    n = len(sam_flag)
    rid = [0] * n if rid is None else rid
    live = [not int(sam_flag[i]) & 4 for i in range(n)]

    def place(i):
        at = i if live[i] else i ^ 1 if paired and live[i ^ 1] else None
        return (1, 0, 0, i) if at is None else (0, int(rid[at]), int(ref_start[at]), i)

    return np.array(sorted(range(n), key=place), np.uint32)
