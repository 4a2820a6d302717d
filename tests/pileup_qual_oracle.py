"""CPU oracle of polyhip_pileup_qual: the definition above polyhip_pileup_qual in include/polyhip.h in plain Python, column by
column, written from that comment and not from the kernel.  The parts that polyhip_pileup's definition supplies unchanged
(err 1..5, the base classes, the consensus and site rules) are tests/pileup_oracle.py's."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import pileup_oracle as po

QSUM_PLANES = 8
MAX_Q = 93
GAP = po.GAP


def entry_err(ncol: int, A: bytes, B: bytes, ref_start: int, ref_end: int, ref: bytes, read_start: int, Q: bytes, qual_offset: int) -> int:
    """of a mapped entry that min_mapq does not skip: polyhip_pileup's err first, then 6, then 7"""
    e = po.entry_err(ncol, A, B, ref_start, ref_end, ref)
    if e:
        return e
    if read_start + sum(1 for a in A if a != GAP) > len(Q):
        return 6
    if any(not qual_offset <= x <= qual_offset + MAX_Q for x in Q):       # the whole string, clipped parts included
        return 7
    return 0


def entry_adds(A: bytes, B: bytes, ref_start: int, strand: int, read_start: int, Q: bytes, qual_offset: int, min_base_qual: int) -> tuple:
    """-> ([(channel, position)], [(qsum plane, position, quality)], events dropped for anchor -1, base columns filtered) of a
    used entry, whatever the region"""
    adds, qadds, edge, filtered = [], [], 0, 0
    p, x, prev = ref_start, read_start, None      # p: text position of the next column with b != '-'; x: index in q of the next with a != '-'
    m = len(Q)
    for a, b in zip(A, B):
        c = "D" if a == GAP else "I" if b == GAP else "B"
        if c in "ID" and prev != c:
            if p - 1 < 0:
                edge += 1
            else:
                adds.append((8 * strand + (6 if c == "I" else 7), p - 1))
        if c == "B":
            quality = Q[m - 1 - x if strand else x] - qual_offset
            if quality >= min_base_qual:
                k = po.base_class(a)
                adds.append((8 * strand + k, p))
                if k < 4:
                    qadds.append((4 * strand + k, p, quality))
            else:
                filtered += 1
        elif c == "D":                            # not filtered: a deleted base has no quality of its own
            adds.append((8 * strand + 5, p))
        if c != "I":
            p += 1
        if c != "D":
            x += 1
        prev = c
    return adds, qadds, edge, filtered


@dataclass
class Result(po.Result):
    qsum: np.ndarray = None


def pileup_qual(flags, mapq, ref_start, ref_end, read_start, alnA: bytes, alnB: bytes, aln_off, qual: bytes, qual_off, ref: bytes,
                region=None, min_mapq=0, min_depth=0, min_alt_count=0, min_alt_permille=0, min_base_qual=0, qual_offset=33) -> Result:
    n = len(flags)
    alnA, alnB, qual, ref = bytes(alnA), bytes(alnB), bytes(qual), bytes(ref)
    lo, hi = (0, len(ref)) if region is None else region
    assert 0 <= lo <= hi <= len(ref) and 0 <= min_alt_permille <= 1000 and (min_mapq == 0 or mapq is not None)
    assert 0 <= min_base_qual <= MAX_Q and 0 <= qual_offset <= 255 - MAX_Q and n * MAX_Q < 1 << 32
    L = hi - lo
    counts = [[0] * L for _ in range(po.CHANNELS)]
    qsum = [[0] * L for _ in range(QSUM_PLANES)]
    err = [0] * n
    info = dict(entries=n, used=0, skipped_mapq=0, bad=0, columns=0, edge_events=0, sites=0, filtered_bases=0)
    for i in range(n):
        if not int(flags[i]) & 1:
            continue
        if min_mapq > 0 and int(mapq[i]) < min_mapq:
            info["skipped_mapq"] += 1
            continue
        o0, o1 = int(aln_off[i]), int(aln_off[i + 1])
        q0, q1 = int(qual_off[i]), int(qual_off[i + 1])
        assert o1 >= o0 and q1 >= q0
        A, B, Q = alnA[o0:o1], alnB[o0:o1], qual[q0:q1]
        err[i] = entry_err(o1 - o0, A, B, int(ref_start[i]), int(ref_end[i]), ref, int(read_start[i]), Q, qual_offset)
        if err[i]:
            info["bad"] += 1
            continue
        info["used"] += 1
        info["columns"] += o1 - o0
        adds, qadds, edge, filtered = entry_adds(A, B, int(ref_start[i]), int(flags[i]) >> 1 & 1, int(read_start[i]), Q, qual_offset,
                                                 min_base_qual)
        info["edge_events"] += edge
        info["filtered_bases"] += filtered
        for ch, p in adds:
            if lo <= p < hi:
                counts[ch][p - lo] += 1
        for pl, p, quality in qadds:
            if lo <= p < hi:
                qsum[pl][p - lo] += quality
    consensus, sites = bytearray(), []
    for j in range(L):
        c, s = po.call_position([counts[ch][j] for ch in range(po.CHANNELS)], ref[lo + j], lo + j, min_depth, min_alt_count,
                                min_alt_permille)
        consensus.append(c)
        sites += s
    info["sites"] = len(sites)
    return Result(np.array(counts, np.uint32).reshape(po.CHANNELS, L), np.frombuffer(bytes(consensus), np.uint8),
                  np.array(sites, po.SITE_DTYPE), np.array(err, np.uint32), info, np.array(qsum, np.uint32).reshape(QSUM_PLANES, L))
