"""CPU oracle of polyhip_pileup: the definition above polyhip_pileup in include/polyhip.h in plain Python, column by column,
written from that comment and not from the kernel.  No numpy in the walk; the arrays at the end are only the shape
poly_amd.pileup.Pileup has."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MAX_COLUMNS = (1 << 28) - 1
CHANNELS = 16
GAP = ord("-")
SITE_DTYPE = np.dtype([("pos", np.uint32), ("depth", np.uint32), ("count", np.uint32), ("count_fwd", np.uint32),
                       ("kind", np.uint8), ("ref", np.uint8), ("alt", np.uint8), ("pad", np.uint8)])
_CLASS = {ord(c): k for k, pair in enumerate(("Aa", "Cc", "Gg", "Tt")) for c in pair}


def base_class(byte: int) -> int:
    """A/a C/c G/g T/t -> 0..3, every other byte 4"""
    return _CLASS.get(byte, 4)


def entry_err(ncol: int, A: bytes, B: bytes, ref_start: int, ref_end: int, ref: bytes) -> int:
    """of a mapped entry that min_mapq does not skip; A, B are read only when it has at most MAX_COLUMNS columns"""
    if ncol > MAX_COLUMNS:
        return 4
    if any(a == GAP and b == GAP for a, b in zip(A, B)):
        return 1
    if ref_start + sum(1 for b in B if b != GAP) != ref_end or ref_end > len(ref):
        return 2
    if ncol == 0:
        return 3
    p = ref_start
    for b in B:
        if b != GAP:
            if b != ref[p]:
                return 5
            p += 1
    return 0


def entry_adds(A: bytes, B: bytes, ref_start: int, strand: int) -> tuple:
    """-> ([(channel, position)], events dropped for anchor -1) of a used entry, whatever the region"""
    adds, edge = [], 0
    p, prev = ref_start, None                 # p: position of the next column with b != '-'; prev: the class before, any class
    for a, b in zip(A, B):
        c = "D" if a == GAP else "I" if b == GAP else "B"
        if c in "ID" and prev != c:           # a maximal run starts: one event at the last text position before it
            if p - 1 < 0:
                edge += 1
            else:
                adds.append((8 * strand + (6 if c == "I" else 7), p - 1))
        if c == "B":
            adds.append((8 * strand + base_class(a), p))
        elif c == "D":
            adds.append((8 * strand + 5, p))
        if c != "I":
            p += 1
        prev = c
    return adds, edge


@dataclass
class Result:
    """what poly_amd.pileup.Pileup holds, plus the info counters"""
    counts: np.ndarray
    consensus: np.ndarray
    sites: np.ndarray
    err: np.ndarray
    info: dict

    def site_list(self):
        return [tuple(int(x) for x in s) for s in self.sites.tolist()]


def call_position(col: list, ref_byte: int, p: int, min_depth: int, min_alt_count: int, min_alt_permille: int) -> tuple:
    """col: the 16 counts of one position -> (consensus byte, [site tuples])"""
    two = [col[k] + col[8 + k] for k in range(8)]
    depth = sum(two[:6])
    if depth < max(min_depth, 1):
        return ord("N"), []
    best = max(range(6), key=lambda k: (two[k], -k))
    passes = lambda cnt: cnt >= max(min_alt_count, 1) and cnt * 1000 >= min_alt_permille * depth   # noqa: E731
    out = []
    for k in range(4):
        if k != base_class(ref_byte) and passes(two[k]):
            out.append((p, depth, two[k], col[k], 1, ref_byte, b"ACGT"[k], 0))
    for kind, k in ((2, 6), (3, 7)):
        if passes(two[k]):
            out.append((p, depth, two[k], col[k], kind, ref_byte, 0, 0))
    return b"ACGTN*"[best], out


def pileup(flags, mapq, ref_start, ref_end, alnA: bytes, alnB: bytes, aln_off, ref: bytes, region=None, min_mapq=0, min_depth=0,
           min_alt_count=0, min_alt_permille=0) -> Result:
    """aln_off may claim more columns than alnA / alnB hold for an entry that is err 4 (its strings are never read)"""
    n = len(flags)
    alnA, alnB, ref = bytes(alnA), bytes(alnB), bytes(ref)
    lo, hi = (0, len(ref)) if region is None else region
    assert 0 <= lo <= hi <= len(ref) and 0 <= min_alt_permille <= 1000 and (min_mapq == 0 or mapq is not None)
    L = hi - lo
    counts = [[0] * L for _ in range(CHANNELS)]
    err = [0] * n
    info = dict(entries=n, used=0, skipped_mapq=0, bad=0, columns=0, edge_events=0, sites=0)
    for i in range(n):
        if not int(flags[i]) & 1:
            continue
        if min_mapq > 0 and int(mapq[i]) < min_mapq:
            info["skipped_mapq"] += 1
            continue
        o0, o1 = int(aln_off[i]), int(aln_off[i + 1])
        assert o1 >= o0
        A, B = alnA[o0:o1], alnB[o0:o1]
        err[i] = entry_err(o1 - o0, A, B, int(ref_start[i]), int(ref_end[i]), ref)
        if err[i]:
            info["bad"] += 1
            continue
        info["used"] += 1
        info["columns"] += o1 - o0
        adds, edge = entry_adds(A, B, int(ref_start[i]), int(flags[i]) >> 1 & 1)
        info["edge_events"] += edge
        for ch, p in adds:
            if lo <= p < hi:
                counts[ch][p - lo] += 1
    consensus, sites = bytearray(), []
    for j in range(L):
        c, s = call_position([counts[ch][j] for ch in range(CHANNELS)], ref[lo + j], lo + j, min_depth, min_alt_count, min_alt_permille)
        consensus.append(c)
        sites += s
    info["sites"] = len(sites)
    return Result(np.array(counts, np.uint32).reshape(CHANNELS, L), np.frombuffer(bytes(consensus), np.uint8),
                  np.array(sites, SITE_DTYPE), np.array(err, np.uint32), info)
