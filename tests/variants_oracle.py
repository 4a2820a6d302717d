"""CPU oracle of polyhip_call_variants: the definition above polyhip_call_variants in include/polyhip.h in plain Python, column
by column, written from that comment and not from the kernels.  The planes (err, used, the depth, the SNV counts) are those of
tests/pileup_oracle.py without qualities and of tests/pileup_qual_oracle.py with them."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import pileup_oracle as po
import pileup_qual_oracle as qo

GAP = po.GAP
MAX_INDEL = 255
KIND_SNV, KIND_INS, KIND_DEL = 1, 2, 3
VARIANT_DTYPE = np.dtype([("allele_off", np.uint64), ("pos", np.uint32), ("depth", np.uint32), ("count", np.uint32),
                          ("count_fwd", np.uint32), ("ref_count", np.uint32), ("qsum", np.uint32), ("allele_len", np.uint32),
                          ("kind", np.uint8), ("ref", np.uint8), ("alt", np.uint8), ("gt", np.uint8)])
INFO_FIELDS = ("entries", "used", "skipped_mapq", "bad", "columns", "edge_events", "sites", "filtered_bases", "events", "long_events",
               "open_events", "shifted_events", "alleles", "allele_bytes")


def fold(x: int) -> int:
    return x - 32 if 97 <= x <= 122 else x


def entry_runs(A: bytes, B: bytes, ref_start: int) -> list:
    """-> [(c0, l, kind, p0)]: the maximal runs of I and of D columns of an entry, anchored as the pileup's channels 6 and 7"""
    out, p, prev = [], ref_start, None
    for c, (a, b) in enumerate(zip(A, B)):
        cls = "D" if a == GAP else "I" if b == GAP else "B"
        if cls in "ID":
            if prev != cls:
                out.append([c, 0, KIND_INS if cls == "I" else KIND_DEL, p - 1])
            out[-1][1] += 1
        if cls != "I":
            p += 1
        prev = cls
    return [tuple(r) for r in out]


def shift(A: bytes, B: bytes, c0: int, l: int, kind: int) -> int:
    """k: the consecutive steps t = 0, 1, ... that succeed"""
    x = A if kind == KIND_INS else B
    k = 0
    while True:
        c = c0 - 1 - k
        if c < 0:
            return k
        a, b = A[c], B[c]
        if a == GAP or b == GAP or fold(a) != fold(b):
            return k
        if fold(x[c]) != fold(x[c + l]):
            return k
        k += 1


def entry_events(A: bytes, B: bytes, ref_start: int, left_align: bool, max_indel: int) -> tuple:
    """-> ([(anchor, kind, l, allele bytes, k)] kept events whatever the region, long, open, edge)"""
    kept, n_long, n_open, n_edge = [], 0, 0, 0
    for c0, l, kind, p0 in entry_runs(A, B, ref_start):
        if l > max_indel:
            n_long += 1
            continue
        k = 0
        if left_align:
            k = shift(A, B, c0, l, kind)
            if k == c0:
                n_open += 1
                continue
        if p0 - k == -1:
            n_edge += 1
            continue
        assert p0 - k >= 0
        allele = bytes(fold(x) for x in A[c0 - k:c0 - k + l]) if kind == KIND_INS else b""
        kept.append((p0 - k, kind, l, allele, k))
    return kept, n_long, n_open, n_edge


@dataclass
class Result:
    records: np.ndarray
    alleles: np.ndarray
    err: np.ndarray
    info: dict
    planes: object          # the pileup oracle's Result the call was made from
    groups: dict            # (anchor, kind, l, allele bytes) -> [count, count_fwd], every allele of the region before the thresholds

    def record_list(self):
        return [tuple(int(x) for x in r) for r in self.records.tolist()]

    def allele(self, i: int) -> bytes:
        r = self.records[i]
        return self.alleles[int(r["allele_off"]):int(r["allele_off"]) + int(r["allele_len"])].tobytes() if r["kind"] == KIND_INS else b""


def call_variants(flags, mapq, ref_start, ref_end, read_start, alnA: bytes, alnB: bytes, aln_off, qual, qual_off, ref: bytes, region=None,
                  min_mapq=0, min_depth=0, min_alt_count=0, min_alt_permille=0, min_base_qual=0, qual_offset=33, left_align=1,
                  hom_permille=800, max_indel=0) -> Result:
    """qual None: without qualities (read_start and qual_off are not looked at)"""
    n = len(flags)
    alnA, alnB, ref = bytes(alnA), bytes(alnB), bytes(ref)
    assert 0 <= hom_permille <= 1000 and 0 <= max_indel <= MAX_INDEL
    max_indel = max_indel or MAX_INDEL
    if qual is None:
        assert min_base_qual == 0 and n < 1 << 32
        planes = po.pileup(flags, mapq, ref_start, ref_end, alnA, alnB, aln_off, ref, region, min_mapq, min_depth, min_alt_count,
                           min_alt_permille)
        qsum = None
    else:
        planes = qo.pileup_qual(flags, mapq, ref_start, ref_end, read_start, alnA, alnB, aln_off, bytes(qual), qual_off, ref, region, min_mapq,
                                min_depth, min_alt_count, min_alt_permille, min_base_qual, qual_offset)
        qsum = planes.qsum
    lo, hi = (0, len(ref)) if region is None else region
    L = hi - lo
    counts = planes.counts
    info = {f: planes.info.get(f, 0) for f in INFO_FIELDS}
    info["edge_events"] = 0
    groups = {}
    for i in range(n):
        if not int(flags[i]) & 1 or (min_mapq > 0 and int(mapq[i]) < min_mapq) or planes.err[i]:
            continue
        o0, o1 = int(aln_off[i]), int(aln_off[i + 1])
        kept, n_long, n_open, n_edge = entry_events(alnA[o0:o1], alnB[o0:o1], int(ref_start[i]), bool(left_align), max_indel)
        info["long_events"] += n_long
        info["open_events"] += n_open
        info["edge_events"] += n_edge
        info["events"] += len(kept)
        for anchor, kind, l, allele, k in kept:
            info["shifted_events"] += k > 0
            if lo <= anchor < hi:
                g = groups.setdefault((anchor, kind, l, allele), [0, 0])
                g[0] += 1
                g[1] += not int(flags[i]) >> 1 & 1
    info["alleles"] = len(groups)
    site_events = {}
    for (anchor, kind, l, allele), (cnt, _) in groups.items():
        site_events[anchor, kind] = site_events.get((anchor, kind), 0) + cnt
    at = {}
    for key in groups:
        at.setdefault(key[0], []).append(key)
    records, pool = [], bytearray()
    for j in range(L):
        p = lo + j
        col = [int(counts[ch][j]) for ch in range(po.CHANNELS)]
        two = [col[k] + col[8 + k] for k in range(8)]
        depth = sum(two[:6])
        if depth < max(min_depth, 1):
            continue
        passes = lambda cnt: cnt >= max(min_alt_count, 1) and cnt * 1000 >= min_alt_permille * depth    # noqa: E731
        gt = lambda cnt: 2 if cnt * 1000 >= hom_permille * depth else 1                                    # noqa: E731
        rc = po.base_class(ref[p])
        for k in range(4):
            if k != rc and passes(two[k]):
                q = 0 if qsum is None else int(qsum[k][j]) + int(qsum[4 + k][j])
                records.append((0, p, depth, two[k], col[k], two[rc] if rc < 4 else 0, q, 1, KIND_SNV, ref[p], b"ACGT"[k], gt(two[k])))
        for key in sorted(at.get(p, ()), key=lambda g: (g[1], g[2], g[3])):      # insertions by (length, bytes), then deletions by length
            _, kind, l, allele = key
            cnt, fwd = groups[key]
            if not passes(cnt):
                continue
            off = 0
            if kind == KIND_INS:
                off = len(pool)
                pool += allele
            records.append((off, p, depth, cnt, fwd, depth - min(depth, site_events[p, kind]), 0, l, kind, ref[p], 0, gt(cnt)))
    info["sites"] = len(records)
    info["allele_bytes"] = len(pool)
    return Result(np.array(records, VARIANT_DTYPE), np.frombuffer(bytes(pool), np.uint8), planes.err.copy(), info, planes, groups)
