"""CPU oracle of polyhip_aln_records and of sam.write's lines: the definition above polyhip_aln_records in include/polyhip.h and
the docstring of poly_amd.sam.write in plain Python, column by column, written from the definition and not from the kernel.
No numpy in the walk; the arrays at the end are only the shape poly_amd.sam.AlnRecords has."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

MAX_COLUMNS = (1 << 28) - 1
OPS = {"M": 0, "I": 1, "D": 2, "S": 4, "=": 7, "X": 8}
OP_CHARS = "MIDNSHP=X"
GAP = ord("-")


@dataclass
class Entry:
    err: int = 0
    live: bool = False
    cigar: list = field(default_factory=list)   # uint32 values, len << 4 | op
    md: bytes = b""
    nm: int = 0
    mapq: int = 0
    columns: int = 0


def column_class(a: int, b: int) -> str:
    if a == GAP and b == GAP:
        return "?"
    if a == GAP:
        return "D"
    if b == GAP:
        return "I"
    return "=" if a == b else "X"


def entry_err(mapped: bool, ncol: int, A: bytes, B: bytes, read_start: int, read_end: int, read_len: int) -> int:
    """A, B are read only when the entry is mapped and has at most MAX_COLUMNS columns"""
    if not mapped:
        return 0
    if ncol > MAX_COLUMNS:
        return 4
    if any(column_class(a, b) == "?" for a, b in zip(A, B)):
        return 1
    if read_start > read_end or read_end > read_len or sum(1 for a in A if a != GAP) != read_end - read_start:
        return 2
    if ncol == 0:
        return 3
    return 0


def cigar_of(A: bytes, B: bytes, read_start: int, read_end: int, read_len: int, eqx: bool) -> list:
    runs = []                                   # [class, length]
    for a, b in zip(A, B):
        c = column_class(a, b)
        if not eqx and c in "=X":
            c = "M"
        if runs and runs[-1][0] == c:
            runs[-1][1] += 1
        else:
            runs.append([c, 1])
    out = [(read_start, "S")] if read_start > 0 else []
    out += [(n, c) for c, n in runs]
    if read_len - read_end > 0:
        out.append((read_len - read_end, "S"))
    return [((n << 4) | OPS[c]) & 0xFFFFFFFF for n, c in out]


def md_of(A: bytes, B: bytes) -> bytes:
    out, k, prev = bytearray(), 0, None        # prev: the class of the column before, I columns included
    for a, b in zip(A, B):
        c = column_class(a, b)
        if c == "=":
            k += 1
        elif c == "X":
            out += b"%d" % k + bytes([b])
            k = 0
        elif c == "D":
            if prev != "D":
                out += b"%d" % k + b"^"
                k = 0
            out.append(b)
        prev = c
    return bytes(out + b"%d" % k)


def mapq_of(score: int, second: int) -> int:
    s, t = score, max(second, 0)
    return 0 if t >= s else min(60, 60 * (s - t) // s)


def one(mapped: bool, ncol: int, A: bytes, B: bytes, read_start: int, read_end: int, read_len: int, score: int, second: int,
        eqx: bool) -> Entry:
    e = Entry(err=entry_err(mapped, ncol, A, B, read_start, read_end, read_len))
    e.live = bool(mapped) and e.err == 0
    if e.live:
        e.cigar = cigar_of(A, B, read_start, read_end, read_len, eqx)
        e.md = md_of(A, B)
        e.nm = sum(1 for a, b in zip(A, B) if column_class(a, b) in "XID")
        e.mapq = mapq_of(score, second)
        e.columns = ncol
    return e


def sam_flags(flags, live, paired: bool) -> list:
    out = []
    for i, f in enumerate(flags):
        v = 0x4 if not live[i] else (0x10 if f & 2 else 0)
        if paired:
            m = i ^ 1
            v |= 0x1 | (0x80 if i & 1 else 0x40)
            if f & 4 and live[i] and live[m]:
                v |= 0x2
            if not live[m]:
                v |= 0x8
            elif flags[m] & 2:
                v |= 0x20
        out.append(v)
    return out


@dataclass
class Records:
    """what poly_amd.sam.AlnRecords holds, plus the info counters"""
    cigar_off: np.ndarray
    cigar: np.ndarray
    md_off: np.ndarray
    md: np.ndarray
    nm: np.ndarray
    mapq: np.ndarray
    sam_flag: np.ndarray
    err: np.ndarray
    info: dict
    entries: list

    def cigar_string(self, i):
        return "".join(f"{x >> 4}{OP_CHARS[x & 15]}" for x in self.entries[i].cigar)

    def md_string(self, i):
        return self.entries[i].md.decode("latin-1")


def records(flags, score, second, read_start, read_end, read_len, alnA: bytes, alnB: bytes, aln_off, eqx=False, paired=False) -> Records:
    """aln_off may claim more columns than alnA / alnB hold for an entry that is err 4 (its strings are never read)"""
    n = len(flags)
    assert not paired or n % 2 == 0
    alnA, alnB = bytes(alnA), bytes(alnB)
    ents = []
    for i in range(n):
        o0, o1 = int(aln_off[i]), int(aln_off[i + 1])
        assert o1 >= o0
        ents.append(one(bool(flags[i] & 1), o1 - o0, alnA[o0:o1], alnB[o0:o1], int(read_start[i]), int(read_end[i]), int(read_len[i]),
                        int(score[i]), int(second[i]), eqx))
    coff, moff = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    coff[1:] = np.cumsum([len(e.cigar) for e in ents], dtype=np.uint64)
    moff[1:] = np.cumsum([len(e.md) for e in ents], dtype=np.uint64)
    info = dict(entries=n, mapped=sum(e.live for e in ents), columns=sum(e.columns for e in ents), cigar_ops=int(coff[n]),
                md_bytes=int(moff[n]), bad=sum(e.err != 0 for e in ents))
    return Records(coff, np.array([x for e in ents for x in e.cigar], np.uint32), moff,
                   np.frombuffer(b"".join(e.md for e in ents), np.uint8), np.array([e.nm for e in ents], np.uint32),
                   np.array([e.mapq for e in ents], np.uint8),
                   np.array(sam_flags([int(f) for f in flags], [e.live for e in ents], paired), np.uint32),
                   np.array([e.err for e in ents], np.uint32), info, ents)


# ---- the round trip: q, CIGAR and MD give back the text the entry was aligned to -------------------------------------------
def parse_md(md: bytes) -> list:
    """-> tokens: int (matches), ('X', byte), ('D', bytes)"""
    out, i = [], 0
    while i < len(md):
        if 48 <= md[i] <= 57:
            j = i
            while j < len(md) and 48 <= md[j] <= 57:
                j += 1
            out.append(int(md[i:j]))
            i = j
        elif md[i] == ord("^"):
            j = i + 1
            while j < len(md) and not 48 <= md[j] <= 57:
                j += 1
            out.append(("D", md[i + 1:j]))
            i = j
        else:
            out.append(("X", md[i]))
            i += 1
    return out


def rebuild_text(q: bytes, cigar, md: bytes):
    """the non-gap bytes of alnB from the oriented read q, a CIGAR (uint32 values) and an MD string -> (text, read bases
    consumed, soft clips included).  Knows nothing of column classes: it reads the two strings as samtools would."""
    toks = parse_md(md)
    assert toks and isinstance(toks[0], int) and isinstance(toks[-1], int), "an MD starts and ends with a number"
    ti, left = 0, toks[0]                       # position in toks; matches left of the current number

    def next_tok():
        nonlocal ti, left
        ti += 1
        left = toks[ti] if isinstance(toks[ti], int) else 0

    out, qi = bytearray(), 0
    for x in cigar:
        n, op = int(x) >> 4, OP_CHARS[int(x) & 15]
        if op in "SI":
            qi += n
        elif op == "D":
            assert left == 0
            next_tok()
            kind, bs = toks[ti]
            assert kind == "D" and len(bs) == n, "a deletion of the CIGAR is one ^ run of the MD"
            out += bs
            next_tok()
        else:
            assert op in "M=X"
            while n:
                if left:
                    step = min(left, n)
                    assert op != "X"
                    out += q[qi:qi + step]
                    qi, n, left = qi + step, n - step, left - step
                else:
                    next_tok()
                    if isinstance(toks[ti], int):
                        continue
                    kind, byte = toks[ti]
                    assert kind == "X" and op != "=" and byte != q[qi], "a mismatch names a byte that differs from the read's"
                    out.append(byte)
                    qi, n = qi + 1, n - 1
                    next_tok()
    assert left == 0 and ti == len(toks) - 1, "the MD is longer than the CIGAR"
    return bytes(out), qi


# ---- sam.write's lines ---------------------------------------------------------------------------------------------------------
_COMP = bytes.maketrans(b"ABCDGHKMNRSTVWYabcdghkmnrstvwy", b"TVGHCDMKNYSABWRtvghcdmknysabwr")
_KNOWN = set(b"ABCDGHKMNRSTVWYabcdghkmnrstvwy")


def sam_lines(ref_name, ref_len, names, reads, quals, ref_start, score, tlen, rec: Records, paired=False) -> list:
    lines = ["@HD\tVN:1.6\tSO:unsorted", f"@SQ\tSN:{ref_name}\tLN:{ref_len}"]
    live = [e.live for e in rec.entries]
    for i, e in enumerate(rec.entries):
        flag = int(rec.sam_flag[i])
        rname, pos, mapq, cigar = (ref_name, int(ref_start[i]) + 1, e.mapq, rec.cigar_string(i)) if e.live else ("*", 0, 0, "*")
        rnext, pnext, t = "*", 0, 0
        if paired and live[i ^ 1]:
            m = i ^ 1
            rnext, pnext = "=", int(ref_start[m]) + 1
            if e.live:
                smaller = int(ref_start[i]) < int(ref_start[m]) or (int(ref_start[i]) == int(ref_start[m]) and i % 2 == 0)
                t = int(tlen[i // 2]) if smaller else -int(tlen[i // 2])
            else:
                rname, pos = ref_name, pnext
        seq, qual = bytes(reads[i]), None if quals is None else str(quals[i])
        if e.live and flag & 0x10:
            seq = bytes(c.to_bytes(1, "little").translate(_COMP)[0] if c in _KNOWN else ord("N") for c in reversed(seq))
            qual = None if qual is None else qual[::-1]
        f = [str(names[i]), str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(t), seq.decode("latin-1") or "*",
             qual or "*"]
        if e.live:
            f += [f"NM:i:{e.nm}", f"MD:Z:{e.md.decode('latin-1')}", f"AS:i:{int(score[i])}"]
        lines.append("\t".join(f))
    return lines
