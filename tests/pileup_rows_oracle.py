"""CPU oracle of polyhip_pileup_rows: the definition above polyhip_pileup_rows in include/polyhip.h in plain Python, column by
column, written from that comment and not from the kernels.  The parts that polyhip_pileup's and polyhip_pileup_qual's
definitions supply unchanged (err 1..7, the base classes) are tests/pileup_oracle.py's and tests/pileup_qual_oracle.py's."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import pileup_oracle as po
import pileup_qual_oracle as qo

GAP = po.GAP
MAX_Q = 93


def fold(x: int) -> int:
    return x - 32 if 97 <= x <= 122 else x


def letter(x: int, strand: int) -> int:
    return (b"acgtn" if strand else b"ACGTN")[po.base_class(x)]


def column_class(a: int, b: int) -> str:
    return "D" if a == GAP else "I" if b == GAP else "B"


def entry_tokens(A: bytes, B: bytes, ref_start: int, strand: int, mapq: int, read_start: int, Q, qual_offset: int) -> tuple:
    """-> ([(position, token bytes, quality byte)] in column order, runs dropped) of a used entry, whatever the region.
    Q: the entry's quality string as sequenced, or None"""
    n = len(A)
    cls = [column_class(A[c], B[c]) for c in range(n)]
    text_cols = [c for c in range(n) if cls[c] != "I"]                     # the columns with b != '-'
    read_cols = [c for c in range(n) if cls[c] != "D"]                     # the columns with a != '-'
    # the maximal runs of I or of D columns, each with its anchor: the last column with b != '-' before it
    runs_at, dropped, c, anchor = {}, 0, 0, None                            # anchor column -> its runs, in column order
    earlier_read = []                                                      # per column: the columns with a != '-' before it
    for k in range(n):
        earlier_read.append(earlier_read[-1] + (cls[k - 1] != "D") if k else 0)
    while c < n:
        if cls[c] in "ID":
            e = c
            while e < n and cls[e] == cls[c]:
                e += 1
            if anchor is None:
                dropped += 1
            else:
                runs_at.setdefault(anchor, []).append((cls[c], c, e))
            if cls[c] == "D":
                anchor = e - 1
            c = e
        else:
            anchor = c
            c += 1
    out, p = [], ref_start
    for c in text_cols:
        tok = bytearray()
        if c == text_cols[0]:
            tok += b"^" + bytes([min(mapq, 93) + 33])
        if cls[c] == "D":
            tok += b"*"
        elif fold(A[c]) == fold(B[c]):
            tok += b"," if strand else b"."
        else:
            tok.append(letter(A[c], strand))
        for kind, r0, r1 in runs_at.get(c, []):                            # in column order
            src = A if kind == "I" else B
            tok += (b"+" if kind == "I" else b"-") + str(r1 - r0).encode() + bytes(letter(src[k], strand) for k in range(r0, r1))
        if c == text_cols[-1]:
            tok += b"$"
        if Q is None:
            qb = ord("~")
        else:
            x = read_start + earlier_read[c]                               # the index in the oriented read
            if cls[c] == "D":
                x = min(x, read_start + len(read_cols) - 1)
            if cls[c] == "D" and not read_cols:
                qb = ord("!")
            else:
                y = len(Q) - 1 - x if strand else x
                qb = Q[y] - qual_offset + 33
        out.append((p, bytes(tok), qb, len(runs_at.get(c, []))))
        p += 1
    return out, dropped


@dataclass
class Result:
    text: bytes
    row_off: np.ndarray
    err: np.ndarray
    info: dict
    rows: dict          # position -> its row
    runs: dict          # position -> the '+' and '-' runs printed in its row


def pileup_rows(flags, mapq, ref_start, ref_end, read_start, alnA, alnB, aln_off, qual, qual_off, ref, name: bytes, order=None, region=None,
                pos_origin=0, min_mapq=0, qual_offset=33, all_positions=0) -> Result:
    """qual None: no qualities (read_start and qual_off are not looked at); mapq None reads as 255"""
    n = len(flags)
    alnA, alnB, ref, name = bytes(alnA), bytes(alnB), bytes(ref), bytes(name)
    qual = None if qual is None else bytes(qual)
    lo, hi = (0, len(ref)) if region is None else region
    assert 0 <= lo <= hi <= len(ref) and pos_origin <= lo and all_positions in (0, 1) and 0 <= qual_offset <= 162
    assert len(name) > 0 and all(0x21 <= x <= 0x7e for x in name) and (min_mapq == 0 or mapq is not None)
    ranks = list(range(n)) if order is None else [int(x) for x in order]
    assert sorted(ranks) == list(range(n))
    L = hi - lo
    err = [0] * n
    info = dict(entries=n, used=0, skipped_mapq=0, bad=0, columns=0, tokens=0, rows=0, text_bytes=0, dropped_events=0, max_row_bytes=0)
    used = [False] * n
    for i in range(n):                       # the whole entry is judged before anything of it is emitted
        if not int(flags[i]) & 1:
            continue
        if min_mapq > 0 and int(mapq[i]) < min_mapq:
            info["skipped_mapq"] += 1
            continue
        o0, o1 = int(aln_off[i]), int(aln_off[i + 1])
        assert o1 >= o0
        A, B = alnA[o0:o1], alnB[o0:o1]
        if qual is None:
            err[i] = po.entry_err(o1 - o0, A, B, int(ref_start[i]), int(ref_end[i]), ref)
        else:
            q0, q1 = int(qual_off[i]), int(qual_off[i + 1])
            assert q1 >= q0
            err[i] = qo.entry_err(o1 - o0, A, B, int(ref_start[i]), int(ref_end[i]), ref, int(read_start[i]), qual[q0:q1], qual_offset)
        if err[i]:
            info["bad"] += 1
            continue
        used[i] = True
        info["used"] += 1
        info["columns"] += o1 - o0
    at = [[] for _ in range(L)]              # per position: (token, quality byte), ascending rank
    runs_printed = {}
    for i in ranks:
        if not used[i]:
            continue
        o0, o1 = int(aln_off[i]), int(aln_off[i + 1])
        Q = None if qual is None else qual[int(qual_off[i]):int(qual_off[i + 1])]
        toks, dropped = entry_tokens(alnA[o0:o1], alnB[o0:o1], int(ref_start[i]), int(flags[i]) >> 1 & 1, 255 if mapq is None else int(mapq[i]),
                                     0 if qual is None else int(read_start[i]), Q, qual_offset)
        info["dropped_events"] += dropped
        for p, tok, qb, nruns in toks:
            if lo <= p < hi:
                at[p - lo].append((tok, qb))
                runs_printed[p] = runs_printed.get(p, 0) + nruns
    text, row_off, rows = bytearray(), [0], {}
    for j in range(L):
        p, d = lo + j, len(at[j])
        R = ref[p] if 0x21 <= ref[p] <= 0x7e else ord("N")
        head = name + b"\t" + str(p - pos_origin + 1).encode() + b"\t" + bytes([R]) + b"\t" + str(d).encode() + b"\t"
        row = b""
        if d:
            row = head + b"".join(t for t, _ in at[j]) + b"\t" + bytes(q for _, q in at[j]) + b"\n"
        elif all_positions:
            row = head + b"*\t*\n"
        if row:
            rows[p] = row
            info["rows"] += 1
            info["max_row_bytes"] = max(info["max_row_bytes"], len(row))
        info["tokens"] += d
        text += row
        row_off.append(len(text))
    info["text_bytes"] = len(text)
    return Result(bytes(text), np.array(row_off, np.uint64), np.array(err, np.uint32), info, rows, runs_printed)
