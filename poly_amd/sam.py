"""The read mapper's output as alignment records: CIGAR, NM, MD, MAPQ and the SAM FLAG word (polyhip_aln_records), and SAM text.

The reference has no mapper and no SAM writer; the definition is the comment above ``polyhip_aln_records`` in
include/polyhip.h and tests/aln_records_oracle.py restates it on the CPU.  The records are computed in HIP from the arrays a
``mapper.MapResult`` holds; ``write`` only formats them as text on the host.

``mapq`` is a stated convention -- min(60, 60 * (score - max(second, 0)) / score) -- not a calibrated quality: nobody has
measured how it relates to the probability that a placement is wrong.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .pcr import _revcomp

CIGAR_OPS = "MIDNSHP=X"
FLAG_PAIRED, FLAG_PROPER, FLAG_UNMAPPED, FLAG_MATE_UNMAPPED, FLAG_REVERSE, FLAG_MATE_REVERSE, FLAG_FIRST, FLAG_LAST = \
    0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40, 0x80
FLAG_DUPLICATE = 0x400


class _CParams(C.Structure):
    _fields_ = [("eqx", C.c_uint32), ("paired", C.c_uint32)]


class _CInfo(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("mapped", C.c_uint64), ("columns", C.c_uint64), ("cigar_ops", C.c_uint64),
                ("md_bytes", C.c_uint64), ("bad", C.c_uint64)]


def last_info() -> dict:
    """polyhip_aln_records_last_info: what the calling thread's last call did"""
    info = _CInfo()
    _lib.check(_lib.lib().polyhip_aln_records_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CInfo._fields_}


@dataclass
class AlnRecords:
    """one entry per entry of the MapResult; entry i's CIGAR is ``cigar[cigar_off[i]:cigar_off[i + 1]]`` (BAM's uint32 len <<
    4 | op), its MD ``md[md_off[i]:md_off[i + 1]]``.  ``status``: OK, or ERR_INVALID when a capacity that the caller fixed
    was short (the offsets then say what is needed and ``cigar`` / ``md`` are None)."""
    cigar_off: np.ndarray
    cigar: np.ndarray | None
    md_off: np.ndarray
    md: np.ndarray | None
    nm: np.ndarray
    mapq: np.ndarray
    sam_flag: np.ndarray
    err: np.ndarray
    status: int = 0

    def cigar_string(self, i: int) -> str:
        """entry i's CIGAR as SAM text ('' for an entry without one)"""
        ops = self.cigar[int(self.cigar_off[i]):int(self.cigar_off[i + 1])]
        return "".join(f"{int(x) >> 4}{CIGAR_OPS[int(x) & 15]}" for x in ops)

    def md_string(self, i: int) -> str:
        return self.md[int(self.md_off[i]):int(self.md_off[i + 1])].tobytes().decode("latin-1")

    last_info = staticmethod(last_info)


def _records_short() -> bool:
    """the last ERR_INVALID was the one about the capacities (everything else was delivered)"""
    return b"the records need" in _lib.lib().polyhip_last_error()


def records_packed(flags, score, second, read_start, read_end, read_len, alnA, alnB, aln_off, eqx: bool = False, paired: bool = False,
                   cigar_capacity: int | None = None, md_capacity: int | None = None) -> AlnRecords:
    """polyhip_aln_records on packed arrays.  The capacities default to a guess; a batch that needs more is run again with
    the exact sizes -- unless a capacity was given, in which case the result carries ``status`` = ERR_INVALID, the offsets,
    and no ``cigar`` / ``md``."""
    n = len(flags)
    flags, read_start, read_end = (np.ascontiguousarray(x, dtype=np.uint32) for x in (flags, read_start, read_end))
    read_len = np.ascontiguousarray(np.broadcast_to(np.asarray(read_len, dtype=np.uint32), (n,)))
    score, second = (np.ascontiguousarray(x, dtype=np.int64) for x in (score, second))
    alnA, alnB = (np.ascontiguousarray(x, dtype=np.uint8) for x in (alnA, alnB))
    aln_off = np.ascontiguousarray(aln_off, dtype=np.uint64)
    if not (len(score) == len(second) == len(read_start) == len(read_end) == n and len(aln_off) == n + 1):
        raise ValueError("records_packed: the arrays hold different numbers of entries")
    if n and int(aln_off[n]) > min(len(alnA), len(alnB)):
        raise ValueError("records_packed: the offsets reach beyond the strings")
    p = _CParams(int(bool(eqx)), int(bool(paired)))
    fixed = cigar_capacity is not None or md_capacity is not None
    ccap = int(cigar_capacity) if cigar_capacity is not None else 8 * n + 1024
    mcap = int(md_capacity) if md_capacity is not None else 32 * n + 4096
    coff, moff = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    nm, sf, err, mapq = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    cigar = md = None
    rc = _lib.OK
    for _ in range(2):
        cigar, md = np.zeros(max(ccap, 1), np.uint32), np.zeros(max(mcap, 1), np.uint8)
        rc = _lib.lib().polyhip_aln_records(C.byref(p), n, flags.ctypes.data, score.ctypes.data, second.ctypes.data,
                                            read_start.ctypes.data, read_end.ctypes.data, read_len.ctypes.data, alnA.ctypes.data,
                                            alnB.ctypes.data, aln_off.ctypes.data, coff.ctypes.data, cigar.ctypes.data, ccap,
                                            moff.ctypes.data, md.ctypes.data, mcap, nm.ctypes.data, mapq.ctypes.data, sf.ctypes.data,
                                            err.ctypes.data)
        if rc == _lib.ERR_INVALID and _records_short():     # the offsets say what the records need
            if fixed:
                return AlnRecords(coff, None, moff, None, nm, mapq, sf, err, int(rc))
            ccap, mcap = int(coff[n]), int(moff[n])
            continue
        _lib.check(rc)
        break
    return AlnRecords(coff, cigar[:int(coff[n])], moff, md[:int(moff[n])], nm, mapq, sf, err, int(rc))


def records(result, read_len, eqx: bool = False, paired: bool = False) -> AlnRecords:
    """The records of a ``mapper.MapResult`` that holds its strings.  ``read_len``: the length of every read (one number, or
    one per entry; for pairs in the result's order 2i, 2i + 1).  ``eqx``: '=' and 'X' instead of 'M'.  ``paired``: the
    entries are mates (2i, 2i + 1), as ``mapper.map_pairs_packed`` returns them."""
    if result.alignA is None or result.alignB is None:
        raise ValueError("sam.records: the MapResult holds no strings")
    a, b = b"".join(result.alignA), b"".join(result.alignB)
    off = np.zeros(len(result.alignA) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in result.alignA], dtype=np.uint64)
    return records_packed(result.flags, result.score, result.second, result.read_start, result.read_end, read_len,
                          np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8), off, eqx, paired)


def _text(x) -> str:
    return x if isinstance(x, str) else bytes(x).decode("latin-1")


def _so(order) -> str:
    return "unsorted" if order is None else "coordinate"


def _entries(n: int, order):
    """the entries in the order they are written: the result's, or ``order`` (a permutation of all of them)"""
    if order is None:
        return range(n)
    order = [int(i) for i in order]
    if sorted(order) != list(range(n)):
        raise ValueError("sam.write: order is not a permutation of the entries")
    return order


def write(fh, ref_name: str, ref_len: int, names, reads, quals, result, records: AlnRecords, paired: bool = False, order=None,
          dup=None) -> None:
    """SAM text on ``fh`` (a text file): an @HD and an @SQ line, then one line of 11 fields per entry, with NM:i, MD:Z and AS:i
    on the live ones.  ``names``, ``reads`` and ``quals`` (or None: '*') have one item per entry, ``str`` or ``bytes``; for
    pairs that is the result's order 2i, 2i + 1, and ``records`` was made with ``paired=True``.  One reference only: RNAME is
    ``ref_name``.  A live entry on the reverse strand is written as the mapper placed it: SEQ is the reverse complement
    (bytes the complement table lacks become N), QUAL is reversed.  An entry that is not live is written unmapped; with
    ``paired`` it takes RNAME / POS of a live mate.  RNEXT is '=', PNEXT the mate's POS and TLEN +/- ``result.tlen`` (plus on
    the mate with the smaller ref_start, ties to mate 1) when the mate is live; TLEN is 0 unless both are.  ``order``: the
    permutation of ``dedup.coord_order``; the header then says SO:coordinate and the lines go out in that order.  ``dup``:
    ``dedup.Duplicates.dup``; 0x400 is set in the FLAG of its entries."""
    n = len(records.sam_flag)
    fh.write(f"@HD\tVN:1.6\tSO:{_so(order)}\n@SQ\tSN:{ref_name}\tLN:{int(ref_len)}\n")
    live = (records.sam_flag & FLAG_UNMAPPED) == 0
    for i in _entries(n, order):
        flag = int(records.sam_flag[i]) | (FLAG_DUPLICATE if dup is not None and dup[i] else 0)
        rname, pos, mapq, cigar = "*", 0, 0, "*"
        if live[i]:
            rname, pos, mapq, cigar = ref_name, int(result.ref_start[i]) + 1, int(records.mapq[i]), records.cigar_string(i)
        rnext, pnext, tlen = "*", 0, 0
        if paired and live[i ^ 1]:
            m = i ^ 1
            rnext, pnext = "=", int(result.ref_start[m]) + 1
            if live[i]:
                first = i if (int(result.ref_start[i]), i) <= (int(result.ref_start[m]), m) else m
                tlen = int(result.tlen[i >> 1]) * (1 if first == i else -1)
            else:
                rname, pos = ref_name, pnext
        seq = reads[i] if isinstance(reads[i], bytes) else _text(reads[i]).encode("latin-1")
        qual = None if quals is None else _text(quals[i])
        if live[i] and flag & FLAG_REVERSE:
            seq = _revcomp(seq).replace(b"\x00", b"N")
            qual = None if qual is None else qual[::-1]
        fields = [_text(names[i]), str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen),
                  _text(seq) or "*", qual or "*"]
        if live[i]:
            fields += [f"NM:i:{int(records.nm[i])}", f"MD:Z:{records.md_string(i)}", f"AS:i:{int(result.score[i])}"]
        fh.write("\t".join(fields) + "\n")


def write_refs(fh, refs, names, reads, quals, result, records: AlnRecords, paired: bool = False, order=None, dup=None) -> None:
    """``write`` for the result of ``mapper.map_reads_refs_packed`` / ``map_pairs_refs_packed`` on the ``refs.RefSet`` it was
    mapped to: one @SQ line per contig, in the set's order; RNAME is the name of ``result.rid[i]``'s contig and POS a position
    in it.  With ``paired``: RNEXT is '=' when the live mate is on the same contig (an entry that is not live takes its live
    mate's RNAME and POS, so '=' too), else the mate's contig name; TLEN is 0 unless both mates are live on one contig.
    Everything else is ``write``'s, ``order`` and ``dup`` included."""
    n = len(records.sam_flag)
    fh.write(f"@HD\tVN:1.6\tSO:{_so(order)}\n")
    for name, length in zip(refs.names, refs.lengths):
        fh.write(f"@SQ\tSN:{name}\tLN:{int(length)}\n")
    live = (records.sam_flag & FLAG_UNMAPPED) == 0
    for i in _entries(n, order):
        flag = int(records.sam_flag[i]) | (FLAG_DUPLICATE if dup is not None and dup[i] else 0)
        rname, pos, mapq, cigar = "*", 0, 0, "*"
        if live[i]:
            rname, pos, mapq, cigar = refs.names[int(result.rid[i])], int(result.ref_start[i]) + 1, int(records.mapq[i]), \
                records.cigar_string(i)
        rnext, pnext, tlen = "*", 0, 0
        if paired and live[i ^ 1]:
            m = i ^ 1
            mate_name = refs.names[int(result.rid[m])]
            pnext = int(result.ref_start[m]) + 1
            if live[i]:
                rnext = "=" if result.rid[i] == result.rid[m] else mate_name
                if result.rid[i] == result.rid[m]:
                    first = i if (int(result.ref_start[i]), i) <= (int(result.ref_start[m]), m) else m
                    tlen = int(result.tlen[i >> 1]) * (1 if first == i else -1)
            else:
                rname, pos, rnext = mate_name, pnext, "="
        seq = reads[i] if isinstance(reads[i], bytes) else _text(reads[i]).encode("latin-1")
        qual = None if quals is None else _text(quals[i])
        if live[i] and flag & FLAG_REVERSE:
            seq = _revcomp(seq).replace(b"\x00", b"N")
            qual = None if qual is None else qual[::-1]
        fields = [_text(names[i]), str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen),
                  _text(seq) or "*", qual or "*"]
        if live[i]:
            fields += [f"NM:i:{int(records.nm[i])}", f"MD:Z:{records.md_string(i)}", f"AS:i:{int(result.score[i])}"]
        fh.write("\t".join(fields) + "\n")
