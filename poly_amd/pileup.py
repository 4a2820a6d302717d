"""Pileup of the read mapper's output: per-position counts, a consensus and the variant sites (polyhip_pileup).

The definition is the comment above ``polyhip_pileup`` in include/polyhip.h and tests/pileup_oracle.py restates it on the
CPU.  Everything is counted in HIP from the arrays a ``mapper.MapResult`` holds and the text the reads were mapped to;
nothing is computed here.  The counts are integers and say how many reads show an insertion, not what was inserted; the
inserted and deleted bytes are in the text rows of ``rows`` / ``rows_packed`` / ``rows_refs`` (polyhip_pileup_rows, restated
in tests/pileup_rows_oracle.py), the six-column pileup format that ``pileup_text`` parses.  The alleles themselves and the records
of a VCF are ``poly_amd.variants`` (polyhip_call_variants) and ``poly_amd.vcf``.  One text.
``pileup`` / ``pileup_packed`` / ``pileup_refs`` do not look at base qualities; the ``*_qual`` calls
(polyhip_pileup_qual, restated in tests/pileup_qual_oracle.py) take the reads' quality strings as ``fastq.pack_qual`` packs
them, count a base only when its quality reaches ``min_base_qual`` and add ``qsum``, the sum of the counted qualities per
base and strand.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

CHANNELS = 16
CH_A, CH_C, CH_G, CH_T, CH_OTHER, CH_DEL, CH_INS_EVENT, CH_DEL_EVENT = range(8)      # + 8 on the reverse strand
KIND_SNV, KIND_INS, KIND_DEL = 1, 2, 3
SITE_DTYPE = np.dtype([("pos", np.uint32), ("depth", np.uint32), ("count", np.uint32), ("count_fwd", np.uint32),
                       ("kind", np.uint8), ("ref", np.uint8), ("alt", np.uint8), ("pad", np.uint8)])


class _CParams(C.Structure):
    _fields_ = [("region_lo", C.c_uint64), ("region_hi", C.c_uint64), ("min_mapq", C.c_uint32), ("min_depth", C.c_uint32),
                ("min_alt_count", C.c_uint32), ("min_alt_permille", C.c_uint32)]


class _CInfo(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("used", C.c_uint64), ("skipped_mapq", C.c_uint64), ("bad", C.c_uint64),
                ("columns", C.c_uint64), ("edge_events", C.c_uint64), ("sites", C.c_uint64)]


def last_info() -> dict:
    """polyhip_pileup_last_info: what the calling thread's last call did"""
    info = _CInfo()
    _lib.check(_lib.lib().polyhip_pileup_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CInfo._fields_}


@dataclass
class Pileup:
    """``counts[8 * strand + k, p - region_lo]``: k = 0..3 reads saying A, C, G, T at p, 4 any other byte, 5 a deleted base,
    6 insertion events and 7 deletion events anchored at p.  ``sites``: a structured array of SITE_DTYPE.  ``status``: OK, or
    ERR_INVALID when a site capacity that the caller fixed was short (``nsites`` then says what is needed and ``sites`` is
    None)."""
    counts: np.ndarray
    consensus: np.ndarray
    sites: np.ndarray | None
    err: np.ndarray
    nsites: int = 0
    region_lo: int = 0
    status: int = 0

    def depth(self) -> np.ndarray:
        """reads covering each position: the base, other and deleted-base channels of both strands"""
        return self.counts[0:6].astype(np.uint64).sum(axis=0) + self.counts[8:14].astype(np.uint64).sum(axis=0)

    def consensus_string(self) -> str:
        return self.consensus.tobytes().decode("latin-1")

    last_info = staticmethod(last_info)


def _sites_short() -> bool:
    """the last ERR_INVALID was the one about the site capacity (everything else was delivered)"""
    return b"the sites need" in _lib.lib().polyhip_last_error()


def _without(flags, dup):
    """the flags with bit 0 (mapped) cleared, in a copy, where ``dup`` is set: the pileup then leaves the duplicates out"""
    if dup is None:
        return flags
    flags, dup = np.asarray(flags, dtype=np.uint32), np.asarray(dup)
    if len(dup) != len(flags):
        raise ValueError("pileup: dup holds another number of entries than the result")
    return np.where(dup != 0, flags & ~np.uint32(1), flags).astype(np.uint32)


def pileup_packed(flags, ref_start, ref_end, alnA, alnB, aln_off, ref, mapq=None, region=None, min_mapq: int = 0, min_depth: int = 1,
                  min_alt_count: int = 1, min_alt_permille: int = 0, site_capacity: int | None = None, dup=None) -> Pileup:
    """polyhip_pileup on packed arrays.  ``region``: (lo, hi) text positions, the whole text by default.  The site capacity
    defaults to a guess; a call that needs more is run again with the exact size -- unless a capacity was given, in which
    case the result carries ``status`` = ERR_INVALID, ``nsites``, and no ``sites``.  ``dup``: ``dedup.Duplicates.dup``; its
    entries are passed as unmapped."""
    n = len(flags)
    flags = _without(flags, dup)
    flags, ref_start, ref_end = (np.ascontiguousarray(x, dtype=np.uint32) for x in (flags, ref_start, ref_end))
    alnA, alnB = (np.ascontiguousarray(x, dtype=np.uint8) for x in (alnA, alnB))
    aln_off = np.ascontiguousarray(aln_off, dtype=np.uint64)
    ref = np.ascontiguousarray(np.frombuffer(ref, np.uint8) if isinstance(ref, (bytes, bytearray)) else ref, dtype=np.uint8)
    if mapq is not None:
        mapq = np.ascontiguousarray(mapq, dtype=np.uint8)
        if len(mapq) != n:
            raise ValueError("pileup_packed: the arrays hold different numbers of entries")
    if not (len(ref_start) == len(ref_end) == n and len(aln_off) == n + 1):
        raise ValueError("pileup_packed: the arrays hold different numbers of entries")
    if n and int(aln_off[n]) > min(len(alnA), len(alnB)):
        raise ValueError("pileup_packed: the offsets reach beyond the strings")
    lo, hi = (0, len(ref)) if region is None else (int(region[0]), int(region[1]))
    p = _CParams(lo, hi, int(min_mapq), int(min_depth), int(min_alt_count), int(min_alt_permille))
    L = max(hi - lo, 0) if hi <= len(ref) else 0         # a region the library refuses: it says so, nothing is sized by it
    fixed = site_capacity is not None
    cap = int(site_capacity) if fixed else L // 64 + 1024
    counts, consensus = np.zeros((CHANNELS, L), np.uint32), np.zeros(L, np.uint8)
    err, nsites = np.zeros(n, np.uint32), C.c_uint64(0)
    ref_buf = ref if len(ref) else np.zeros(1, np.uint8)       # ref is always required, an empty text too
    sites = None
    rc = _lib.OK
    for _ in range(2):
        sites = np.zeros(max(cap, 1), SITE_DTYPE)
        rc = _lib.lib().polyhip_pileup(C.byref(p), n, flags.ctypes.data, None if mapq is None else mapq.ctypes.data,
                                       ref_start.ctypes.data, ref_end.ctypes.data, alnA.ctypes.data, alnB.ctypes.data,
                                       aln_off.ctypes.data, ref_buf.ctypes.data, len(ref), counts.ctypes.data, consensus.ctypes.data,
                                       C.byref(nsites), sites.ctypes.data, cap, err.ctypes.data)
        if rc == _lib.ERR_INVALID and _sites_short():       # nsites says what the sites need
            if fixed:
                return Pileup(counts, consensus, None, err, int(nsites.value), lo, int(rc))
            cap = int(nsites.value)
            continue
        _lib.check(rc)
        break
    return Pileup(counts, consensus, sites[:int(nsites.value)], err, int(nsites.value), lo, int(rc))


def _joined(result):
    """the strings of a MapResult as polyhip_pileup takes them: alnA, alnB back to back and their offsets"""
    a, b = b"".join(result.alignA), b"".join(result.alignB)
    off = np.zeros(len(result.alignA) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in result.alignA], dtype=np.uint64)
    return np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8), off


def _on_contig(who: str, result, refs, contig: int, region):
    """one contig of a RefSet as a region of the set's concatenated text -> (flags, ref_start, ref_end, region, base, lo):
    every entry moved to ``ref_start + starts[rid]``, entries of other contigs passed as unmapped"""
    if result.alignA is None or result.alignB is None:
        raise ValueError(f"pileup.{who}: the MapResult holds no strings")
    if result.rid is None:
        raise ValueError(f"pileup.{who}: the MapResult holds no contigs (it is not the result of a refs call)")
    c = int(contig)
    if not 0 <= c < len(refs):
        raise ValueError(f"pileup.{who}: contig {c} of {len(refs)}")
    base, length = int(refs.starts[c]), int(refs.lengths[c])
    lo, hi = (0, length) if region is None else (int(region[0]), int(region[1]))
    if not 0 <= lo <= hi <= length:
        raise ValueError(f"pileup.{who}: region [{lo}, {hi}) is not inside the contig of {length} bytes")
    here = np.asarray(result.rid) == c
    shift = refs.starts[np.asarray(result.rid, dtype=np.int64)]
    flags = np.where(here, result.flags, 0).astype(np.uint32)
    return (flags, (result.ref_start + shift).astype(np.uint32), (result.ref_end + shift).astype(np.uint32), (base + lo, base + hi), base,
            lo)


def _local(out, base: int, lo: int):
    """a pileup of the concatenation back in the contig's own positions"""
    out.region_lo = lo
    if out.sites is not None:
        out.sites["pos"] -= np.uint32(base)
    return out


def pileup(result, ref, records=None, region=None, min_mapq: int = 0, min_depth: int = 1, min_alt_count: int = 1,
           min_alt_permille: int = 0, site_capacity: int | None = None, dup=None) -> Pileup:
    """The pileup of a ``mapper.MapResult`` that holds its strings on the text ``ref`` it was mapped to.  ``records``: the
    ``sam.AlnRecords`` of the same result; its ``mapq`` is what ``min_mapq`` is compared with (without one, ``min_mapq`` must
    be 0)."""
    if result.alignA is None or result.alignB is None:
        raise ValueError("pileup.pileup: the MapResult holds no strings")
    a, b, off = _joined(result)
    if isinstance(ref, str):
        ref = ref.encode("latin-1")
    return pileup_packed(result.flags, result.ref_start, result.ref_end, a, b, off, ref, None if records is None else records.mapq,
                         region, min_mapq, min_depth, min_alt_count, min_alt_permille, site_capacity, dup)


def pileup_refs(result, refs, contig: int, records=None, region=None, min_mapq: int = 0, min_depth: int = 1,
                min_alt_count: int = 1, min_alt_permille: int = 0, site_capacity: int | None = None, dup=None) -> Pileup:
    """The pileup of one contig of a ``refs.RefSet`` from the result of ``mapper.map_reads_refs_packed`` /
    ``map_pairs_refs_packed`` on that set.  ``region``: (lo, hi) inside the contig, the whole contig by default.
    polyhip_pileup runs on the set's concatenated text (``refs.text()``, read back from the index) with every entry moved
    to ``ref_start + starts[rid]`` and the region to ``[starts[contig] + lo, starts[contig] + hi)``; entries of other contigs
    are passed as unmapped.  No alignment crosses a contig, so nothing else is needed.  The Pileup that comes back is local
    to the contig: ``region_lo`` and the sites' ``pos`` are positions in it."""
    flags, ref_start, ref_end, where, base, lo = _on_contig("pileup_refs", result, refs, contig, region)
    a, b, off = _joined(result)
    out = pileup_packed(flags, ref_start, ref_end, a, b, off, refs.text(), None if records is None else records.mapq, where, min_mapq,
                        min_depth, min_alt_count, min_alt_permille, site_capacity, dup)
    return _local(out, base, lo)


# ---- with base qualities (polyhip_pileup_qual) ----------------------------------------------------------------------------------
QSUM_PLANES = 8


class _CQualParams(C.Structure):
    _fields_ = [("base", _CParams), ("min_base_qual", C.c_uint32), ("qual_offset", C.c_uint32)]


class _CQualInfo(C.Structure):
    _fields_ = _CInfo._fields_ + [("filtered_bases", C.c_uint64)]


def last_qual_info() -> dict:
    """polyhip_pileup_qual_last_info: what the calling thread's last ``*_qual`` call did"""
    info = _CQualInfo()
    _lib.check(_lib.lib().polyhip_pileup_qual_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CQualInfo._fields_}


@dataclass
class PileupQual(Pileup):
    """``Pileup`` of the bases whose quality reached ``min_base_qual``, plus ``qsum[4 * strand + k, p - region_lo]``: the sum of
    the qualities of the counted bases k = 0..3 (A, C, G, T) at p.  Deleted bases and the events are not filtered."""
    qsum: np.ndarray | None = None

    last_info = staticmethod(last_qual_info)


def pileup_qual_packed(flags, ref_start, ref_end, read_start, alnA, alnB, aln_off, qual, qual_off, ref, mapq=None, region=None,
                       min_mapq: int = 0, min_depth: int = 1, min_alt_count: int = 1, min_alt_permille: int = 0,
                       site_capacity: int | None = None, min_base_qual: int = 0, qual_offset: int = 33, dup=None) -> PileupQual:
    """polyhip_pileup_qual on packed arrays: ``pileup_packed`` plus ``read_start`` (of the mapper's result), the quality
    strings ``qual`` / ``qual_off`` of the reads as sequenced, one per entry, and the two quality settings."""
    n = len(flags)
    flags = _without(flags, dup)
    flags, ref_start, ref_end, read_start = (np.ascontiguousarray(x, dtype=np.uint32) for x in (flags, ref_start, ref_end, read_start))
    alnA, alnB, qual = (np.ascontiguousarray(x, dtype=np.uint8) for x in (alnA, alnB, qual))
    aln_off, qual_off = (np.ascontiguousarray(x, dtype=np.uint64) for x in (aln_off, qual_off))
    ref = np.ascontiguousarray(np.frombuffer(ref, np.uint8) if isinstance(ref, (bytes, bytearray)) else ref, dtype=np.uint8)
    if mapq is not None:
        mapq = np.ascontiguousarray(mapq, dtype=np.uint8)
        if len(mapq) != n:
            raise ValueError("pileup_qual_packed: the arrays hold different numbers of entries")
    if not (len(ref_start) == len(ref_end) == len(read_start) == n and len(aln_off) == len(qual_off) == n + 1):
        raise ValueError("pileup_qual_packed: the arrays hold different numbers of entries")
    if n and (int(aln_off[n]) > min(len(alnA), len(alnB)) or int(qual_off[n]) > len(qual)):
        raise ValueError("pileup_qual_packed: the offsets reach beyond the strings")
    lo, hi = (0, len(ref)) if region is None else (int(region[0]), int(region[1]))
    p = _CQualParams(_CParams(lo, hi, int(min_mapq), int(min_depth), int(min_alt_count), int(min_alt_permille)), int(min_base_qual),
                     int(qual_offset))
    L = max(hi - lo, 0) if hi <= len(ref) else 0         # a region the library refuses: it says so, nothing is sized by it
    fixed = site_capacity is not None
    cap = int(site_capacity) if fixed else L // 64 + 1024
    counts, qsum, consensus = np.zeros((CHANNELS, L), np.uint32), np.zeros((QSUM_PLANES, L), np.uint32), np.zeros(L, np.uint8)
    err, nsites = np.zeros(n, np.uint32), C.c_uint64(0)
    ref_buf = ref if len(ref) else np.zeros(1, np.uint8)       # ref is always required, an empty text too
    sites = None
    rc = _lib.OK
    for _ in range(2):
        sites = np.zeros(max(cap, 1), SITE_DTYPE)
        rc = _lib.lib().polyhip_pileup_qual(C.byref(p), n, flags.ctypes.data, None if mapq is None else mapq.ctypes.data,
                                            ref_start.ctypes.data, ref_end.ctypes.data, read_start.ctypes.data, alnA.ctypes.data,
                                            alnB.ctypes.data, aln_off.ctypes.data, qual.ctypes.data, qual_off.ctypes.data,
                                            ref_buf.ctypes.data, len(ref), counts.ctypes.data, qsum.ctypes.data, consensus.ctypes.data,
                                            C.byref(nsites), sites.ctypes.data, cap, err.ctypes.data)
        if rc == _lib.ERR_INVALID and _sites_short():       # nsites says what the sites need
            if fixed:
                return PileupQual(counts, consensus, None, err, int(nsites.value), lo, int(rc), qsum)
            cap = int(nsites.value)
            continue
        _lib.check(rc)
        break
    return PileupQual(counts, consensus, sites[:int(nsites.value)], err, int(nsites.value), lo, int(rc), qsum)


def _same_lengths(who: str, read_offsets, qual_offsets):
    """a quality longer than its read raises no err in the library (it reads as a clip): caught here when the caller hands
    the reads' offsets in"""
    if read_offsets is None:
        return
    r, q = np.asarray(read_offsets, dtype=np.uint64), np.asarray(qual_offsets, dtype=np.uint64)
    if len(r) != len(q) or (np.diff(r) != np.diff(q)).any():
        raise ValueError(f"pileup.{who}: some quality string is not as long as its read (fastq.pack_qual's mismatch count is not 0)")


def pileup_qual(result, ref, quals, qual_offsets, records=None, region=None, min_mapq: int = 0, min_depth: int = 1,
                min_alt_count: int = 1, min_alt_permille: int = 0, site_capacity: int | None = None, min_base_qual: int = 0,
                qual_offset: int = 33, read_offsets=None, dup=None) -> PileupQual:
    """``pileup`` with the base qualities: ``quals`` / ``qual_offsets`` as ``fastq.pack_qual`` returns them for the reads the
    result was mapped from (every quality as long as its read), in the result's entry order -- for a paired result the
    mates' strings interleaved, 2i and 2i + 1.  ``read_offsets``: the offsets of those reads (``fastq.pack_qual``'s
    ``offsets``); when given, a quality of another length than its read is a ValueError instead of bases silently paired
    with the wrong bytes."""
    if result.alignA is None or result.alignB is None:
        raise ValueError("pileup.pileup_qual: the MapResult holds no strings")
    _same_lengths("pileup_qual", read_offsets, qual_offsets)
    a, b, off = _joined(result)
    if isinstance(ref, str):
        ref = ref.encode("latin-1")
    return pileup_qual_packed(result.flags, result.ref_start, result.ref_end, result.read_start, a, b, off, quals, qual_offsets, ref,
                              None if records is None else records.mapq, region, min_mapq, min_depth, min_alt_count, min_alt_permille,
                              site_capacity, min_base_qual, qual_offset, dup)


def pileup_qual_refs(result, refs, contig: int, quals, qual_offsets, records=None, region=None, min_mapq: int = 0, min_depth: int = 1,
                     min_alt_count: int = 1, min_alt_permille: int = 0, site_capacity: int | None = None, min_base_qual: int = 0,
                     qual_offset: int = 33, read_offsets=None, dup=None) -> PileupQual:
    """``pileup_refs`` with the base qualities: one contig of a ``refs.RefSet``, moved to the set's concatenated text and back
    exactly as ``pileup_refs`` does it.  ``read_offsets`` as in ``pileup_qual``."""
    flags, ref_start, ref_end, where, base, lo = _on_contig("pileup_qual_refs", result, refs, contig, region)
    _same_lengths("pileup_qual_refs", read_offsets, qual_offsets)
    a, b, off = _joined(result)
    out = pileup_qual_packed(flags, ref_start, ref_end, result.read_start, a, b, off, quals, qual_offsets, refs.text(),
                             None if records is None else records.mapq, where, min_mapq, min_depth, min_alt_count, min_alt_permille,
                             site_capacity, min_base_qual, qual_offset, dup)
    return _local(out, base, lo)


# ---- as text rows (polyhip_pileup_rows) -------------------------------------------------------------------------------------------
class _CRowsParams(C.Structure):
    _fields_ = [("region_lo", C.c_uint64), ("region_hi", C.c_uint64), ("pos_origin", C.c_uint64), ("min_mapq", C.c_uint32),
                ("qual_offset", C.c_uint32), ("all_positions", C.c_uint32), ("pad", C.c_uint32)]


class _CRowsInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("entries", "used", "skipped_mapq", "bad", "columns", "tokens", "rows", "text_bytes",
                                           "dropped_events", "max_row_bytes")]


def last_rows_info() -> dict:
    """polyhip_pileup_rows_last_info: what the calling thread's last ``rows*`` call did.  ``max_row_bytes`` above
    ``pileup_text.MAX_LINE_SIZE`` means the reference's parser refuses the longest row."""
    info = _CRowsInfo()
    _lib.check(_lib.lib().polyhip_pileup_rows_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CRowsInfo._fields_}


@dataclass
class PileupRows:
    """``text``: the rows of the region as one uint8 array, ascending position, each ``name \\t pos \\t ref \\t depth \\t tokens \\t
    qualities \\n``.  ``row_off``: L + 1 offsets, the row of position p is ``text[row_off[p - region_lo]:row_off[p - region_lo + 1]]``
    (empty where no row is written).  ``status``: OK, or ERR_INVALID when a text capacity that the caller fixed was short
    (``ntext`` then says what is needed and ``text`` is None)."""
    text: np.ndarray | None
    row_off: np.ndarray
    err: np.ndarray
    nrows: int = 0
    status: int = 0
    region_lo: int = 0
    ntext: int = 0

    def row(self, p: int) -> bytes:
        """the row of text position p (in the positions ``region_lo`` counts in), b"" where none was written"""
        j = int(p) - self.region_lo
        if not 0 <= j < len(self.row_off) - 1:
            raise IndexError(f"PileupRows.row: position {p} is outside the region")
        if self.text is None:
            raise ValueError("PileupRows.row: the call delivered no text")
        return self.text[int(self.row_off[j]):int(self.row_off[j + 1])].tobytes()

    def tobytes(self) -> bytes:
        return b"" if self.text is None else self.text.tobytes()

    def parse(self) -> list:
        """the rows as ``pileup_text.Pileup`` records"""
        from . import pileup_text
        return pileup_text.parse(self.tobytes())

    last_info = staticmethod(last_rows_info)


def _text_short() -> bool:
    return b"the text needs" in _lib.lib().polyhip_last_error()


def rows_packed(flags, ref_start, ref_end, alnA, alnB, aln_off, ref, name, mapq=None, read_start=None, qual=None, qual_off=None,
                order=None, region=None, pos_origin: int = 0, min_mapq: int = 0, qual_offset: int = 33, all_positions: bool = False,
                text_capacity: int | None = None, dup=None) -> PileupRows:
    """polyhip_pileup_rows on packed arrays.  ``name``: the sequence name of column 1.  ``qual`` / ``qual_off`` / ``read_start``:
    as in ``pileup_qual_packed``, or all None for rows without qualities ('~' everywhere).  ``order``: the permutation of
    ``dedup.coord_order``; None is entry order.  ``pos_origin``: column 2 prints ``p - pos_origin + 1``.  The text capacity
    defaults to a guess; a call that needs more is run again with the exact size -- unless a capacity was given, in which
    case the result carries ``status`` = ERR_INVALID, ``ntext``, and no ``text``.  ``dup``: as in ``pileup_packed``."""
    n = len(flags)
    flags = _without(flags, dup)
    flags, ref_start, ref_end = (np.ascontiguousarray(x, dtype=np.uint32) for x in (flags, ref_start, ref_end))
    alnA, alnB = (np.ascontiguousarray(x, dtype=np.uint8) for x in (alnA, alnB))
    aln_off = np.ascontiguousarray(aln_off, dtype=np.uint64)
    ref = np.ascontiguousarray(np.frombuffer(ref, np.uint8) if isinstance(ref, (bytes, bytearray)) else ref, dtype=np.uint8)
    if isinstance(name, str):
        name = name.encode("latin-1")
    name = np.frombuffer(bytes(name), np.uint8)
    if not (len(ref_start) == len(ref_end) == n and len(aln_off) == n + 1):
        raise ValueError("rows_packed: the arrays hold different numbers of entries")
    if n and int(aln_off[n]) > min(len(alnA), len(alnB)):
        raise ValueError("rows_packed: the offsets reach beyond the strings")
    if mapq is not None:
        mapq = np.ascontiguousarray(mapq, dtype=np.uint8)
        if len(mapq) != n:
            raise ValueError("rows_packed: the arrays hold different numbers of entries")
    if qual is not None:
        if read_start is None or qual_off is None:
            raise ValueError("rows_packed: qual comes with read_start and qual_off")
        qual, read_start = np.ascontiguousarray(qual, dtype=np.uint8), np.ascontiguousarray(read_start, dtype=np.uint32)
        qual_off = np.ascontiguousarray(qual_off, dtype=np.uint64)
        if len(read_start) != n or len(qual_off) != n + 1:
            raise ValueError("rows_packed: the arrays hold different numbers of entries")
        if n and int(qual_off[n]) > len(qual):
            raise ValueError("rows_packed: the offsets reach beyond the strings")
        if len(qual) == 0:
            qual = np.zeros(1, np.uint8)       # a non-NULL pointer: the qualities are given, and empty
    if order is not None:
        order = np.ascontiguousarray(order, dtype=np.uint32)
        if len(order) != n:
            raise ValueError("rows_packed: order holds another number of entries than the result")
        if n == 0:
            order = None
    lo, hi = (0, len(ref)) if region is None else (int(region[0]), int(region[1]))
    p = _CRowsParams(lo, hi, int(pos_origin), int(min_mapq), int(qual_offset), int(all_positions), 0)
    L = max(hi - lo, 0) if hi <= len(ref) else 0         # a region the library refuses: it says so, nothing is sized by it
    nbytes = int(aln_off[n] - aln_off[0]) if n else 0
    fixed = text_capacity is not None
    cap = int(text_capacity) if fixed else 2 * nbytes + (L if all_positions else min(L, nbytes)) * (len(name) + 16) + 1024
    row_off, err, ntext = np.zeros(L + 1, np.uint64), np.zeros(n, np.uint32), C.c_uint64(0)
    ref_buf = ref if len(ref) else np.zeros(1, np.uint8)       # ref is always required, an empty text too
    ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    text = None
    rc = _lib.OK
    for _ in range(2):
        text = np.zeros(max(cap, 1), np.uint8)
        rc = _lib.lib().polyhip_pileup_rows(C.byref(p), n, flags.ctypes.data, ptr(mapq), ref_start.ctypes.data, ref_end.ctypes.data,
                                            ptr(read_start) if qual is not None else None, alnA.ctypes.data, alnB.ctypes.data,
                                            aln_off.ctypes.data, ptr(qual), ptr(qual_off) if qual is not None else None,
                                            ref_buf.ctypes.data, len(ref), ptr(order), name.ctypes.data if len(name) else None, len(name),
                                            C.byref(ntext), text.ctypes.data, cap, row_off.ctypes.data, err.ctypes.data)
        if rc == _lib.ERR_INVALID and _text_short():        # ntext says what the text needs
            if fixed:
                return PileupRows(None, row_off, err, last_rows_info()["rows"], int(rc), lo, int(ntext.value))
            cap = int(ntext.value)
            continue
        _lib.check(rc)
        break
    return PileupRows(text[:int(ntext.value)], row_off, err, last_rows_info()["rows"], int(rc), lo, int(ntext.value))


def _rows_quals(who: str, quals, qual_offsets, read_offsets, result):
    if quals is None:
        return None, None, None
    if qual_offsets is None:
        raise ValueError(f"pileup.{who}: quals comes with qual_offsets")
    _same_lengths(who, read_offsets, qual_offsets)
    return result.read_start, quals, qual_offsets


def rows(result, ref, name, quals=None, qual_offsets=None, records=None, region=None, min_mapq: int = 0, order=None, dup=None,
         all_positions: bool = False, read_offsets=None, qual_offset: int = 33, text_capacity: int | None = None) -> PileupRows:
    """The pileup rows of a ``mapper.MapResult`` that holds its strings on the text ``ref``, named ``name`` in column 1.
    ``records``: the ``sam.AlnRecords`` of the result; its ``mapq`` feeds both ``min_mapq`` and the byte behind '^' (without
    one that byte is '~').  ``quals`` / ``qual_offsets`` / ``read_offsets`` and ``dup`` as in ``pileup_qual``; ``order``: the
    permutation ``dedup.coord_order`` returns, which gives the reads of a row the order samtools would print them in."""
    if result.alignA is None or result.alignB is None:
        raise ValueError("pileup.rows: the MapResult holds no strings")
    read_start, quals, qual_offsets = _rows_quals("rows", quals, qual_offsets, read_offsets, result)
    a, b, off = _joined(result)
    if isinstance(ref, str):
        ref = ref.encode("latin-1")
    return rows_packed(result.flags, result.ref_start, result.ref_end, a, b, off, ref, name, None if records is None else records.mapq,
                       read_start, quals, qual_offsets, order, region, 0, min_mapq, qual_offset, all_positions, text_capacity, dup)


def rows_refs(result, refs, contig: int, name, quals=None, qual_offsets=None, records=None, region=None, min_mapq: int = 0, order=None,
              dup=None, all_positions: bool = False, read_offsets=None, qual_offset: int = 33,
              text_capacity: int | None = None) -> PileupRows:
    """``rows`` for one contig of a ``refs.RefSet``, moved to the set's concatenated text exactly as ``pileup_refs`` does it, with
    ``pos_origin`` at the contig's start: column 2 and ``region_lo`` are positions in the contig."""
    flags, ref_start, ref_end, where, base, lo = _on_contig("rows_refs", result, refs, contig, region)
    read_start, quals, qual_offsets = _rows_quals("rows_refs", quals, qual_offsets, read_offsets, result)
    a, b, off = _joined(result)
    out = rows_packed(flags, ref_start, ref_end, a, b, off, refs.text(), name, None if records is None else records.mapq, read_start,
                      quals, qual_offsets, order, where, base, min_mapq, qual_offset, all_positions, text_capacity, dup)
    out.region_lo = lo
    return out
