"""Variant calls from the read mapper's output: SNVs, insertion and deletion alleles with their bytes, indels left-aligned
(polyhip_call_variants).

The definition is the comment above ``polyhip_call_variants`` in include/polyhip.h and tests/variants_oracle.py restates it on
the CPU.  The reads' events are grouped into alleles, counted per strand and put to the pileup's thresholds in HIP; nothing is
computed here.  What comes back are records, one per SNV and per passing allele, and the pool of the inserted bytes;
``poly_amd.vcf`` writes them as VCF text.  The arrays are those of ``pileup.pileup_qual*``; the qualities are optional.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .pileup import KIND_DEL, KIND_INS, KIND_SNV, _CParams, _CQualParams, _joined, _on_contig, _same_lengths, _without  # noqa: F401

MAX_INDEL = 255
VARIANT_DTYPE = np.dtype([("allele_off", np.uint64), ("pos", np.uint32), ("depth", np.uint32), ("count", np.uint32),
                          ("count_fwd", np.uint32), ("ref_count", np.uint32), ("qsum", np.uint32), ("allele_len", np.uint32),
                          ("kind", np.uint8), ("ref", np.uint8), ("alt", np.uint8), ("gt", np.uint8)])
assert VARIANT_DTYPE.itemsize == 40


class _CVarParams(C.Structure):
    _fields_ = [("base", _CQualParams), ("left_align", C.c_uint32), ("hom_permille", C.c_uint32), ("max_indel", C.c_uint32),
                ("pad", C.c_uint32)]


class _CVarInfo(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("entries", "used", "skipped_mapq", "bad", "columns", "edge_events", "sites", "filtered_bases",
                                           "events", "long_events", "open_events", "shifted_events", "alleles", "allele_bytes")]


def last_info() -> dict:
    """polyhip_call_variants_last_info: what the calling thread's last call did"""
    info = _CVarInfo()
    _lib.check(_lib.lib().polyhip_call_variants_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CVarInfo._fields_}


@dataclass
class Variants:
    """``records``: a structured array of VARIANT_DTYPE, ascending position; within a position the SNVs to A, C, G, T, then the
    insertion alleles by (length, bytes), then the deletion alleles by length.  ``alleles``: the inserted bytes of the records,
    upper case, ``alleles[allele_off:allele_off + allele_len]`` for an insertion.  ``ref``: the text the positions count in
    (for a contig of a RefSet the contig's own text).  ``status``: OK, or ERR_INVALID when a capacity that the caller fixed was
    short (``nvariants`` and ``nallele_bytes`` then say what is needed, ``records`` and ``alleles`` are None)."""
    records: np.ndarray | None
    alleles: np.ndarray | None
    err: np.ndarray
    ref: np.ndarray
    status: int = 0
    region_lo: int = 0
    nvariants: int = 0
    nallele_bytes: int = 0

    def inserted(self, i: int) -> bytes:
        """the inserted bytes of record i (b"" for an SNV and a deletion)"""
        r = self.records[i]
        if r["kind"] != KIND_INS:
            return b""
        return self.alleles[int(r["allele_off"]):int(r["allele_off"]) + int(r["allele_len"])].tobytes()

    def ref_allele(self, i: int) -> bytes:
        """the VCF REF of record i: the text byte for an SNV, the anchor byte for an insertion, the anchor byte and the deleted
        text for a deletion"""
        r = self.records[i]
        p = int(r["pos"])
        return self.ref[p:p + 1 + (int(r["allele_len"]) if r["kind"] == KIND_DEL else 0)].tobytes()

    def alt_allele(self, i: int) -> bytes:
        """the VCF ALT of record i: the called base, the anchor byte and the inserted bytes, or the anchor byte alone"""
        r = self.records[i]
        if r["kind"] == KIND_SNV:
            return bytes([int(r["alt"])])
        return bytes([int(r["ref"])]) + self.inserted(i)

    last_info = staticmethod(last_info)


def _short() -> bool:
    msg = _lib.lib().polyhip_last_error()
    return b"the variants need" in msg or b"the alleles need" in msg


def call_packed(flags, ref_start, ref_end, alnA, alnB, aln_off, ref, mapq=None, read_start=None, qual=None, qual_off=None, region=None,
                min_mapq: int = 0, min_depth: int = 1, min_alt_count: int = 1, min_alt_permille: int = 0, min_base_qual: int = 0,
                qual_offset: int = 33, left_align: bool = True, hom_permille: int = 800, max_indel: int = 0,
                variant_capacity: int | None = None, allele_capacity: int | None = None, dup=None) -> Variants:
    """polyhip_call_variants on packed arrays.  ``qual`` / ``qual_off`` / ``read_start``: as in ``pileup.pileup_qual_packed``, or all
    None for a call without qualities.  The capacities default to a guess; a call that needs more is run again with the exact
    sizes -- unless a capacity was given, in which case the result carries ``status`` = ERR_INVALID and the sizes.  ``dup``: as
    in ``pileup.pileup_packed``."""
    n = len(flags)
    flags = _without(flags, dup)
    flags, ref_start, ref_end = (np.ascontiguousarray(x, dtype=np.uint32) for x in (flags, ref_start, ref_end))
    alnA, alnB = (np.ascontiguousarray(x, dtype=np.uint8) for x in (alnA, alnB))
    aln_off = np.ascontiguousarray(aln_off, dtype=np.uint64)
    ref = np.ascontiguousarray(np.frombuffer(ref, np.uint8) if isinstance(ref, (bytes, bytearray)) else ref, dtype=np.uint8)
    if not (len(ref_start) == len(ref_end) == n and len(aln_off) == n + 1):
        raise ValueError("call_packed: the arrays hold different numbers of entries")
    if n and int(aln_off[n]) > min(len(alnA), len(alnB)):
        raise ValueError("call_packed: the offsets reach beyond the strings")
    if mapq is not None:
        mapq = np.ascontiguousarray(mapq, dtype=np.uint8)
        if len(mapq) != n:
            raise ValueError("call_packed: the arrays hold different numbers of entries")
    if qual is not None:
        if read_start is None or qual_off is None:
            raise ValueError("call_packed: qual comes with read_start and qual_off")
        qual, read_start = np.ascontiguousarray(qual, dtype=np.uint8), np.ascontiguousarray(read_start, dtype=np.uint32)
        qual_off = np.ascontiguousarray(qual_off, dtype=np.uint64)
        if len(read_start) != n or len(qual_off) != n + 1:
            raise ValueError("call_packed: the arrays hold different numbers of entries")
        if n and int(qual_off[n]) > len(qual):
            raise ValueError("call_packed: the offsets reach beyond the strings")
        if len(qual) == 0:
            qual = np.zeros(1, np.uint8)       # a non-NULL pointer: the qualities are given, and empty
    lo, hi = (0, len(ref)) if region is None else (int(region[0]), int(region[1]))
    p = _CVarParams(_CQualParams(_CParams(lo, hi, int(min_mapq), int(min_depth), int(min_alt_count), int(min_alt_permille)), int(min_base_qual),
                                 int(qual_offset)), int(bool(left_align)), int(hom_permille), int(max_indel), 0)
    L = max(hi - lo, 0) if hi <= len(ref) else 0         # a region the library refuses: it says so, nothing is sized by it
    fixed = variant_capacity is not None or allele_capacity is not None
    vcap = int(variant_capacity) if variant_capacity is not None else L // 64 + 1024
    acap = int(allele_capacity) if allele_capacity is not None else L // 64 + 4096
    err, nvar, nbytes = np.zeros(n, np.uint32), C.c_uint64(0), C.c_uint64(0)
    ref_buf = ref if len(ref) else np.zeros(1, np.uint8)       # ref is always required, an empty text too
    ptr = lambda a: None if a is None else a.ctypes.data       # noqa: E731
    records = alleles = None
    rc = _lib.OK
    for _ in range(2):
        records, alleles = np.zeros(max(vcap, 1), VARIANT_DTYPE), np.zeros(max(acap, 1), np.uint8)
        rc = _lib.lib().polyhip_call_variants(C.byref(p), n, flags.ctypes.data, ptr(mapq), ref_start.ctypes.data, ref_end.ctypes.data,
                                              ptr(read_start) if qual is not None else None, alnA.ctypes.data, alnB.ctypes.data,
                                              aln_off.ctypes.data, ptr(qual), ptr(qual_off) if qual is not None else None,
                                              ref_buf.ctypes.data, len(ref), C.byref(nvar), records.ctypes.data, vcap, C.byref(nbytes),
                                              alleles.ctypes.data, acap, err.ctypes.data)
        if rc == _lib.ERR_INVALID and _short():             # nvar and nbytes say what the outputs need
            if fixed:
                return Variants(None, None, err, ref, int(rc), lo, int(nvar.value), int(nbytes.value))
            vcap, acap = int(nvar.value), int(nbytes.value)
            continue
        _lib.check(rc)
        break
    return Variants(records[:int(nvar.value)], alleles[:int(nbytes.value)], err, ref, int(rc), lo, int(nvar.value), int(nbytes.value))


def _quals(who: str, quals, qual_offsets, read_offsets, result):
    if quals is None:
        return None, None, None
    if qual_offsets is None:
        raise ValueError(f"variants.{who}: quals comes with qual_offsets")
    _same_lengths(who, read_offsets, qual_offsets)
    return result.read_start, quals, qual_offsets


def call(result, ref, quals=None, qual_offsets=None, records=None, region=None, min_mapq: int = 0, min_depth: int = 1,
         min_alt_count: int = 1, min_alt_permille: int = 0, min_base_qual: int = 0, qual_offset: int = 33, left_align: bool = True,
         hom_permille: int = 800, max_indel: int = 0, variant_capacity: int | None = None, allele_capacity: int | None = None,
         read_offsets=None, dup=None) -> Variants:
    """The variants of a ``mapper.MapResult`` that holds its strings on the text ``ref`` it was mapped to.  ``quals`` /
    ``qual_offsets`` / ``read_offsets``, ``records`` and ``dup`` as in ``pileup.pileup_qual``; without ``quals`` no base is
    filtered."""
    if result.alignA is None or result.alignB is None:
        raise ValueError("variants.call: the MapResult holds no strings")
    read_start, quals, qual_offsets = _quals("call", quals, qual_offsets, read_offsets, result)
    a, b, off = _joined(result)
    if isinstance(ref, str):
        ref = ref.encode("latin-1")
    return call_packed(result.flags, result.ref_start, result.ref_end, a, b, off, ref, None if records is None else records.mapq, read_start,
                       quals, qual_offsets, region, min_mapq, min_depth, min_alt_count, min_alt_permille, min_base_qual, qual_offset,
                       left_align, hom_permille, max_indel, variant_capacity, allele_capacity, dup)


def call_refs(result, refs, contig: int, quals=None, qual_offsets=None, records=None, region=None, min_mapq: int = 0, min_depth: int = 1,
              min_alt_count: int = 1, min_alt_permille: int = 0, min_base_qual: int = 0, qual_offset: int = 33, left_align: bool = True,
              hom_permille: int = 800, max_indel: int = 0, variant_capacity: int | None = None, allele_capacity: int | None = None,
              read_offsets=None, dup=None) -> Variants:
    """``call`` for one contig of a ``refs.RefSet``, moved to the set's concatenated text exactly as ``pileup.pileup_refs`` does it.
    What comes back is local to the contig: ``region_lo``, the records' ``pos`` and ``ref`` are the contig's own."""
    flags, ref_start, ref_end, where, base, lo = _on_contig("call_refs", result, refs, contig, region)
    read_start, quals, qual_offsets = _quals("call_refs", quals, qual_offsets, read_offsets, result)
    a, b, off = _joined(result)
    out = call_packed(flags, ref_start, ref_end, a, b, off, refs.text(), None if records is None else records.mapq, read_start, quals,
                      qual_offsets, where, min_mapq, min_depth, min_alt_count, min_alt_permille, min_base_qual, qual_offset, left_align,
                      hom_permille, max_indel, variant_capacity, allele_capacity, dup)
    out.region_lo = lo
    if out.records is not None:
        out.records["pos"] -= np.uint32(base)
    out.ref = out.ref[base:base + int(refs.lengths[int(contig)])]
    return out
