"""Pileup of the read mapper's output: per-position counts, a consensus and the variant sites (polyhip_pileup).

The definition is the comment above ``polyhip_pileup`` in include/polyhip.h and tests/pileup_oracle.py restates it on the
CPU.  Everything is counted in HIP from the arrays a ``mapper.MapResult`` holds and the text the reads were mapped to;
nothing is computed here.  Integer counts only: no base qualities, no inserted sequences (hence no VCF indel records), no
samtools text rows, one text.
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


def pileup_packed(flags, ref_start, ref_end, alnA, alnB, aln_off, ref, mapq=None, region=None, min_mapq: int = 0, min_depth: int = 1,
                  min_alt_count: int = 1, min_alt_permille: int = 0, site_capacity: int | None = None) -> Pileup:
    """polyhip_pileup on packed arrays.  ``region``: (lo, hi) text positions, the whole text by default.  The site capacity
    defaults to a guess; a call that needs more is run again with the exact size -- unless a capacity was given, in which
    case the result carries ``status`` = ERR_INVALID, ``nsites``, and no ``sites``."""
    n = len(flags)
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


def pileup(result, ref, records=None, region=None, min_mapq: int = 0, min_depth: int = 1, min_alt_count: int = 1,
           min_alt_permille: int = 0, site_capacity: int | None = None) -> Pileup:
    """The pileup of a ``mapper.MapResult`` that holds its strings on the text ``ref`` it was mapped to.  ``records``: the
    ``sam.AlnRecords`` of the same result; its ``mapq`` is what ``min_mapq`` is compared with (without one, ``min_mapq`` must
    be 0)."""
    if result.alignA is None or result.alignB is None:
        raise ValueError("pileup.pileup: the MapResult holds no strings")
    a, b = b"".join(result.alignA), b"".join(result.alignB)
    off = np.zeros(len(result.alignA) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in result.alignA], dtype=np.uint64)
    if isinstance(ref, str):
        ref = ref.encode("latin-1")
    return pileup_packed(result.flags, result.ref_start, result.ref_end, np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8), off,
                         ref, None if records is None else records.mapq, region, min_mapq, min_depth, min_alt_count,
                         min_alt_permille, site_capacity)


def pileup_refs(result, refs, contig: int, records=None, region=None, min_mapq: int = 0, min_depth: int = 1,
                min_alt_count: int = 1, min_alt_permille: int = 0, site_capacity: int | None = None) -> Pileup:
    """The pileup of one contig of a ``refs.RefSet`` from the result of ``mapper.map_reads_refs_packed`` /
    ``map_pairs_refs_packed`` on that set.  ``region``: (lo, hi) inside the contig, the whole contig by default.
    polyhip_pileup runs on the set's concatenated text (``refs.text()``, read back from the index) with every entry moved
    to ``ref_start + starts[rid]`` and the region to ``[starts[contig] + lo, starts[contig] + hi)``; entries of other contigs
    are passed as unmapped.  No alignment crosses a contig, so nothing else is needed.  The Pileup that comes back is local
    to the contig: ``region_lo`` and the sites' ``pos`` are positions in it."""
    if result.alignA is None or result.alignB is None:
        raise ValueError("pileup.pileup_refs: the MapResult holds no strings")
    if result.rid is None:
        raise ValueError("pileup.pileup_refs: the MapResult holds no contigs (it is not the result of a refs call)")
    c = int(contig)
    if not 0 <= c < len(refs):
        raise ValueError(f"pileup.pileup_refs: contig {c} of {len(refs)}")
    base, length = int(refs.starts[c]), int(refs.lengths[c])
    lo, hi = (0, length) if region is None else (int(region[0]), int(region[1]))
    if not 0 <= lo <= hi <= length:
        raise ValueError(f"pileup.pileup_refs: region [{lo}, {hi}) is not inside the contig of {length} bytes")
    a, b = b"".join(result.alignA), b"".join(result.alignB)
    off = np.zeros(len(result.alignA) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in result.alignA], dtype=np.uint64)
    ref = refs.text()
    here = np.asarray(result.rid) == c
    shift = refs.starts[np.asarray(result.rid, dtype=np.int64)]
    flags = np.where(here, result.flags, 0).astype(np.uint32)
    out = pileup_packed(flags, (result.ref_start + shift).astype(np.uint32), (result.ref_end + shift).astype(np.uint32),
                        np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8), off, ref, None if records is None else records.mapq,
                        (base + lo, base + hi), min_mapq, min_depth, min_alt_count, min_alt_permille, site_capacity)
    out.region_lo = lo
    if out.sites is not None:
        out.sites["pos"] -= np.uint32(base)
    return out
