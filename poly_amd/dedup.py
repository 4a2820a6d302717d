"""Duplicate marking and coordinate order of the read mapper's output (polyhip_mark_duplicates, polyhip_coord_order).

PCR duplicates are copies of one template molecule: reads, or pairs, whose unclipped 5' ends coincide.  The definition is the
comment above ``polyhip_mark_duplicates`` in include/polyhip.h and tests/dedup_oracle.py restates it on the CPU.  The keys,
the sorts and the marks are computed in HIP from the arrays a ``mapper.MapResult`` holds; nothing is computed here, and nothing
is removed: ``sam.write(..., dup=d.dup)`` sets 0x400 on the duplicates and ``pileup.pileup(..., dup=d.dup)`` leaves them out.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib


class _CParams(C.Structure):
    _fields_ = [("paired", C.c_uint32), ("weight_mode", C.c_uint32), ("min_weight_qual", C.c_uint32), ("qual_offset", C.c_uint32)]


class _CInfo(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("candidates", C.c_uint64), ("bad", C.c_uint64), ("pairs", C.c_uint64),
                ("fragments", C.c_uint64), ("dup_pairs", C.c_uint64), ("dup_fragments", C.c_uint64), ("pair_sets", C.c_uint64),
                ("end_sets", C.c_uint64)]


def last_info() -> dict:
    """polyhip_dedup_last_info: what the calling thread's last ``mark`` / ``mark_packed`` did"""
    info = _CInfo()
    _lib.check(_lib.lib().polyhip_dedup_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CInfo._fields_}


@dataclass
class Duplicates:
    """one value per entry: ``dup`` 1 for a duplicate, ``rep`` the entry it is a copy of (itself when it is none), ``weight``
    what it was ranked by, ``err`` as the header numbers it (2, 6, 7; 0 for an entry that was judged and found well)."""
    dup: np.ndarray
    rep: np.ndarray
    weight: np.ndarray
    err: np.ndarray
    status: int = 0

    last_info = staticmethod(last_info)


def mark_packed(flags, ref_start, ref_end, read_start, read_end, read_len, rid=None, paired: bool = False, weight=None, qual=None,
                qual_off=None, min_weight_qual: int = 15, qual_offset: int = 33) -> Duplicates:
    """polyhip_mark_duplicates on packed arrays.  ``weight``: one uint32 per entry, the greatest wins its set; or ``qual`` /
    ``qual_off``, the quality strings as ``fastq.pack_qual`` packs them, one per entry: the weight is then the sum of the
    qualities that reach ``min_weight_qual``, computed on the device.  Neither: all weights are 0 and the lowest index wins."""
    n = len(flags)
    flags, ref_start, ref_end, read_start, read_end = (np.ascontiguousarray(x, dtype=np.uint32)
                                                       for x in (flags, ref_start, ref_end, read_start, read_end))
    read_len = np.ascontiguousarray(np.broadcast_to(np.asarray(read_len, dtype=np.uint32), (n,)))
    if not len(ref_start) == len(ref_end) == len(read_start) == len(read_end) == n:
        raise ValueError("mark_packed: the arrays hold different numbers of entries")
    if weight is not None and qual_off is not None:
        raise ValueError("mark_packed: weights or quality strings, not both")
    ptr = lambda x: None if x is None else x.ctypes.data        # noqa: E731
    rid, weight = (None if x is None else np.ascontiguousarray(x, dtype=np.uint32) for x in (rid, weight))
    if any(x is not None and len(x) != n for x in (rid, weight)):
        raise ValueError("mark_packed: the arrays hold different numbers of entries")
    if qual_off is not None:
        qual_off = np.ascontiguousarray(qual_off, dtype=np.uint64)
        qual = np.ascontiguousarray(np.zeros(0, np.uint8) if qual is None else
                                    np.frombuffer(qual, np.uint8) if isinstance(qual, (bytes, bytearray)) else qual, dtype=np.uint8)
        if len(qual_off) != n + 1:
            raise ValueError("mark_packed: the arrays hold different numbers of entries")
        if n and int(qual_off[n]) > len(qual):
            raise ValueError("mark_packed: the offsets reach beyond the strings")
        if len(qual) == 0:
            qual = np.zeros(1, np.uint8)
    p = _CParams(int(bool(paired)), 0 if qual_off is None else 1, int(min_weight_qual), int(qual_offset))
    dup, rep, w, err = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rc = _lib.lib().polyhip_mark_duplicates(C.byref(p), n, flags.ctypes.data, ptr(rid), ref_start.ctypes.data, ref_end.ctypes.data,
                                            read_start.ctypes.data, read_end.ctypes.data, read_len.ctypes.data, ptr(weight),
                                            ptr(qual) if qual_off is not None else None, ptr(qual_off), w.ctypes.data, dup.ctypes.data,
                                            rep.ctypes.data, err.ctypes.data)
    _lib.check(rc)
    return Duplicates(dup, rep, w, err, int(rc))


def mark(result, read_len, paired: bool = False, weight=None, quals=None, qual_offsets=None, min_weight_qual: int = 15,
         qual_offset: int = 33) -> Duplicates:
    """The duplicates among the entries of a ``mapper.MapResult``.  ``read_len``: the length of every read (one number, or
    one per entry; for pairs in the result's order 2i, 2i + 1).  ``paired``: the entries are mates (2i, 2i + 1), as
    ``mapper.map_pairs_packed`` returns them.  ``quals`` / ``qual_offsets``: as ``fastq.pack_qual`` returns them, in the
    result's entry order.  A result of a refs call brings its contigs (``result.rid``) along."""
    return mark_packed(result.flags, result.ref_start, result.ref_end, result.read_start, result.read_end, read_len,
                       getattr(result, "rid", None), paired, weight, quals, qual_offsets, min_weight_qual, qual_offset)


def coord_order_packed(sam_flag, ref_start, rid=None, paired: bool = False) -> np.ndarray:
    """polyhip_coord_order on packed arrays: the stable permutation into SAM's coordinate order"""
    n = len(sam_flag)
    sam_flag, ref_start = (np.ascontiguousarray(x, dtype=np.uint32) for x in (sam_flag, ref_start))
    if rid is not None:
        rid = np.ascontiguousarray(rid, dtype=np.uint32)
    if len(ref_start) != n or (rid is not None and len(rid) != n):
        raise ValueError("coord_order_packed: the arrays hold different numbers of entries")
    order = np.zeros(n, np.uint32)
    _lib.check(_lib.lib().polyhip_coord_order(n, int(bool(paired)), sam_flag.ctypes.data, None if rid is None else rid.ctypes.data,
                                              ref_start.ctypes.data, order.ctypes.data))
    return order


def coord_order(records, result, paired: bool = False) -> np.ndarray:
    """The order ``sam.write`` / ``sam.write_refs`` take as ``order=`` for SO:coordinate: live entries by (contig, position),
    an entry that is not live beside its live mate, everything else last; ties in the result's order.  ``records``: the
    ``sam.AlnRecords`` of ``result``."""
    return coord_order_packed(records.sam_flag, result.ref_start, getattr(result, "rid", None), paired)
