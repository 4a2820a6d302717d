"""Read trimming before the mapper (polyhip_trim_reads, polyhip_trim_pairs): low-quality ends, 3' adapters and, for pairs, the
overlap of two mates whose insert is shorter than the reads.

The definition is the comment above ``polyhip_trim_reads`` in include/polyhip.h and tests/trim_oracle.py restates it on the CPU.
The decisions, the offsets and the trimmed batch are computed in HIP from the packed batch ``fastq.pack_qual`` returns; nothing
is computed here.  No read is removed: an emptied read has length 0 in the output, so pairs, ``rec_start`` and every later stage
keep their indices, and the mappers report it as unmapped.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib, fastq

FLAG_QUAL_3P, FLAG_QUAL_5P, FLAG_ADAPTER, FLAG_SHORT, FLAG_OVERLAP = 1, 2, 4, 8, 16


class _CParams(C.Structure):
    _fields_ = [("qual_offset", C.c_uint32), ("min_qual_5p", C.c_uint32), ("min_qual_3p", C.c_uint32), ("adapter_err_pct", C.c_uint32),
                ("min_overlap", C.c_uint32), ("min_len", C.c_uint32), ("pair_min_overlap", C.c_uint32), ("pair_err_pct", C.c_uint32)]


class _CInfo(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64), ("cut_3p", C.c_uint64),
                ("cut_5p", C.c_uint64), ("adapter_hits", C.c_uint64), ("overlap_cut", C.c_uint64), ("too_short", C.c_uint64),
                ("bad", C.c_uint64)]


@dataclass
class TrimParams:
    """polyhip_trim_params.  The defaults switch every step off."""
    qual_offset: int = 33
    min_qual_5p: int = 0
    min_qual_3p: int = 0
    adapter_err_pct: int = 10
    min_overlap: int = 3
    min_len: int = 0
    pair_min_overlap: int = 0
    pair_err_pct: int = 10

    def _c(self) -> _CParams:
        return _CParams(*(int(getattr(self, name)) for name, _ in _CParams._fields_))


def last_info() -> dict:
    """polyhip_trim_last_info: what the calling thread's last ``trim_packed`` / ``trim_pairs_packed`` did"""
    info = _CInfo()
    _lib.check(_lib.lib().polyhip_trim_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CInfo._fields_}


@dataclass
class Trimmed:
    """The trimmed batch (``seqs``, ``offsets``, and ``quals`` under the same offsets, None without qualities) and one value per
    entry: ``start`` and ``end`` of what was kept, ``flags`` and ``err`` as the header numbers them.  For pairs ``seqs``,
    ``offsets`` and ``quals`` are two-item tuples, one per mate, and the entries are 2i (mate 1) and 2i + 1 (mate 2)."""
    seqs: object
    offsets: object
    quals: object
    start: np.ndarray
    end: np.ndarray
    flags: np.ndarray
    err: np.ndarray

    last_info = staticmethod(last_info)


def _bytes(x) -> np.ndarray:
    return np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray, memoryview)) else np.ascontiguousarray(x, dtype=np.uint8)


def _pack_adapters(adapters):
    adapters = [a.encode("ascii") if isinstance(a, str) else bytes(a) for a in (adapters or [])]
    off = np.zeros(len(adapters) + 1, np.uint32)
    off[1:] = np.cumsum([len(a) for a in adapters], dtype=np.uint64)
    return np.frombuffer(b"".join(adapters) + b"\0", np.uint8), off, len(adapters)


class _Batch:
    """one batch's arrays in the shapes the call wants, and buffers for its output"""

    def __init__(self, who: str, buf, offs, quals, qual_offs):
        if (quals is None) != (qual_offs is None):
            raise ValueError(f"{who}: quals and qual_offsets come together or not at all")
        self.offs = np.ascontiguousarray(offs, dtype=np.uint64)
        self.n = len(self.offs) - 1
        if self.n < 0:
            raise ValueError(f"{who}: offsets hold n + 1 entries")
        self.buf = _bytes(buf)
        if self.n and int(self.offs[self.n]) > len(self.buf):
            raise ValueError(f"{who}: the offsets reach beyond the bytes")
        self.quals = self.qoffs = self.out_quals = None
        if quals is not None:
            self.qoffs = np.ascontiguousarray(qual_offs, dtype=np.uint64)
            if len(self.qoffs) != self.n + 1:
                raise ValueError(f"{who}: the batches hold different numbers of reads")
            self.quals = _bytes(quals)
            if self.n and int(self.qoffs[self.n]) > len(self.quals):
                raise ValueError(f"{who}: the offsets reach beyond the bytes")
            if len(self.quals) == 0:
                self.quals = np.zeros(1, np.uint8)
        if len(self.buf) == 0:
            self.buf = np.zeros(1, np.uint8)
        total = int(self.offs[self.n]) - int(self.offs[0]) if self.n and int(self.offs[self.n]) >= int(self.offs[0]) else 0
        self.out = np.zeros(max(total, 1), np.uint8)
        if quals is not None:
            self.out_quals = np.zeros(max(total, 1), np.uint8)
        self.out_offs = np.zeros(self.n + 1, np.uint64)

    def inputs(self):
        p = lambda x: None if x is None else x.ctypes.data        # noqa: E731
        return self.buf.ctypes.data, self.offs.ctypes.data, p(self.quals), p(self.qoffs)

    def outputs(self):
        return self.out.ctypes.data, None if self.out_quals is None else self.out_quals.ctypes.data, self.out_offs.ctypes.data

    def result(self):
        kept = int(self.out_offs[self.n])
        return self.out[:kept], self.out_offs, None if self.out_quals is None else self.out_quals[:kept]


def trim_packed(buf, offs, quals=None, qual_offs=None, adapters=None, params: TrimParams | None = None) -> Trimmed:
    """polyhip_trim_reads on a packed batch: ``buf`` / ``offs`` as the mappers take them, ``quals`` / ``qual_offs`` as
    ``fastq.pack_qual`` returns them (or neither), ``adapters`` a list of upper-case ACGT strings."""
    b = _Batch("trim_packed", buf, offs, quals, qual_offs)
    ad, ad_off, nad = _pack_adapters(adapters)
    p = (params or TrimParams())._c()
    start, end, flags, err = (np.zeros(b.n, np.uint32) for _ in range(4))
    _lib.check(_lib.lib().polyhip_trim_reads(C.byref(p), ad.ctypes.data, ad_off.ctypes.data, nad, *b.inputs(), b.n, start.ctypes.data,
                                             end.ctypes.data, flags.ctypes.data, err.ctypes.data, *b.outputs()))
    seqs, out_offs, out_quals = b.result()
    return Trimmed(seqs, out_offs, out_quals, start, end, flags, err)


def trim_pairs_packed(buf1, offs1, buf2, offs2, quals1=None, qual_offs1=None, quals2=None, qual_offs2=None, adapters=None,
                      params: TrimParams | None = None) -> Trimmed:
    """polyhip_trim_pairs: mate i of (buf1, offs1) with mate i of (buf2, offs2).  ``seqs``, ``offsets`` and ``quals`` of the
    result are (mate 1's, mate 2's); ``start`` / ``end`` / ``flags`` / ``err`` have 2n entries, 2i for mate 1 and 2i + 1 for
    mate 2, as ``mapper.map_pairs_packed`` orders its result."""
    b1 = _Batch("trim_pairs_packed", buf1, offs1, quals1, qual_offs1)
    b2 = _Batch("trim_pairs_packed", buf2, offs2, quals2, qual_offs2)
    if b1.n != b2.n:
        raise ValueError("trim_pairs_packed: the two batches hold different numbers of reads")
    ad, ad_off, nad = _pack_adapters(adapters)
    p = (params or TrimParams())._c()
    start, end, flags, err = (np.zeros(2 * b1.n, np.uint32) for _ in range(4))
    _lib.check(_lib.lib().polyhip_trim_pairs(C.byref(p), ad.ctypes.data, ad_off.ctypes.data, nad, *b1.inputs(), *b2.inputs(), b1.n,
                                             start.ctypes.data, end.ctypes.data, flags.ctypes.data, err.ctypes.data, *b1.outputs(),
                                             *b2.outputs()))
    r1, r2 = b1.result(), b2.result()
    return Trimmed((r1[0], r2[0]), (r1[1], r2[1]), (r1[2], r2[2]), start, end, flags, err)


def trim_fastq(data, adapters=None, params: TrimParams | None = None, max_records: int | None = None):
    """``fastq.pack_qual`` followed by ``trim_packed``: FASTQ bytes -> (Trimmed, rec_start, parse error | None).  Like ParseN,
    the records before the first bad one are trimmed and returned together with the error."""
    seqs, offs, quals, qoffs, rec, perr = fastq.pack_qual(data, max_records)
    return trim_packed(seqs, offs, quals, qoffs, adapters, params), rec, perr
