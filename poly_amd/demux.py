"""Demultiplexing before the trimmer (polyhip_demux_reads, polyhip_demux_pairs): the inline 5' barcode of every read of a pooled
batch, and the batch grouped by sample.

The definition is the comment above ``polyhip_demux_reads`` in include/polyhip.h and tests/demux_oracle.py restates it on the CPU.
The barcodes, the samples, the order and the grouped batch are computed in HIP from the packed batch ``fastq.pack_qual`` returns;
nothing is computed here.  Sample k of the result is a contiguous run of reads of one batch: ``Demuxed.sample_batch(k)`` is a view
of it that ``trim.trim_packed`` and the mappers take as it is.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib, fastq
from .trim import _Batch

NONE = 0xFFFFFFFF
FLAG_NO_BARCODE, FLAG_AMBIGUOUS, FLAG_NOT_IN_SHEET = 1, 2, 4


class _CParams(C.Structure):
    _fields_ = [("max_shift", C.c_uint32), ("max_mismatches", C.c_uint32), ("min_margin", C.c_uint32), ("clip", C.c_uint32),
                ("clip_extra", C.c_uint32), ("nsamples", C.c_uint32)]


class _CInfo(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("assigned", C.c_uint64), ("exact", C.c_uint64), ("no_barcode", C.c_uint64),
                ("ambiguous", C.c_uint64), ("not_in_sheet", C.c_uint64), ("bad", C.c_uint64), ("bytes_in", C.c_uint64),
                ("bytes_out", C.c_uint64)]


@dataclass
class DemuxParams:
    """polyhip_demux_params without nsamples, which the calls take from the barcodes or the table."""
    max_shift: int = 0
    max_mismatches: int = 1
    min_margin: int = 1
    clip: int = 1
    clip_extra: int = 0

    def _c(self, nsamples: int) -> _CParams:
        return _CParams(int(self.max_shift), int(self.max_mismatches), int(self.min_margin), int(self.clip), int(self.clip_extra),
                        int(nsamples))


def last_info() -> dict:
    """polyhip_demux_last_info: what the calling thread's last ``demux_packed`` / ``demux_pairs_packed`` did"""
    info = _CInfo()
    _lib.check(_lib.lib().polyhip_demux_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CInfo._fields_}


@dataclass
class Demuxed:
    """The grouped batch (``seqs``, ``offsets``, and ``quals`` under the same offsets, None without qualities), ``order`` (output
    read j is input read ``order[j]``), ``sample_start`` (sample k is output reads ``sample_start[k]`` .. ``sample_start[k + 1]``,
    the unassigned are sample ``nsamples``), ``sample`` per read or pair and one value per entry: ``barcode``, ``bstart``,
    ``mism``, ``flags`` and ``err`` as the header numbers them.  For pairs ``seqs``, ``offsets`` and ``quals`` are two-item
    tuples, one per mate, and the entries are 2i (mate 1) and 2i + 1 (mate 2)."""
    seqs: object
    offsets: object
    quals: object
    nsamples: int
    barcode: np.ndarray
    bstart: np.ndarray
    mism: np.ndarray
    flags: np.ndarray
    err: np.ndarray
    sample: np.ndarray
    order: np.ndarray
    sample_start: np.ndarray

    last_info = staticmethod(last_info)

    def _slice(self, k: int):
        lo, hi = int(self.sample_start[k]), int(self.sample_start[k + 1])
        if isinstance(self.seqs, tuple):
            return tuple((s, o[lo:hi + 1], q) for s, o, q in zip(self.seqs, self.offsets, self.quals))
        return self.seqs, self.offsets[lo:hi + 1], self.quals

    def sample_batch(self, k: int):
        """sample k for the next stage: (seqs, the sample's slice of the offsets, quals) -- views, nothing is copied; for pairs
        one such triple per mate"""
        if not 0 <= k < self.nsamples:
            raise IndexError(f"sample {k} of {self.nsamples}")
        return self._slice(k)

    def unassigned(self):
        """the reads (pairs) without a sample, as ``sample_batch`` returns a sample"""
        return self._slice(self.nsamples)


def _pack_barcodes(barcodes):
    barcodes = [b.encode("ascii") if isinstance(b, str) else bytes(b) for b in (barcodes or [])]
    off = np.zeros(len(barcodes) + 1, np.uint32)
    off[1:] = np.cumsum([len(b) for b in barcodes], dtype=np.uint64)
    return np.frombuffer(b"".join(barcodes) + b"\0", np.uint8), off, len(barcodes)


def demux_packed(buf, offs, barcodes, quals=None, qual_offs=None, params: DemuxParams | None = None) -> Demuxed:
    """polyhip_demux_reads on a packed batch: ``buf`` / ``offs`` as the mappers take them, ``quals`` / ``qual_offs`` as
    ``fastq.pack_qual`` returns them (or neither), ``barcodes`` a list of upper-case ACGT strings: barcode k is sample k."""
    b = _Batch("demux_packed", buf, offs, quals, qual_offs)
    bc, bc_off, nbc = _pack_barcodes(barcodes)
    p = (params or DemuxParams())._c(nbc)
    barcode, bstart, mism, flags, err, sample, order = (np.zeros(b.n, np.uint32) for _ in range(7))
    starts = np.zeros(max(nbc, 1) + 2, np.uint64)
    _lib.check(_lib.lib().polyhip_demux_reads(C.byref(p), bc.ctypes.data, bc_off.ctypes.data, nbc, *b.inputs(), b.n, barcode.ctypes.data,
                                              bstart.ctypes.data, mism.ctypes.data, flags.ctypes.data, err.ctypes.data,
                                              sample.ctypes.data, order.ctypes.data, starts.ctypes.data, *b.outputs()))
    seqs, out_offs, out_quals = b.result()
    return Demuxed(seqs, out_offs, out_quals, nbc, barcode, bstart, mism, flags, err, sample, order, starts)


def demux_pairs_packed(buf1, offs1, buf2, offs2, barcodes1, barcodes2=None, pair_sample=None, nsamples: int | None = None, quals1=None,
                       qual_offs1=None, quals2=None, qual_offs2=None, params: DemuxParams | None = None) -> Demuxed:
    """polyhip_demux_pairs: mate i of (buf1, offs1) with mate i of (buf2, offs2).  Without ``barcodes2`` mate 1's barcode is the
    sample; with them ``pair_sample`` (len(barcodes1) x len(barcodes2), 0xFFFFFFFF for a combination that is not in the sheet)
    names the sample of every combination and ``nsamples`` says how many there are (default: the largest named one + 1)."""
    b1 = _Batch("demux_pairs_packed", buf1, offs1, quals1, qual_offs1)
    b2 = _Batch("demux_pairs_packed", buf2, offs2, quals2, qual_offs2)
    if b1.n != b2.n:
        raise ValueError("demux_pairs_packed: the two batches hold different numbers of reads")
    bc1, bc_off1, nbc1 = _pack_barcodes(barcodes1)
    bc2, bc_off2, nbc2 = _pack_barcodes(barcodes2)
    table = None
    if nbc2:
        if pair_sample is None:
            raise ValueError("demux_pairs_packed: two barcode sets need pair_sample")
        table = np.ascontiguousarray(pair_sample, dtype=np.uint32).reshape(-1)
        if len(table) != nbc1 * nbc2:
            raise ValueError("demux_pairs_packed: pair_sample holds len(barcodes1) x len(barcodes2) entries")
        if nsamples is None:
            named = table[table != NONE]
            nsamples = int(named.max()) + 1 if len(named) else 1
    elif nsamples is None:
        nsamples = nbc1
    p = (params or DemuxParams())._c(nsamples)
    barcode, bstart, mism, flags, err = (np.zeros(2 * b1.n, np.uint32) for _ in range(5))
    sample, order = np.zeros(b1.n, np.uint32), np.zeros(b1.n, np.uint32)
    starts = np.zeros(min(max(int(nsamples), 1), 65536) + 2, np.uint64)
    _lib.check(_lib.lib().polyhip_demux_pairs(C.byref(p), bc1.ctypes.data, bc_off1.ctypes.data, nbc1, bc2.ctypes.data, bc_off2.ctypes.data,
                                              nbc2, None if table is None else table.ctypes.data, *b1.inputs(), *b2.inputs(), b1.n,
                                              barcode.ctypes.data, bstart.ctypes.data, mism.ctypes.data, flags.ctypes.data,
                                              err.ctypes.data, sample.ctypes.data, order.ctypes.data, starts.ctypes.data, *b1.outputs(),
                                              *b2.outputs()))
    r1, r2 = b1.result(), b2.result()
    return Demuxed((r1[0], r2[0]), (r1[1], r2[1]), (r1[2], r2[2]), int(nsamples), barcode, bstart, mism, flags, err, sample, order, starts)


def demux_fastq(data, barcodes, params: DemuxParams | None = None, max_records: int | None = None):
    """``fastq.pack_qual`` followed by ``demux_packed``: FASTQ bytes -> (Demuxed, rec_start, parse error | None).  Like ParseN,
    the records before the first bad one are demultiplexed and returned together with the error."""
    seqs, offs, quals, qoffs, rec, perr = fastq.pack_qual(data, max_records)
    return demux_packed(seqs, offs, barcodes, quals, qoffs, params), rec, perr
