"""Read mapping on MI355X: FM-index seeds (poly_amd.bwt), diagonal clusters, SmithWaterman extension (poly_amd.align).

The reference has no mapper; the definition is the comment above ``polyhip_map_reads`` in include/polyhip.h and
tests/map_oracle.py restates it on the CPU.  Everything is computed in HIP (polyhip_map_*); nothing is computed here.

Reads are Go strings, i.e. bytes: a ``str`` is taken one byte per character (latin-1), and ``MapReads`` returns aligned
strings as ``str`` when the reads were ``str`` (``bytes`` otherwise), as poly_amd.bwt does.

What tools downstream of a mapper read -- CIGAR, NM, MD, a mapping quality, the SAM FLAG word, SAM text -- is made from a
``MapResult`` by poly_amd.sam (``sam.records``, ``sam.write``; polyhip_aln_records), a pass over the arrays and strings
returned here.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .mash import _pack

FLAG_MAPPED, FLAG_REVERSE = 1, 2


class _CParams(C.Structure):
    _fields_ = [("seed_len", C.c_uint32), ("seed_stride", C.c_uint32), ("max_occ", C.c_uint32), ("band", C.c_uint32),
                ("max_cand", C.c_uint32), ("both_strands", C.c_uint32), ("min_score", C.c_int64)]


class _CInfo(C.Structure):
    _fields_ = [("seeds", C.c_uint64), ("seeds_over_max_occ", C.c_uint64), ("hits", C.c_uint64), ("clusters", C.c_uint64),
                ("pairs_aligned", C.c_uint64), ("reads_mapped", C.c_uint64), ("chunks", C.c_uint32)]


class _CAffineInfo(C.Structure):
    _fields_ = [("seeds", C.c_uint64), ("seeds_over_max_occ", C.c_uint64), ("hits", C.c_uint64), ("clusters", C.c_uint64),
                ("pairs_aligned", C.c_uint64), ("reads_mapped", C.c_uint64), ("pairs_traced", C.c_uint64), ("tb_cells", C.c_uint64),
                ("chunks", C.c_uint32), ("tb_chunks", C.c_uint32)]


@dataclass
class MapParams:
    """polyhip_map_params.  The defaults are unmeasured: they are what short-read mappers commonly start from, not the
    result of a sweep on this hardware."""
    seed_len: int = 20
    seed_stride: int = 10
    max_occ: int = 32
    band: int = 24
    max_cand: int = 4
    both_strands: bool = True
    min_score: int = 1

    def _c(self) -> _CParams:
        return _CParams(int(self.seed_len), int(self.seed_stride), int(self.max_occ), int(self.band), int(self.max_cand),
                        1 if self.both_strands else 0, int(self.min_score))


@dataclass
class MapResult:
    """one entry per read; ``alignA[i]`` / ``alignB[i]`` are bytes (None when no strings were asked for)"""
    score: np.ndarray
    second: np.ndarray
    flags: np.ndarray
    votes: np.ndarray
    ref_start: np.ndarray
    ref_end: np.ndarray
    read_start: np.ndarray
    read_end: np.ndarray
    err: np.ndarray
    alignA: list | None
    alignB: list | None
    aln_off: np.ndarray | None = None
    status: int = 0
    tlen: np.ndarray | None = None      # map_pairs_packed only: one entry per pair
    rid: np.ndarray | None = None       # the refs calls only: the contig of every entry (ref_start / ref_end are local to it)


@dataclass
class MapRecord:
    mapped: bool
    reverse: bool
    score: int
    second: int
    votes: int
    ref_start: int
    ref_end: int
    read_start: int
    read_end: int
    alignA: object
    alignB: object
    err: int
    rid: int = 0


def _strings_short() -> bool:
    """the last ERR_INVALID was the one about the strings' capacity (everything else was delivered)"""
    return b"aligned strings need" in _lib.lib().polyhip_last_error()


def last_info() -> dict:
    """polyhip_map_last_info: what the calling thread's last call did"""
    info = _CInfo()
    _lib.check(_lib.lib().polyhip_map_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CInfo._fields_}


def workspace_bytes(index, scoring, params: MapParams, nreads: int, max_len: int) -> int:
    p = params._c()
    return int(_lib.lib().polyhip_map_workspace_bytes(index.handle(), scoring.handle(), C.byref(p), int(nreads), int(max_len)))


def _packed(call, buf: np.ndarray, offs: np.ndarray, params: MapParams | None, strings: bool, capacity: int | None,
            max_len: int | None, per_read: int = 1, with_rid: bool = False) -> MapResult:
    """what the host-pointer entry points share: the output arrays, the retry with the exact string capacity, the strings as
    lists.  call(params, reads, offs, n, max_len, *outputs, capacity) -> status.  per_read: output entries per read of
    ``offs`` (2 for pairs, whose second batch the caller holds).  with_rid: the outputs hold ``rid`` before ``ref_start``
    (the refs calls)"""
    params = params or MapParams()
    nin = len(offs) - 1
    n = nin * per_read
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    if max_len is None:
        max_len = int(np.diff(offs.astype(np.int64)).max()) if n else 0
    p = params._c()
    score, second = np.zeros(n, np.int64), np.zeros(n, np.int64)
    u32 = [np.zeros(n, np.uint32) for _ in range(7)]
    rid = np.zeros(n, np.uint32) if with_rid else None
    outs = u32[:2] + ([rid] if with_rid else []) + u32[2:]
    off = np.zeros(n + 1, np.uint64)
    cap = int(capacity) if capacity is not None else int(int(offs[nin] - offs[0]) * 1.25 * per_read) + (64 << 10)
    alnA = alnB = None
    rc = _lib.OK
    for _ in range(2):
        if strings:
            alnA, alnB = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        rc = call(C.byref(p), buf.ctypes.data, offs.ctypes.data, nin, int(max_len),
                  score.ctypes.data, second.ctypes.data, *[a.ctypes.data for a in outs],
                  alnA.ctypes.data if strings else None, alnB.ctypes.data if strings else None, off.ctypes.data if strings else None, cap)
        if strings and rc == _lib.ERR_INVALID and _strings_short():  # the strings did not fit: off[n] says what they need
            if capacity is not None:
                break
            cap = int(off[n])
            continue
        _lib.check(rc)
        break
    sa = sb = None
    if strings and rc == _lib.OK:
        o = off.astype(np.int64)
        sa = [alnA[o[i]:o[i + 1]].tobytes() for i in range(n)]
        sb = [alnB[o[i]:o[i + 1]].tobytes() for i in range(n)]
    return MapResult(score, second, *u32, sa, sb, off if strings else None, int(rc), rid=rid)


def map_reads_packed(index, scoring, buf: np.ndarray, offs: np.ndarray, params: MapParams | None = None, strings: bool = True,
                     capacity: int | None = None, max_len: int | None = None) -> MapResult:
    """Host-pointer entry point on a packed batch.  ``capacity`` bytes per string buffer (default: 1.25 x the reads' bytes
    + 64 KB; a batch that needs more is run again with the exact size -- unless ``capacity`` was given, in which case the
    result carries ``status`` = ERR_INVALID, ``aln_off[-1]`` = the bytes needed, and no strings)."""
    def call(p, *rest):
        return _lib.lib().polyhip_map_reads(index.handle(), scoring.handle(), p, *rest)
    return _packed(call, buf, offs, params, strings, capacity, max_len)


def MapReads(index, scoring, reads, params: MapParams | None = None) -> list:
    """Every read of a list placed on the index's text -> list of MapRecord"""
    as_str = bool(reads) and all(isinstance(r, str) for r in reads)
    buf, offs = _pack(reads)
    r = map_reads_packed(index, scoring, buf, offs, params)
    conv = (lambda b: b.decode("latin-1")) if as_str else (lambda b: b)
    return [MapRecord(bool(r.flags[i] & FLAG_MAPPED), bool(r.flags[i] & FLAG_REVERSE), int(r.score[i]), int(r.second[i]),
                      int(r.votes[i]), int(r.ref_start[i]), int(r.ref_end[i]), int(r.read_start[i]), int(r.read_end[i]),
                      conv(r.alignA[i]), conv(r.alignB[i]), int(r.err[i])) for i in range(len(reads))]


# ---- affine gaps in the extension (polyhip_map_reads_affine; host pointers only) ---------------------------------------------
def last_affine_info() -> dict:
    """polyhip_map_affine_last_info: what the calling thread's last affine call did"""
    info = _CAffineInfo()
    _lib.check(_lib.lib().polyhip_map_affine_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CAffineInfo._fields_}


def map_reads_affine_packed(index, scoring, gap_open: int, gap_extend: int, buf: np.ndarray, offs: np.ndarray,
                            params: MapParams | None = None, strings: bool = True, capacity: int | None = None,
                            max_len: int | None = None, work_limit: int = 0) -> MapResult:
    """map_reads_packed with Gotoh's affine gaps in the extension: the first symbol of a gap costs ``gap_open``, each
    further one ``gap_extend`` (added values, gap_open <= gap_extend <= -1; the scoring handle's own gap is ignored).
    ``work_limit``: the most device workspace in bytes (0: the default); ``capacity`` as in map_reads_packed."""
    def call(p, reads, off, n, max_len_, *rest):
        return _lib.lib().polyhip_map_reads_affine(index.handle(), scoring.handle(), p, int(gap_open), int(gap_extend), reads, off, n,
                                                   max_len_, int(work_limit), *rest)
    return _packed(call, buf, offs, params, strings, capacity, max_len)


def MapReadsAffine(index, scoring, reads, gap_open: int, gap_extend: int, params: MapParams | None = None) -> list:
    """MapReads with affine gaps in the extension -> list of MapRecord"""
    as_str = bool(reads) and all(isinstance(r, str) for r in reads)
    buf, offs = _pack(reads)
    r = map_reads_affine_packed(index, scoring, gap_open, gap_extend, buf, offs, params)
    conv = (lambda b: b.decode("latin-1")) if as_str else (lambda b: b)
    return [MapRecord(bool(r.flags[i] & FLAG_MAPPED), bool(r.flags[i] & FLAG_REVERSE), int(r.score[i]), int(r.second[i]),
                      int(r.votes[i]), int(r.ref_start[i]), int(r.ref_end[i]), int(r.read_start[i]), int(r.read_end[i]),
                      conv(r.alignA[i]), conv(r.alignB[i]), int(r.err[i])) for i in range(len(reads))]


# ---- paired-end reads (polyhip_map_pairs; host pointers only) ---------------------------------------------------------------
FLAG_PROPER, FLAG_RESCUED = 4, 8


class _CPairParams(C.Structure):
    _fields_ = [("min_insert", C.c_uint32), ("max_insert", C.c_uint32), ("rescue", C.c_uint32)]


class _CPairsInfo(C.Structure):
    _fields_ = [("seeds", C.c_uint64), ("seeds_over_max_occ", C.c_uint64), ("hits", C.c_uint64), ("clusters", C.c_uint64),
                ("pairs_aligned", C.c_uint64), ("reads_mapped", C.c_uint64), ("proper_pairs", C.c_uint64),
                ("rescue_attempts", C.c_uint64), ("rescued", C.c_uint64), ("pairs_traced", C.c_uint64), ("chunks", C.c_uint32)]


@dataclass
class PairParams:
    """polyhip_map_pair_params: the inserts (outer distance of a forward-reverse pair) that make a pair proper, and whether a
    mate without a placement of its own is searched for in the window its partner implies"""
    min_insert: int
    max_insert: int
    rescue: bool = True

    def _c(self) -> _CPairParams:
        return _CPairParams(int(self.min_insert), int(self.max_insert), int(self.rescue))


def last_pairs_info() -> dict:
    """polyhip_map_pairs_last_info: what the calling thread's last paired call did"""
    info = _CPairsInfo()
    _lib.check(_lib.lib().polyhip_map_pairs_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CPairsInfo._fields_}


def map_pairs_packed(index, scoring, gap_open: int, gap_extend: int, buf1: np.ndarray, offs1: np.ndarray, buf2: np.ndarray,
                     offs2: np.ndarray, params: MapParams | None = None, pair_params: PairParams | None = None, strings: bool = True,
                     capacity: int | None = None, max_len: int | None = None, work_limit: int = 0) -> MapResult:
    """Mate i of (buf1, offs1) with mate i of (buf2, offs2) -> a MapResult of 2n entries (2i: mate 1 of pair i, 2i + 1: mate
    2) whose ``tlen`` has one entry per pair: the insert of a proper pair, else 0.  ``pair_params`` is required; the other
    arguments are map_reads_affine_packed's."""
    if pair_params is None:
        raise ValueError("map_pairs_packed: pair_params is required")
    n = len(offs1) - 1
    if len(offs2) - 1 != n:
        raise ValueError("map_pairs_packed: the two batches hold different numbers of reads")
    buf2 = np.ascontiguousarray(buf2, dtype=np.uint8)
    offs2 = np.ascontiguousarray(offs2, dtype=np.uint64)
    if max_len is None:
        max_len = max((int(np.diff(o.astype(np.int64)).max()) for o in (np.asarray(offs1), offs2)), default=0) if n else 0
    pp = pair_params._c()
    tlen = np.zeros(n, np.int64)

    def call(p, reads, off, n_, max_len_, *rest):
        per_mate, tail = rest[:9], rest[9:]
        return _lib.lib().polyhip_map_pairs(index.handle(), scoring.handle(), p, C.byref(pp), int(gap_open), int(gap_extend), reads, off,
                                            buf2.ctypes.data, offs2.ctypes.data, n_, max_len_, int(work_limit), *per_mate,
                                            tlen.ctypes.data, *tail)
    r = _packed(call, buf1, offs1, params, strings, capacity, max_len, per_read=2)
    r.tlen = tlen
    return r


def MapPairs(index, scoring, reads1, reads2, gap_open: int, gap_extend: int, pair_params: PairParams,
             params: MapParams | None = None) -> list:
    """Every pair (reads1[i], reads2[i]) placed on the index's text -> list of (MapRecord, MapRecord, proper, tlen)"""
    if len(reads1) != len(reads2):
        raise ValueError("MapPairs: reads1 and reads2 differ in length")
    both = list(reads1) + list(reads2)
    as_str = bool(both) and all(isinstance(r, str) for r in both)
    buf1, offs1 = _pack(reads1)
    buf2, offs2 = _pack(reads2)
    r = map_pairs_packed(index, scoring, gap_open, gap_extend, buf1, offs1, buf2, offs2, params, pair_params)
    conv = (lambda b: b.decode("latin-1")) if as_str else (lambda b: b)

    def rec(i):
        return MapRecord(bool(r.flags[i] & FLAG_MAPPED), bool(r.flags[i] & FLAG_REVERSE), int(r.score[i]), int(r.second[i]),
                         int(r.votes[i]), int(r.ref_start[i]), int(r.ref_end[i]), int(r.read_start[i]), int(r.read_end[i]),
                         conv(r.alignA[i]), conv(r.alignB[i]), int(r.err[i]))
    return [(rec(2 * i), rec(2 * i + 1), bool(r.flags[2 * i] & FLAG_PROPER), int(r.tlen[i])) for i in range(len(reads1))]


# ---- a reference of several contigs (polyhip_map_reads_refs, polyhip_map_pairs_refs; host pointers only) -------------------
class _CRefsInfo(C.Structure):
    _fields_ = [("contigs", C.c_uint64), ("straddling", C.c_uint64)]


def last_refs_info() -> dict:
    """polyhip_map_refs_last_info: the contigs of the calling thread's last refs call and the seed occurrences it dropped
    because they straddle a boundary (the other counters are last_affine_info's / last_pairs_info's)"""
    info = _CRefsInfo()
    _lib.check(_lib.lib().polyhip_map_refs_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CRefsInfo._fields_}


def map_reads_refs_packed(refset, scoring, gap_open: int, gap_extend: int, buf: np.ndarray, offs: np.ndarray,
                          params: MapParams | None = None, strings: bool = True, capacity: int | None = None,
                          max_len: int | None = None, work_limit: int = 0) -> MapResult:
    """map_reads_affine_packed on a ``refs.RefSet``: no seed, cluster, window or alignment crosses a contig boundary;
    ``rid`` is every entry's contig and ``ref_start`` / ``ref_end`` are positions in it (gap_open == gap_extend: linear gaps)"""
    def call(p, reads, off, n, max_len_, *rest):
        return _lib.lib().polyhip_map_reads_refs(refset.handle(), scoring.handle(), p, int(gap_open), int(gap_extend), reads, off, n,
                                                 max_len_, int(work_limit), *rest)
    return _packed(call, buf, offs, params, strings, capacity, max_len, with_rid=True)


def _record(r: MapResult, i: int, conv) -> MapRecord:
    return MapRecord(bool(r.flags[i] & FLAG_MAPPED), bool(r.flags[i] & FLAG_REVERSE), int(r.score[i]), int(r.second[i]),
                     int(r.votes[i]), int(r.ref_start[i]), int(r.ref_end[i]), int(r.read_start[i]), int(r.read_end[i]),
                     conv(r.alignA[i]), conv(r.alignB[i]), int(r.err[i]), int(r.rid[i]))


def MapReadsRefs(refset, scoring, reads, gap_open: int, gap_extend: int, params: MapParams | None = None) -> list:
    """Every read of a list placed on the set -> list of MapRecord (``rid`` = the contig, ``refset.names[rid]`` its name)"""
    as_str = bool(reads) and all(isinstance(r, str) for r in reads)
    buf, offs = _pack(reads)
    r = map_reads_refs_packed(refset, scoring, gap_open, gap_extend, buf, offs, params)
    conv = (lambda b: b.decode("latin-1")) if as_str else (lambda b: b)
    return [_record(r, i, conv) for i in range(len(reads))]


def map_pairs_refs_packed(refset, scoring, gap_open: int, gap_extend: int, buf1: np.ndarray, offs1: np.ndarray, buf2: np.ndarray,
                          offs2: np.ndarray, params: MapParams | None = None, pair_params: PairParams | None = None,
                          strings: bool = True, capacity: int | None = None, max_len: int | None = None,
                          work_limit: int = 0) -> MapResult:
    """map_pairs_packed on a ``refs.RefSet``: a proper pair lies on one contig, a rescue window inside the anchor's"""
    if pair_params is None:
        raise ValueError("map_pairs_refs_packed: pair_params is required")
    n = len(offs1) - 1
    if len(offs2) - 1 != n:
        raise ValueError("map_pairs_refs_packed: the two batches hold different numbers of reads")
    buf2 = np.ascontiguousarray(buf2, dtype=np.uint8)
    offs2 = np.ascontiguousarray(offs2, dtype=np.uint64)
    if max_len is None:
        max_len = max((int(np.diff(o.astype(np.int64)).max()) for o in (np.asarray(offs1), offs2)), default=0) if n else 0
    pp = pair_params._c()
    tlen = np.zeros(n, np.int64)

    def call(p, reads, off, n_, max_len_, *rest):
        per_mate, tail = rest[:10], rest[10:]
        return _lib.lib().polyhip_map_pairs_refs(refset.handle(), scoring.handle(), p, C.byref(pp), int(gap_open), int(gap_extend),
                                                 reads, off, buf2.ctypes.data, offs2.ctypes.data, n_, max_len_, int(work_limit),
                                                 *per_mate, tlen.ctypes.data, *tail)
    r = _packed(call, buf1, offs1, params, strings, capacity, max_len, per_read=2, with_rid=True)
    r.tlen = tlen
    return r


def MapPairsRefs(refset, scoring, reads1, reads2, gap_open: int, gap_extend: int, pair_params: PairParams,
                 params: MapParams | None = None) -> list:
    """Every pair placed on the set -> list of (MapRecord, MapRecord, proper, tlen)"""
    if len(reads1) != len(reads2):
        raise ValueError("MapPairsRefs: reads1 and reads2 differ in length")
    both = list(reads1) + list(reads2)
    as_str = bool(both) and all(isinstance(r, str) for r in both)
    buf1, offs1 = _pack(reads1)
    buf2, offs2 = _pack(reads2)
    r = map_pairs_refs_packed(refset, scoring, gap_open, gap_extend, buf1, offs1, buf2, offs2, params, pair_params)
    conv = (lambda b: b.decode("latin-1")) if as_str else (lambda b: b)
    return [(_record(r, 2 * i, conv), _record(r, 2 * i + 1, conv), bool(r.flags[2 * i] & FLAG_PROPER), int(r.tlen[i]))
            for i in range(len(reads1))]


# ---- device-resident entry point (torch CUDA tensors) ---------------------------------------------------------------------
def map_reads_dev(index, scoring, reads_t, off_t, max_len: int, params: MapParams, score_t, second_t, flags_t, votes_t,
                  ref_start_t, ref_end_t, read_start_t, read_end_t, err_t, alnA_t=None, alnB_t=None, alnOff_t=None, work_t=None,
                  stream=None) -> int:
    """off_t: uint64-sized (torch.int64) [n + 1]; score / second: torch.int64 [n]; the others uint32-sized (torch.int32)
    [n]; alnA_t / alnB_t: uint8 of one capacity, alnOff_t [n + 1]; work_t: any size polyhip_map_workspace_bytes allows
    (allocated if omitted).  Returns the status: OK, or ERR_INVALID when only the strings' capacity was short
    (alnOff_t[n] = the bytes needed); everything else raises."""
    import torch
    n = off_t.numel() - 1
    if work_t is None:
        work_t = torch.empty(max(workspace_bytes(index, scoring, params, n, max_len), 1), dtype=torch.uint8, device=off_t.device)
    p = params._c()
    strings = alnA_t is not None
    rc = _lib.lib().polyhip_map_reads_dev(
        index.handle(), scoring.handle(), C.byref(p), reads_t.data_ptr(), off_t.data_ptr(), n, int(max_len),
        score_t.data_ptr(), second_t.data_ptr(), flags_t.data_ptr(), votes_t.data_ptr(), ref_start_t.data_ptr(),
        ref_end_t.data_ptr(), read_start_t.data_ptr(), read_end_t.data_ptr(), err_t.data_ptr(),
        alnA_t.data_ptr() if strings else None, alnB_t.data_ptr() if strings else None, alnOff_t.data_ptr() if strings else None,
        alnA_t.numel() if strings else 0, work_t.data_ptr(), work_t.numel() * work_t.element_size(), _lib.stream_ptr(stream))
    if rc == _lib.ERR_INVALID and strings and _strings_short():
        return int(rc)
    _lib.check(rc)
    return int(rc)
