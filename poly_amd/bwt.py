"""search/bwt of bebop/poly on MI355X.

Mirrors search/bwt/bwt.go: ``New`` (:455-517) and ``BWT`` with ``Count`` (:235-247), ``Locate`` (:249-273),
``Extract`` (:275-299), ``Len`` (:301-304) and ``GetTransform`` (:306-323), plus the batch forms a GPU needs
(``CountBatch``, ``LocateBatch``, ``ExtractBatch``), ``*_dev`` entry points on torch tensors, and the search with up to
four substitutions (``CountMismatch``, ``LocateMismatch`` and their batch forms).  The suffix array,
the last column and the occurrence structure are built and queried in HIP (polyhip_bwt_*); nothing is computed here.

Sequences and patterns are Go strings, i.e. bytes: a ``str`` is taken one byte per character (latin-1), and a BWT
built from a ``str`` returns ``str`` from ``Extract`` / ``GetTransform`` (``bytes`` otherwise).  Errors are raised
as ``ValueError`` with the reference's messages.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .mash import _pack

NULL_CHAR = b"$"
_EXTRACT_ERRORS = {
    1: lambda s, e, n: "Start must be strictly less than end",
    2: lambda s, e, n: f"end [{e}] exceeds the max range of the BWT [{n}]",
    3: lambda s, e, n: f"start [{s}] exceeds the min range of the BWT [0]",
}


def _bytes(s) -> bytes:
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def _validate_sequence(seq: bytes) -> None:
    """bwt.go:636-644, before any device call"""
    if len(seq) == 0:
        raise ValueError("Provided sequence must not by empty. BWT cannot be constructed")
    if NULL_CHAR in seq:
        raise ValueError("Provided sequence contains the nullChar $. BWT cannot be constructed")


class BWT:
    """bwt.go:188-200: a handle to the device-resident index (freed with the object)."""

    def __init__(self, handle: C.c_void_p, n: int, as_str: bool):
        self._handle = handle
        self._n = int(n)
        self._str = as_str

    def __del__(self):
        if getattr(self, "_handle", None) is not None:
            try:
                _lib.lib().polyhip_bwt_destroy(self._handle)
            except Exception:
                pass
            self._handle = None

    def _out(self, b: bytes):
        return b.decode("latin-1") if self._str else b

    # -- the reference's API ---------------------------------------------------------------------------------------------
    def Count(self, pattern) -> int:
        """bwt.go:235-247"""
        if len(pattern) == 0:
            raise ValueError("Pattern can not be empty")
        return int(self.CountBatch([pattern])[0])

    def Locate(self, pattern):
        """bwt.go:249-273: offsets in suffix-array row order (unsorted); None when there is no match"""
        if len(pattern) == 0:
            raise ValueError("Pattern can not be empty")
        first, offsets = self.LocateBatch([pattern])
        return None if first[1] == 0 else [int(x) for x in offsets]

    def Extract(self, start: int, end: int):
        """bwt.go:275-299"""
        return self.ExtractBatch([(start, end)])[0]

    def Len(self) -> int:
        """bwt.go:301-304"""
        return self._n

    def GetTransform(self):
        """bwt.go:306-323: the last column, '$' included"""
        out = np.zeros(self._n + 1, dtype=np.uint8)
        _lib.check(_lib.lib().polyhip_bwt_transform(self._handle, out.ctypes.data))
        return self._out(out.tobytes())

    # -- batches ---------------------------------------------------------------------------------------------------------
    def Intervals(self, patterns):
        """(start uint32[n], end uint32[n], err uint32[n]): the rows [start, end) that begin with each pattern;
        err = 1 marks an empty pattern"""
        buf, offs = _pack(patterns)
        return self.intervals_packed(buf, offs)

    def intervals_packed(self, buf: np.ndarray, offs: np.ndarray):
        n = len(offs) - 1
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        start = np.zeros(n, np.uint32)
        end = np.zeros(n, np.uint32)
        err = np.zeros(n, np.uint32)
        _lib.check(_lib.lib().polyhip_bwt_count(self._handle, buf.ctypes.data, offs.ctypes.data, n, start.ctypes.data,
                                                end.ctypes.data, err.ctypes.data))
        return start, end, err

    def CountBatch(self, patterns) -> np.ndarray:
        """Count of every pattern (int64); an empty pattern raises, as Count does"""
        start, end, err = self.Intervals(patterns)
        if err.any():
            raise ValueError("Pattern can not be empty")
        return end.astype(np.int64) - start.astype(np.int64)

    def LocateBatch(self, patterns, capacity: int | None = None):
        """(first uint64[n+1], offsets uint32[first[n]]): pattern p's offsets are offsets[first[p]:first[p+1]], in row
        order.  ``capacity`` (default: exactly what is needed, from a Count pass) sizes the output buffer."""
        buf, offs = _pack(patterns)
        return self.locate_packed(buf, offs, capacity)

    def locate_packed(self, buf: np.ndarray, offs: np.ndarray, capacity: int | None = None):
        n = len(offs) - 1
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        if capacity is None:
            start, end, err = self.intervals_packed(buf, offs)
            if err.any():
                raise ValueError("Pattern can not be empty")
            capacity = int((end.astype(np.int64) - start.astype(np.int64)).sum())
        first = np.zeros(n + 1, np.uint64)
        out = np.zeros(max(int(capacity), 1), np.uint32)
        err = np.zeros(n, np.uint32)
        _lib.check(_lib.lib().polyhip_bwt_locate(self._handle, buf.ctypes.data, offs.ctypes.data, n, first.ctypes.data,
                                                 out.ctypes.data, int(capacity), err.ctypes.data))
        if err.any():
            raise ValueError("Pattern can not be empty")
        return first, out[: int(first[n])]

    # -- with mismatches (polyhip_bwt_*_mismatch: substitutions only, matches inside the sequence) ---------------------------
    def count_mismatch_packed(self, buf: np.ndarray, offs: np.ndarray, k: int):
        """(counts uint32[n, k + 1], err uint32[n]): counts[p, d] = positions where pattern p has exactly d mismatches;
        err = 1 marks an empty pattern"""
        n = len(offs) - 1
        k = int(k)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        counts = np.zeros((n, max(k, 0) + 1), np.uint32)
        err = np.zeros(n, np.uint32)
        _lib.check(_lib.lib().polyhip_bwt_count_mismatch(self._handle, buf.ctypes.data, offs.ctypes.data, n, k, counts.ctypes.data,
                                                         err.ctypes.data))
        return counts, err

    def CountMismatchBatch(self, patterns, k: int) -> np.ndarray:
        """int64[n, k + 1]: per pattern, the positions at Hamming distance exactly 0..k; an empty pattern raises"""
        counts, err = self.count_mismatch_packed(*_pack(patterns), k)
        if err.any():
            raise ValueError("Pattern can not be empty")
        return counts.astype(np.int64)

    def CountMismatch(self, pattern, k: int) -> np.ndarray:
        if len(pattern) == 0:
            raise ValueError("Pattern can not be empty")
        return self.CountMismatchBatch([pattern], k)[0]

    def locate_mismatch_packed(self, buf: np.ndarray, offs: np.ndarray, k: int, capacity: int | None = None):
        """(first uint64[n + 1], pos uint32[], mm uint8[], err uint32[n])"""
        n = len(offs) - 1
        k = int(k)
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        if capacity is None:
            capacity = int(self.count_mismatch_packed(buf, offs, k)[0].sum(dtype=np.uint64))
        first = np.zeros(n + 1, np.uint64)
        pos = np.zeros(max(int(capacity), 1), np.uint32)
        mm = np.zeros(max(int(capacity), 1), np.uint8)
        err = np.zeros(n, np.uint32)
        _lib.check(_lib.lib().polyhip_bwt_locate_mismatch(self._handle, buf.ctypes.data, offs.ctypes.data, n, k, first.ctypes.data,
                                                          pos.ctypes.data, mm.ctypes.data, int(capacity), err.ctypes.data))
        total = int(first[n])
        return first, pos[:total], mm[:total], err

    def LocateMismatchBatch(self, patterns, k: int, capacity: int | None = None):
        """(first uint64[n + 1], pos uint32[first[n]], mm uint8[first[n]]): pattern p's hits are pos[first[p]:first[p + 1]],
        ascending, with their mismatches in mm.  ``capacity`` (default: what a count pass says is needed) sizes the buffers."""
        first, pos, mm, err = self.locate_mismatch_packed(*_pack(patterns), k, capacity)
        if err.any():
            raise ValueError("Pattern can not be empty")
        return first, pos, mm

    def LocateMismatch(self, pattern, k: int):
        """[(position, mismatches)] ascending by position; None when there is no hit, as Locate"""
        if len(pattern) == 0:
            raise ValueError("Pattern can not be empty")
        first, pos, mm = self.LocateMismatchBatch([pattern], k)
        return None if first[1] == 0 else [(int(a), int(b)) for a, b in zip(pos, mm)]

    def MismatchInfo(self) -> dict:
        """polyhip_bwt_mismatch_last_info: the calling thread's last mismatch call"""
        info = (C.c_uint64 * 5)()
        _lib.check(_lib.lib().polyhip_bwt_mismatch_last_info(C.addressof(info)))
        return dict(zip(("patterns", "nodes", "occ_lines", "leaves", "hits"), (int(v) for v in info)))

    def extract_raw(self, requests):
        """(bytes per request or None, err uint32[n]) with err = 0 or the reference's failing check (1, 2, 3)"""
        s = np.ascontiguousarray([int(a) for a, _ in requests], dtype=np.int64)
        e = np.ascontiguousarray([int(b) for _, b in requests], dtype=np.int64)
        ok = (s < e) & (e <= self._n) & (s >= 0)
        w = np.where(ok, e - s, 0).astype(np.uint64)
        off = np.zeros(len(requests) + 1, np.uint64)
        off[1:] = np.cumsum(w, dtype=np.uint64)
        out = np.zeros(max(int(off[-1]), 1), np.uint8)
        err = np.zeros(len(requests), np.uint32)
        _lib.check(_lib.lib().polyhip_bwt_extract(self._handle, s.ctypes.data, e.ctypes.data, len(requests), off.ctypes.data,
                                                  out.ctypes.data, err.ctypes.data))
        res = [None if err[i] else out[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(requests))]
        return res, err

    def ExtractBatch(self, requests):
        """Extract of every (start, end); the first failing request raises with the reference's message"""
        res, err = self.extract_raw(requests)
        for (a, b), r, c in zip(requests, res, err):
            if c:
                raise ValueError(_EXTRACT_ERRORS[int(c)](int(a), int(b), self._n))
        return [self._out(r) for r in res]

    # -- introspection ---------------------------------------------------------------------------------------------------
    def SuffixArray(self) -> np.ndarray:
        out = np.zeros(self._n + 1, np.uint32)
        _lib.check(_lib.lib().polyhip_bwt_suffix_array(self._handle, out.ctypes.data))
        return out

    def Layout(self) -> str:
        return ("nucleotide", "general")[_lib.lib().polyhip_bwt_layout(self._handle)]

    def Rounds(self) -> int:
        return int(_lib.lib().polyhip_bwt_rounds(self._handle))

    def handle(self):
        return self._handle


def New(sequence) -> BWT:
    """bwt.go:455-517"""
    as_str = isinstance(sequence, str)
    seq = _bytes(sequence)
    _validate_sequence(seq)
    buf = np.frombuffer(seq, dtype=np.uint8)
    h = C.c_void_p()
    _lib.check(_lib.lib().polyhip_bwt_create(buf.ctypes.data, len(seq), C.byref(h)))
    return BWT(h, len(seq), as_str)


# ---- device-resident entry points (torch CUDA tensors) -------------------------------------------------------------------
def workspace_bytes(n: int) -> int:
    return int(_lib.lib().polyhip_bwt_workspace_bytes(int(n)))


def new_dev(seq_t, work_t=None, stream=None) -> BWT:
    """Build from a device uint8 tensor (no '$'); ``work_t`` >= workspace_bytes(n) bytes (allocated if omitted)."""
    import torch
    n = seq_t.numel()
    if n == 0:
        raise ValueError("Provided sequence must not by empty. BWT cannot be constructed")
    if work_t is None:
        work_t = torch.empty(workspace_bytes(n), dtype=torch.uint8, device=seq_t.device)
    h = C.c_void_p()
    status = _lib.lib().polyhip_bwt_create_dev(seq_t.data_ptr(), n, work_t.data_ptr(), work_t.numel() * work_t.element_size(),
                                               _lib.stream_ptr(stream), C.byref(h))
    if status == _lib.ERR_INVALID:
        raise ValueError(_lib.lib().polyhip_last_error().decode("utf-8", "replace"))
    _lib.check(status)
    return BWT(h, n, False)


def count_dev(index: BWT, pat_t, off_t, start_t, end_t, err_t, stream=None) -> None:
    n = off_t.numel() - 1
    _lib.check(_lib.lib().polyhip_bwt_count_dev(index.handle(), pat_t.data_ptr(), off_t.data_ptr(), n, start_t.data_ptr(),
                                                end_t.data_ptr(), err_t.data_ptr(), _lib.stream_ptr(stream)))


def locate_workspace_bytes(npat: int) -> int:
    return int(_lib.lib().polyhip_bwt_locate_workspace_bytes(int(npat)))


def locate_dev(index: BWT, start_t, end_t, first_t, out_t, work_t=None, stream=None) -> None:
    """first_t: uint64-sized (torch.int64) [n+1]; out_t: uint32-sized (torch.int32) with its capacity = numel()"""
    import torch
    n = start_t.numel()
    wb = locate_workspace_bytes(n)
    if work_t is None:
        work_t = torch.empty(max(wb, 1), dtype=torch.uint8, device=start_t.device)
    _lib.check(_lib.lib().polyhip_bwt_locate_dev(index.handle(), start_t.data_ptr(), end_t.data_ptr(), n, first_t.data_ptr(),
                                                 out_t.data_ptr() if out_t.numel() else None, out_t.numel(), work_t.data_ptr(),
                                                 work_t.numel(), _lib.stream_ptr(stream)))


def extract_dev(index: BWT, start_t, end_t, out_off_t, out_t, err_t, stream=None) -> None:
    n = start_t.numel()
    _lib.check(_lib.lib().polyhip_bwt_extract_dev(index.handle(), start_t.data_ptr(), end_t.data_ptr(), n, out_off_t.data_ptr(),
                                                  out_t.data_ptr(), err_t.data_ptr(), _lib.stream_ptr(stream)))


def transform_dev(index: BWT, out_t, stream=None) -> None:
    _lib.check(_lib.lib().polyhip_bwt_transform_dev(index.handle(), out_t.data_ptr(), _lib.stream_ptr(stream)))
