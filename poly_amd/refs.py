"""A reference of several contigs (polyhip_refs): one FM-index over their concatenation, and the contigs' starts in it.

The reference (bebop/poly) has nothing like it; the definition is the comment above ``polyhip_refs_create`` in
include/polyhip.h.  ``RefSet.index`` is the index of the concatenation C as a ``bwt.BWT`` that does not own its handle: Count
and Locate work on it as on any index and return positions in C, which ``resolve`` turns into (contig, local position) on
the device.  ``mapper.map_reads_refs_packed`` / ``map_pairs_refs_packed`` map reads onto the set with the contigs' boundaries
respected; ``sam.write_refs`` and ``pileup.pileup_refs`` take their results.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, bwt
from .mash import _pack


class _BorrowedBWT(bwt.BWT):
    """the set's index: the set owns the handle (and is kept alive by this view)"""

    def __init__(self, owner, handle, n: int, as_str: bool):
        super().__init__(handle, n, as_str)
        self._owner = owner

    def __del__(self):
        self._handle = None


class RefSet:
    """k named contigs.  ``names`` (str), ``lengths`` and ``starts`` (int64; ``starts[k]`` = the length of C)."""

    def __init__(self, handle, names, starts: np.ndarray, as_str: bool):
        self._handle = handle
        self.names = [n if isinstance(n, str) else bytes(n).decode("latin-1") for n in names]
        self.starts = starts.astype(np.int64)
        self.lengths = np.diff(self.starts)
        raw = _lib.lib().polyhip_refs_index(handle)
        self.index = _BorrowedBWT(self, C.c_void_p(raw), int(self.starts[-1]), as_str)

    def __del__(self):
        if getattr(self, "_handle", None) is not None:
            try:
                _lib.lib().polyhip_refs_destroy(self._handle)
            except Exception:
                pass
            self._handle = None

    def __len__(self) -> int:
        return len(self.names)

    def handle(self):
        return self._handle

    def text(self) -> bytes:
        """C, the contigs joined in order, read back from the index"""
        res, _ = self.index.extract_raw([(0, int(self.starts[-1]))])
        return res[0]

    def resolve(self, pos, length=None):
        """positions in C (what ``index.Locate`` returns), with ``length`` bytes each (one number, one per position, or None:
        1) -> (rid uint32[n], local uint32[n], err uint32[n]); err 1: the position is not in C, 2: the span runs past its
        contig's end"""
        pos = np.ascontiguousarray(pos, dtype=np.uint32)
        n = len(pos)
        ln = None if length is None else np.ascontiguousarray(np.broadcast_to(np.asarray(length, dtype=np.uint32), (n,)))
        rid, local, err = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        _lib.check(_lib.lib().polyhip_refs_resolve(self._handle, pos.ctypes.data, None if ln is None else ln.ctypes.data, n,
                                                   rid.ctypes.data, local.ctypes.data, err.ctypes.data))
        return rid, local, err


def new_packed(names, buf: np.ndarray, offs: np.ndarray, as_str: bool = False) -> RefSet:
    """the set of the packed batch (buf, offs): contig c is buf[offs[c]:offs[c + 1]]"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    k = len(offs) - 1
    if len(names) != k:
        raise ValueError("refs: the names and the sequences differ in number")
    h = C.c_void_p()
    if not len(buf):
        buf = np.zeros(1, np.uint8)       # an empty batch is refused for what it lacks, not for a null pointer
    _lib.check(_lib.lib().polyhip_refs_create(buf.ctypes.data, offs.ctypes.data, k, C.byref(h)))
    starts = np.zeros(k + 1, np.uint64)
    _lib.check(_lib.lib().polyhip_refs_starts(h, starts.ctypes.data))
    return RefSet(h, names, starts, as_str)


def New(names, seqs) -> RefSet:
    """contigs ``seqs`` (``str`` or ``bytes``) called ``names``"""
    seqs = list(seqs)
    as_str = bool(seqs) and all(isinstance(s, str) for s in seqs)
    buf, offs = _pack(seqs)
    return new_packed(list(names), buf, offs, as_str)


def from_fasta(data) -> RefSet:
    """every record of FASTA text, parsed on the device (``poly_amd.fasta``); a contig's name is its header up to the first
    blank"""
    from . import fasta
    recs = fasta.records(data)
    return New([name.split()[0].decode("latin-1") if name.split() else "" for name, _ in recs], [seq for _, seq in recs])
