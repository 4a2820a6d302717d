"""CPU oracle for search/bwt, written from the reference's semantics (not from its code):

- T = sequence + '$'; rows = T's rotations in sorted order, '$' lowest, every other byte by its unsigned value;
- GetTransform = the last column of those rows; Count(p) / Locate(p) = the rows whose rotation (repeated as often as
  needed) starts with p -- cyclic, so '$' inside p and p longer than T are meaningful; Locate lists SA[start:end) in
  row order.

Two independent constructions: brute force over the rotations (tiny texts) and prefix doubling with numpy's stable
argsort (up to megabases).  Intervals for patterns come from searchsorted over the rows' fixed-width cyclic prefixes.
"""
from __future__ import annotations

import numpy as np

NULL = 0x24  # '$'


def text(seq: bytes) -> bytes:
    return bytes(seq) + b"$"


def codes(T: bytes) -> np.ndarray:
    """'$' -> 0, the other bytes present -> 1, 2, ... in unsigned byte order"""
    t = np.frombuffer(T, dtype=np.uint8)
    present = np.zeros(256, bool)
    present[t] = True
    present[NULL] = False
    lut = np.zeros(256, np.int64)
    lut[present] = np.arange(1, int(present.sum()) + 1)
    return lut[t]


def suffix_array_brute(T: bytes) -> np.ndarray:
    c = codes(T).tolist()
    n = len(c)
    return np.array(sorted(range(n), key=lambda i: c[i:] + c[:i]), dtype=np.int64)


def suffix_array(T: bytes) -> np.ndarray:
    """prefix doubling: rank pairs sorted with a stable argsort until every rank is unique"""
    N = len(T)
    rank = codes(T) + 1  # >= 1; 0 stands for "past the end"
    k = 1
    while True:
        r2 = np.zeros(N, np.int64)
        if k < N:
            r2[: N - k] = rank[k:]
        key = rank * (N + 2) + r2
        sa = np.argsort(key, kind="stable")
        ks = key[sa]
        head = np.ones(N, np.int64)
        head[1:] = ks[1:] != ks[:-1]
        new = np.empty(N, np.int64)
        new[sa] = np.cumsum(head)
        rank = new
        if int(rank.max()) == N:
            return sa.astype(np.int64)
        k *= 2


def last_column(T: bytes, sa: np.ndarray) -> bytes:
    t = np.frombuffer(T, dtype=np.uint8)
    return t[(sa - 1) % len(t)].tobytes()


class Oracle:
    """The rows of T with their cyclic prefixes of width W, for intervals of patterns up to W bytes"""

    def __init__(self, seq: bytes, width: int = 32, sa: np.ndarray | None = None):
        self.seq = bytes(seq)
        self.T = text(self.seq)
        self.N = len(self.T)
        self.sa = suffix_array(self.T) if sa is None else sa
        self.width = width
        t = np.frombuffer(self.T, dtype=np.uint8)
        present = np.zeros(256, bool)
        present[t] = True
        present[NULL] = False
        self.lut = np.full(256, -1, np.int64)
        self.lut[NULL] = 0
        self.lut[present] = np.arange(1, int(present.sum()) + 1)
        c = self.lut[t].astype(np.uint8)  # <= 255 codes: '$' 0, bytes 1..255
        reps = -(-(self.N + width) // self.N)
        cyc = np.tile(c, reps)[: self.N + width]
        win = np.lib.stride_tricks.sliding_window_view(cyc, width)[self.sa]
        self.rows = np.ascontiguousarray(win).view(f"S{width}").ravel()

    def interval(self, p: bytes) -> tuple[int, int]:
        p = bytes(p)
        assert 0 < len(p) <= self.width
        cp = self.lut[np.frombuffer(p, np.uint8)]
        if (cp < 0).any():
            return 0, 0
        lo = np.zeros(self.width, np.uint8)
        hi = np.full(self.width, 0xFF, np.uint8)
        lo[: len(p)] = cp
        hi[: len(p)] = cp
        s = int(np.searchsorted(self.rows, lo.tobytes(), "left"))
        e = int(np.searchsorted(self.rows, hi.tobytes(), "right"))
        return (s, e) if s < e else (0, 0)

    def intervals_fixed(self, pats: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """vectorised interval of an (n, m) uint8 array of patterns, m <= width, every byte present in T"""
        n, m = pats.shape
        cp = self.lut[pats]
        assert (cp >= 0).all()
        lo = np.zeros((n, self.width), np.uint8)
        hi = np.full((n, self.width), 0xFF, np.uint8)
        lo[:, :m] = cp
        hi[:, :m] = cp
        s = np.searchsorted(self.rows, lo.view(f"S{self.width}").ravel(), "left")
        e = np.searchsorted(self.rows, hi.view(f"S{self.width}").ravel(), "right")
        empty = s >= e
        s[empty] = 0
        e[empty] = 0
        return s, e

    def count(self, p: bytes) -> int:
        s, e = self.interval(p)
        return e - s

    def locate(self, p: bytes) -> list[int]:
        s, e = self.interval(p)
        return [int(x) for x in self.sa[s:e]]

    def transform(self) -> bytes:
        return last_column(self.T, self.sa)


def interval_brute(seq: bytes, p: bytes) -> tuple[int, int]:
    """rows whose rotation, repeated, starts with p -- straight from the definition (tiny texts)"""
    T = text(seq)
    sa = suffix_array_brute(T)
    rows = []
    for i in sa:
        rot = T[i:] + T[:i]
        rot = rot * (len(p) // len(rot) + 1)
        rows.append(rot[: len(p)] == p)
    idx = [j for j, r in enumerate(rows) if r]
    if not idx:
        return 0, 0
    assert idx == list(range(idx[0], idx[-1] + 1)), "matching rows are not contiguous"
    return idx[0], idx[-1] + 1
