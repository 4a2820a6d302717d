"""Primer dimers (polyhip_primer_stack_dg, polyhip_primer_dimer_matrix, polyhip_primer_dimer_screen): which primers of a pool
bind each other, ranked by the stacking energy of their best ungapped Watson-Crick duplex -- over any run of pairs (``any``) and
over the runs that hold x's 3' base (``end``), the ones a polymerase can extend.

The definition is the comment above ``polyhip_primer_stack_dg`` in include/polyhip.h and tests/dimers_oracle.py restates it on
the CPU.  It is a ranking screen, not a Tm: no initiation, terminal-AT, dangling-end, loop or mismatch term.  The energies, the
partners and the counts are computed in HIP; nothing is computed here but ``render``, which is text for the eye.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .mash import _pack

NONE = 0xFFFFFFFF
MAX_PRIMER = 64


class _CParams(C.Structure):
    _fields_ = [("stack_dg", C.c_int32 * 16), ("any_threshold", C.c_int32), ("end_threshold", C.c_int32)]


class _CInfo(C.Structure):
    _fields_ = [("primers", C.c_uint64), ("bad", C.c_uint64), ("pairs", C.c_uint64), ("shifts", C.c_uint64), ("launches", C.c_uint64)]


def stack_dg(temp_c: float = 37.0) -> np.ndarray:
    """polyhip_primer_stack_dg: the 16 stacking energies (int32, cal/mol, AA AC AG AT CA ... TT) at ``temp_c`` degrees Celsius,
    taken to the millikelvin"""
    out = np.zeros(16, np.int32)
    _lib.check(_lib.lib().polyhip_primer_stack_dg(int(round((float(temp_c) + 273.15) * 1000)), out.ctypes.data))
    return out


def last_info() -> dict:
    """polyhip_primer_dimer_last_info: what the calling thread's last matrix or screen call did"""
    info = _CInfo()
    _lib.check(_lib.lib().polyhip_primer_dimer_last_info(C.byref(info)))
    return {name: int(getattr(info, name)) for name, _ in _CInfo._fields_}


@dataclass
class DimerMatrix:
    """``dg_any`` and ``dg_end``: int32 (nx, ny), cal/mol, None for a plane that was not asked for; ``errX`` / ``errY`` per primer
    (1 empty, 2 longer than 64 bytes; ``errY`` is ``errX`` in pool mode)"""
    dg_any: np.ndarray | None
    dg_end: np.ndarray | None
    errX: np.ndarray
    errY: np.ndarray


@dataclass
class DimerScreen:
    """One entry per primer of X.  ``any_*``: the partner with the lowest energy over any run (``NONE``: none below 0), that
    energy, and where the run sits (``shift`` = s + len(y) - 1, ``pos`` = the run's first position on x, ``pairs``);
    ``end_*``: the same over the runs that hold x's 3' base; ``any_count`` / ``end_count``: the partners at or below the
    thresholds."""
    any_dg: np.ndarray
    any_partner: np.ndarray
    any_shift: np.ndarray
    any_pos: np.ndarray
    any_pairs: np.ndarray
    end_dg: np.ndarray
    end_partner: np.ndarray
    end_shift: np.ndarray
    end_pairs: np.ndarray
    any_count: np.ndarray
    end_count: np.ndarray
    errX: np.ndarray
    errY: np.ndarray


def _side(who, buf, offs):
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    if offs.ndim != 1 or len(offs) < 1:
        raise ValueError(f"{who}: offsets hold one entry more than there are primers")
    if len(offs) > 1 and int(offs.max()) > len(buf):
        raise ValueError(f"{who}: the offsets reach beyond the bytes")
    if len(buf) == 0:
        buf = np.zeros(1, np.uint8)                              # a pointer that is not NULL
    return buf, offs, len(offs) - 1


def _sides(who, buf, offs, other_buf, other_offs):
    X = _side(who, buf, offs)
    if (other_buf is None) != (other_offs is None):
        raise ValueError(f"{who}: other_buf and other_offs come together or not at all")
    Y = None if other_buf is None else _side(who, other_buf, other_offs)
    errX = np.zeros(X[2], np.uint32)
    errY = errX if Y is None else np.zeros(Y[2], np.uint32)
    yargs = (None, None, 0) if Y is None else (Y[0].ctypes.data, Y[1].ctypes.data, Y[2])
    return X, Y, errX, errY, (X[0].ctypes.data, X[1].ctypes.data, X[2]) + yargs


def _table(table, temp_c):
    return stack_dg(temp_c) if table is None else np.ascontiguousarray(table, dtype=np.int32).reshape(16)


def matrix_packed(buf, offs, other_buf=None, other_offs=None, table=None, temp_c: float = 37.0, want_any: bool = True,
                  want_end: bool = True) -> DimerMatrix:
    """polyhip_primer_dimer_matrix on packed primers (``buf`` / ``offs`` as the mappers take reads); without ``other_*`` the pool
    against itself.  ``table``: 16 int32 of one's own instead of ``stack_dg(temp_c)``."""
    X, Y, errX, errY, args = _sides("matrix_packed", buf, offs, other_buf, other_offs)
    tab = _table(table, temp_c)
    ny = X[2] if Y is None else Y[2]
    dg_any = np.zeros((X[2], ny), np.int32) if want_any else None
    dg_end = np.zeros((X[2], ny), np.int32) if want_end else None
    _lib.check(_lib.lib().polyhip_primer_dimer_matrix(tab.ctypes.data, *args, None if dg_any is None else dg_any.ctypes.data,
                                                      None if dg_end is None else dg_end.ctypes.data, errX.ctypes.data,
                                                      None if Y is None else errY.ctypes.data))
    return DimerMatrix(dg_any, dg_end, errX, errY)


def screen_packed(buf, offs, other_buf=None, other_offs=None, any_threshold: int = -6000, end_threshold: int = -4000, table=None,
                  temp_c: float = 37.0) -> DimerScreen:
    """polyhip_primer_dimer_screen on packed primers; the thresholds in cal/mol, at most 0"""
    X, Y, errX, errY, args = _sides("screen_packed", buf, offs, other_buf, other_offs)
    p = _CParams((C.c_int32 * 16)(*[int(v) for v in _table(table, temp_c)]), int(any_threshold), int(end_threshold))
    nx = X[2]
    any_dg, end_dg = np.zeros(nx, np.int32), np.zeros(nx, np.int32)
    any_partner, any_shift, any_pos, any_pairs, end_partner, end_shift, end_pairs, any_count, end_count = (np.zeros(nx, np.uint32)
                                                                                                           for _ in range(9))
    _lib.check(_lib.lib().polyhip_primer_dimer_screen(C.byref(p), *args, any_dg.ctypes.data, any_partner.ctypes.data, any_shift.ctypes.data,
                                                      any_pos.ctypes.data, any_pairs.ctypes.data, end_dg.ctypes.data, end_partner.ctypes.data,
                                                      end_shift.ctypes.data, end_pairs.ctypes.data, any_count.ctypes.data,
                                                      end_count.ctypes.data, errX.ctypes.data, None if Y is None else errY.ctypes.data))
    return DimerScreen(any_dg, any_partner, any_shift, any_pos, any_pairs, end_dg, end_partner, end_shift, end_pairs, any_count, end_count,
                       errX, errY)


def matrix(seqs, other=None, **kw) -> DimerMatrix:
    """``matrix_packed`` on lists of str / bytes: every primer of ``seqs`` against every one of ``other`` (default: of ``seqs``)"""
    return matrix_packed(*_pack(seqs), *(_pack(other) if other is not None else (None, None)), **kw)


def screen(seqs, other=None, any_threshold: int = -6000, end_threshold: int = -4000, **kw) -> DimerScreen:
    """``screen_packed`` on lists of str / bytes"""
    return screen_packed(*_pack(seqs), *(_pack(other) if other is not None else (None, None)), any_threshold=any_threshold,
                         end_threshold=end_threshold, **kw)


def _code(b: int) -> int:
    return {0x41: 0, 0x43: 1, 0x47: 2, 0x54: 3}.get(b & ~0x20, 4)                # either case of ACGT, 4 for every other byte


def render(x, y, shift: int) -> str:
    """The duplex at ``shift`` (as the screen reports it: s + len(y) - 1) as three lines of text: x 5'->3', a ``|`` under every
    paired position, y 3'->5'.  Host only, for the eye."""
    x = x.encode("latin-1") if isinstance(x, str) else bytes(x)
    y = y.encode("latin-1") if isinstance(y, str) else bytes(y)
    m, n = len(x), len(y)
    s = int(shift) - (n - 1)
    if not (1 <= m <= MAX_PRIMER and 1 <= n <= MAX_PRIMER and -(n - 1) <= s <= m - 1):
        raise ValueError("render: primers of 1..64 bytes and a shift of 0..len(x) + len(y) - 2")
    left = max(0, -s)                                            # columns in front of x[0]: y's 3' end hangs over
    yr = y[::-1]                                                 # y 3'->5'; yr[k] faces x[k + s]
    width = max(left + m, left + s + n)
    top = " " * left + x.decode("latin-1")
    bottom = " " * (left + s) + yr.decode("latin-1")
    bars = [" "] * width
    for i in range(m):
        k = i - s
        if 0 <= k < n and _code(x[i]) < 4 and _code(yr[k]) == 3 - _code(x[i]):
            bars[left + i] = "|"
    return "\n".join(line.rstrip() for line in (top, "".join(bars), bottom))
