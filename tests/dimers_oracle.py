"""The primer-dimer screen on the CPU: the definition above polyhip_primer_stack_dg in include/polyhip.h restated in plain Python
-- loops over the shifts and the positions, no bit masks, the table by the integer formula.  What the tests hold
polyhip_primer_dimer_matrix and polyhip_primer_dimer_screen to."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

NONE = 0xFFFFFFFF
MAX_PRIMER = 64
PAIRS16 = ("AA", "AC", "AG", "AT", "CA", "CC", "CG", "CT", "GA", "GC", "GG", "GT", "TA", "TC", "TG", "TT")
# SantaLucia 1998, unified nearest-neighbour parameters: dH in kcal/mol and dS in cal/(mol K), times ten, in the order of PAIRS16
H10 = (-76, -84, -78, -72, -85, -80, -106, -78, -82, -98, -80, -84, -72, -82, -85, -76)
S10 = (-213, -224, -210, -204, -227, -199, -272, -210, -222, -244, -199, -224, -213, -222, -227, -213)
MIN_TEMP_MK, MAX_TEMP_MK = 273150, 338000
INFO_FIELDS = ("primers", "bad", "pairs", "shifts", "launches")


def stack_table(temp_mk: int = 310150) -> list:
    """the 16 entries in cal/mol: (10 dH * 1e6 - temp_mK * 10 dS) / 1e4, rounded half away from zero, in integers"""
    assert MIN_TEMP_MK <= temp_mk <= MAX_TEMP_MK
    out = []
    for h, s in zip(H10, S10):
        num = h * 1_000_000 - temp_mk * s
        mag = (abs(num) + 5000) // 10000
        out.append(-mag if num < 0 else mag)
    return out


def code(b: int) -> int:
    if 0x61 <= b <= 0x7A:
        b -= 0x20
    return {0x41: 0, 0x43: 1, 0x47: 2, 0x54: 3}.get(b, 4)


def err_of(p: bytes) -> int:
    return 1 if len(p) == 0 else 2 if len(p) > MAX_PRIMER else 0


def runs(x: bytes, y: bytes, table):
    """every run of two or more pairs of the ordered pair (x, y): (dg, s, i0, i1), shifts ascending, then positions ascending"""
    m, n = len(x), len(y)
    cx, cy = [code(b) for b in x], [code(b) for b in y]
    for s in range(-(n - 1), m):
        lo, hi = max(0, s), min(m - 1, s + n - 1)                 # the positions i of x with 0 <= i - s <= n - 1
        paired = {i: cx[i] < 4 and cy[n - 1 - (i - s)] == 3 - cx[i] for i in range(lo, hi + 1)}
        i = lo
        while i <= hi:
            if not paired[i]:
                i += 1
                continue
            i0 = i
            while i + 1 <= hi and paired[i + 1]:
                i += 1
            if i > i0:
                yield sum(table[4 * cx[t] + cx[t + 1]] for t in range(i0, i)), s, i0, i
            i += 1


@dataclass
class Pair:
    dg_any: int = 0
    any_shift: int = 0
    any_pos: int = 0
    any_pairs: int = 0
    dg_end: int = 0
    end_shift: int = 0
    end_pairs: int = 0


def pair(x: bytes, y: bytes, table=None) -> Pair:
    """the per-pair results of two valid primers; among equal dg the smallest s, then the smallest i0"""
    table = stack_table() if table is None else table
    m, n = len(x), len(y)
    assert 1 <= m <= MAX_PRIMER and 1 <= n <= MAX_PRIMER
    best, best_end = None, None
    for dg, s, i0, i1 in runs(x, y, table):
        if best is None or dg < best[0]:
            best = (dg, s, i0, i1)
        if i1 == m - 1 and (best_end is None or dg < best_end[0]):
            best_end = (dg, s, i0, i1)
    r = Pair()
    if best is not None:
        r.dg_any, r.any_shift, r.any_pos, r.any_pairs = best[0], best[1] + n - 1, best[2], best[3] - best[2] + 1
    if best_end is not None:
        r.dg_end, r.end_shift, r.end_pairs = best_end[0], best_end[1] + n - 1, best_end[3] - best_end[2] + 1
    return r


def matrix(X, Y=None, table=None):
    """(dg_any, dg_end, errX, errY): int32 planes of len(X) x len(Y); a pair with a bad primer is 0 in both"""
    table = stack_table() if table is None else table
    Y = X if Y is None else Y
    any_ = np.zeros((len(X), len(Y)), np.int32)
    end = np.zeros((len(X), len(Y)), np.int32)
    seen = {}                                                    # a pair that occurs more than once is worked out once
    for i, x in enumerate(X):
        for j, y in enumerate(Y):
            if err_of(x) == 0 and err_of(y) == 0:
                p = seen.get((x, y))
                if p is None:
                    p = seen[(x, y)] = pair(x, y, table)
                any_[i, j], end[i, j] = p.dg_any, p.dg_end
    return any_, end, np.array([err_of(x) for x in X], np.uint32), np.array([err_of(y) for y in Y], np.uint32)


SCREEN_FIELDS = ("any_dg", "any_partner", "any_shift", "any_pos", "any_pairs", "end_dg", "end_partner", "end_shift", "end_pairs",
                 "any_count", "end_count")


def screen_row(x: bytes, Y, any_threshold: int, end_threshold: int, table=None) -> dict:
    """one row of the screen: the smallest dg over the valid y, ties to the smallest j; no partner when that dg is 0"""
    table = stack_table() if table is None else table
    r = dict.fromkeys(SCREEN_FIELDS, 0)
    r["any_partner"] = r["end_partner"] = NONE
    if err_of(x):
        return r
    seen = {}                                                    # a y that stands in Y more than once is worked out once
    for j, y in enumerate(Y):
        if err_of(y):
            continue
        p = seen.get(y)
        if p is None:
            p = seen[y] = pair(x, y, table)
        r["any_count"] += p.dg_any <= any_threshold
        r["end_count"] += p.dg_end <= end_threshold
        if p.dg_any < r["any_dg"]:
            r.update(any_dg=p.dg_any, any_partner=j, any_shift=p.any_shift, any_pos=p.any_pos, any_pairs=p.any_pairs)
        if p.dg_end < r["end_dg"]:
            r.update(end_dg=p.dg_end, end_partner=j, end_shift=p.end_shift, end_pairs=p.end_pairs)
    return r


def screen(X, Y=None, any_threshold: int = -6000, end_threshold: int = -4000, table=None) -> dict:
    """the screen's outputs as arrays, with errX and errY"""
    Y = X if Y is None else Y
    got = [screen_row(x, Y, any_threshold, end_threshold, table) for x in X]
    out = {f: np.array([g[f] for g in got], np.int32 if f.endswith("_dg") else np.uint32) for f in SCREEN_FIELDS}
    out["errX"] = np.array([err_of(x) for x in X], np.uint32)
    out["errY"] = np.array([err_of(y) for y in Y], np.uint32)
    return out


def screen_from_matrix(dg_any, dg_end, errX, errY, any_threshold: int, end_threshold: int) -> dict:
    """dg, partner and count of the screen as a numpy reduction of the matrix call's planes"""
    okx, oky = np.asarray(errX) == 0, np.asarray(errY) == 0
    out = {}
    for name, plane, thr in (("any", dg_any, any_threshold), ("end", dg_end, end_threshold)):
        p = np.where(oky[None, :] & okx[:, None], plane.astype(np.int64), 1)       # 1: not a candidate
        if p.shape[1] == 0:
            p = np.ones((p.shape[0], 1), np.int64)
        best = p.min(axis=1)
        arg = p.argmin(axis=1)                                                       # the first of equals
        hit = best < 0
        out[name + "_dg"] = np.where(hit, best, 0).astype(np.int32)
        out[name + "_partner"] = np.where(hit, arg, NONE).astype(np.uint32)
        out[name + "_count"] = ((p <= thr) & (p < 1)).sum(axis=1).astype(np.uint32)
    return out


def info(X, Y=None, launches=None) -> dict:
    """polyhip_primer_dimer_last_info for a call on (X, Y); launches is the call's own business"""
    pool = Y is None
    Y = X if pool else Y
    gx, gy = [len(x) for x in X if err_of(x) == 0], [len(y) for y in Y if err_of(y) == 0]
    primers = len(X) + (0 if pool else len(Y))
    bad = len(X) - len(gx) + (0 if pool else len(Y) - len(gy))
    d = dict(primers=primers, bad=bad, pairs=len(gx) * len(gy), shifts=sum(m + n - 1 for m in gx for n in gy))
    if launches is not None:
        d["launches"] = launches
    return d


def revcomp(x: bytes) -> bytes:
    return bytes(b"ACGT"[3 - code(b)] if code(b) < 4 else ord("N") for b in reversed(x))
