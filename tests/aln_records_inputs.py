"""Hand-built inputs of polyhip_aln_records (tests/test_aln_records_cpu.py and tests/test_aln_records_gpu.py share them): entries
given as strings of column classes ('=' X I D, '?' for the invalid column), turned into the two gapped strings with a fixed
seed.  What they hold -- every column count, run placement, column mix, clip, score setting, err value and batch size the
kernel takes another path at -- is asserted in tests/test_aln_records_cpu.py.  Callers leave what they get unchanged."""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass

import numpy as np

SEED = 404
COLUMN_COUNTS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
LONGEST = 4096 + 7168                    # what a mapper call can emit at most: max_len rows and the widest window
MATCH_RUNS = (9, 10, 99, 100, 999, 1000)
BATCH_SIZES = (1, 255, 256, 257)
MAPPED, REVERSE, PROPER = 1, 2, 4


@dataclass(frozen=True)
class Case:
    name: str
    classes: str        # one character per column
    A: bytes
    B: bytes
    read_start: int
    read_end: int
    read_len: int
    flags: int = MAPPED
    score: int = 100
    second: int = 40


def strings(classes: str, rng) -> tuple:
    """the two gapped strings of a class string: random bases, X columns get two different ones"""
    a, b = bytearray(), bytearray()
    for c in classes:
        x = b"ACGT"[int(rng.integers(0, 4))]
        y = next(z for z in b"CGTA"[int(rng.integers(0, 4)):] + b"CGTA" if z != x)
        a.append(45 if c in "D?" else x)
        b.append(45 if c in "I?" else x if c == "=" else y)
    return bytes(a), bytes(b)


def runs(*parts) -> str:
    """runs(('=', 3), ('X', 1)) -> '===X'"""
    return "".join(c * k for c, k in parts)


def random_classes(rng, ncol: int) -> str:
    """runs of random class and length 1..40 (matches three times as likely), cut to ncol columns"""
    out = ""
    while len(out) < ncol:
        out += "===XID"[int(rng.integers(0, 6))] * int(rng.integers(1, 41))
    return out[:ncol]


def case(name, classes, rng, left=0, right=0, **kw) -> Case:
    A, B = strings(classes, rng)
    used = sum(1 for x in A if x != 45)
    return Case(name, classes, A, B, left, left + used, left + used + right, **kw)


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    rng = np.random.default_rng(SEED)
    out = []
    # column counts: a step is 64 columns
    for n in COLUMN_COUNTS + (LONGEST,):
        out.append(case(f"cols{n}", random_classes(rng, n), rng, left=n % 3, right=n % 2))
    # runs against the 64-column boundary: ending one before it, at it, one after it; and over three steps
    for end in (63, 64, 65):
        for c in "XID=":
            other = "X" if c == "=" else "="
            out.append(case(f"run_{c}_ends{end}", runs((other, end - 5), (c, 5), (other, 70 - end)), rng))
    for c in "XID=":
        other = "X" if c == "=" else "="
        out.append(case(f"run_{c}_three_steps", runs((other, 60), (c, 140), (other, 10)), rng))
    # MD digit counts
    for k in MATCH_RUNS:
        out.append(case(f"match{k}", runs(("=", k), ("X", 1), ("=", k), ("D", 2), ("=", k)), rng))
    # column mixes
    for name, cl in (("adjacent_mismatches", "===XX==="), ("d_then_x", "===DDX==="), ("d_i_d", "===DID==="), ("i_first", "II===="),
                     ("d_first", "D====="), ("i_last", "====I"), ("d_last", "===DD"), ("all_x", "X" * 70), ("x_then_d", "==XD=="),
                     ("i_d_i", "==IDI=="), ("one_match", "="), ("one_x", "X")):
        out.append(case(name, cl, rng))
    # soft clips
    for name, left, right in (("clip_none", 0, 0), ("clip_left", 7, 0), ("clip_right", 0, 9), ("clip_both", 30, 12)):
        out.append(case(name, runs(("=", 20), ("X", 1), ("=", 30)), rng, left=left, right=right))
    # score and second
    for name, s, t in (("second_zero", 90, 0), ("second_negative", 90, -5), ("second_equal", 90, 90), ("second_above", 90, 120),
                       ("score_one", 1, 0), ("second_close", 120, 119), ("second_half", 120, 60)):
        out.append(case(name, "=" * 30, rng, score=s, second=t))
    out.append(case("reverse", runs(("=", 10), ("I", 2), ("=", 10)), rng, left=3, flags=MAPPED | REVERSE))
    # err 1-3 (4 needs 2^28 columns: tests/test_aln_records_cpu.py fakes the offsets on the oracle's side)
    out.append(case("err1", "====?===", rng))
    out.append(case("err1_second_step", "=" * 100 + "?" + "=" * 5, rng))
    e = case("e", "=" * 12, rng, left=4)
    out.append(Case("err2_start_above_end", e.classes, e.A, e.B, 17, 16, 16))
    out.append(Case("err2_end_above_len", e.classes, e.A, e.B, 4, 16, 15))
    out.append(Case("err2_symbols", e.classes, e.A, e.B, 4, 15, 16))
    out.append(Case("err3", "", b"", b"", 5, 5, 20))
    out.append(Case("err2_before_err3", "", b"", b"", 5, 6, 20))
    e = case("e", "==?==", rng)
    out.append(Case("err1_before_err2", e.classes, e.A, e.B, 0, e.read_end + 1, e.read_len + 1))   # its symbols differ as well
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def unmapped(k: int) -> Case:
    """an entry that is not mapped; every second one has columns all the same, invalid ones, which are never read"""
    s = b"-" * (5 if k % 2 else 0)
    return Case(f"unmapped{k}", "?" * len(s), s, s, 0, 0, 30, flags=0, score=0, second=0)


def pack(cs) -> dict:
    """the arrays polyhip_aln_records takes"""
    off = np.zeros(len(cs) + 1, np.uint64)
    off[1:] = np.cumsum([len(c.A) for c in cs], dtype=np.uint64)
    u32 = lambda f: np.array([getattr(c, f) for c in cs], np.uint32)    # noqa: E731
    i64 = lambda f: np.array([getattr(c, f) for c in cs], np.int64)     # noqa: E731
    return dict(flags=u32("flags"), score=i64("score"), second=i64("second"), read_start=u32("read_start"), read_end=u32("read_end"),
                read_len=u32("read_len"), alnA=np.frombuffer(b"".join(c.A for c in cs), np.uint8),
                alnB=np.frombuffer(b"".join(c.B for c in cs), np.uint8), aln_off=off)


@functools.lru_cache(maxsize=None)
def batch(n: int) -> tuple:
    """n entries: the cases in turn (the longest one only once), every third entry unmapped"""
    pool = [c for c in cases() if len(c.A) <= 1100]
    out = [c for c in cases() if len(c.A) == LONGEST] if n > 200 else []
    it = itertools.cycle(pool)
    while len(out) < n:
        out.append(unmapped(len(out)) if len(out) % 3 == 1 else next(it))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def paired_batch() -> tuple:
    """every combination, per mate, of live / unmapped / err, forward / reverse, proper bit set or not: 144 pairs"""
    rng = np.random.default_rng(SEED + 1)
    kinds = list(itertools.product(("live", "unmapped", "err"), (0, REVERSE), (0, PROPER)))
    out = []
    for k1, k2 in itertools.product(kinds, kinds):
        for state, rev, proper in (k1, k2):
            cl = {"live": "====X==I==", "unmapped": "", "err": "==?=="}[state]
            out.append(case(f"{state}_{rev}_{proper}", cl, rng, left=len(out) % 2, flags=(0 if state == "unmapped" else MAPPED) | rev | proper))
    return tuple(out)
