"""Inputs of polyhip_pileup_qual (tests/test_pileup_qual_cpu.py and tests/test_pileup_qual_gpu.py share them): every InputSet of
tests/pileup_inputs.py with a read_start, a trailing clip and a seeded quality string over '!'..'J' attached to each entry, and
sets of their own for err 6, err 7 and the runs that cross a 64-column step.  What they hold is asserted in
tests/test_pileup_qual_cpu.py.  Callers leave what they get unchanged."""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace

import numpy as np

import pileup_inputs as pi
from aln_records_inputs import runs

SEED = 707
Q_LO, Q_HI = ord("!"), ord("J")          # Phred 0..41 at offset 33
MIN_BASE_QUALS = (0, 20, 42)             # nothing filtered; some; every base


@dataclass(frozen=True)
class QualSet:
    name: str
    entries: tuple          # pileup_inputs.Entry
    read_start: tuple       # per entry: bases of the oriented read in front of the first column (a leading clip)
    quals: tuple            # per entry: bytes, the quality string of the read as sequenced
    ref: bytes
    settings: tuple


def read_columns(A: bytes) -> int:
    return sum(1 for a in A if a != pi.GAP)


def clips(k: int) -> tuple:
    """(leading, trailing) clip of the k-th entry of a set: every combination of zero and non-zero comes up"""
    return (0 if k % 3 == 0 else 1 + k % 5), (0 if k % 2 == 0 else 1 + k % 4)


def attach(s: pi.InputSet, seed: int) -> QualSet:
    rng = np.random.default_rng(SEED + seed)
    starts, quals = [], []
    for k, e in enumerate(s.entries):
        lead, trail = clips(k)
        starts.append(lead)
        quals.append(bytes(rng.integers(Q_LO, Q_HI + 1, lead + read_columns(e.A) + trail, dtype=np.uint8)))
    return QualSet(s.name, s.entries, tuple(starts), tuple(quals), s.ref, s.settings)


# ---- err 6 and err 7 ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def quality_errs() -> QualSet:
    rng = np.random.default_rng(SEED + 100)
    text = pi.random_text(rng, 400)
    qs = lambda n: bytearray(rng.integers(Q_LO, Q_HI + 1, n, dtype=np.uint8))    # noqa: E731
    ents, starts, quals = [], [], []

    def add(e, lead, q):
        ents.append(e)
        starts.append(lead)
        quals.append(bytes(q))

    good = pi.on_text("good", "===X==II==DD==", text, 10, rng)               # 12 read columns
    rev = replace(good, name="good_reverse", flags=pi.MAPPED | pi.REVERSE)
    nA = read_columns(good.A)
    add(good, 2, qs(2 + nA + 3))
    add(rev, 2, qs(2 + nA + 3))
    add(replace(good, name="exact_length"), 0, qs(nA))                       # m_i equals the aligned length
    add(replace(good, name="err6_one_short"), 2, qs(2 + nA - 1))
    add(replace(rev, name="err6_one_short_reverse"), 2, qs(2 + nA - 1))
    add(replace(good, name="err6_no_quality"), 0, b"")                       # m_i = 0
    add(replace(good, name="err6_read_start_beyond"), 40, qs(2 + nA + 3))
    differs = bytes([good.B[0]]) + bytes([b"CGTA"[b"ACGT".index(good.B[1])]]) + good.B[2:]
    add(replace(good, name="err5_before_err6", B=differs), 2, qs(3))
    add(replace(good, name="err2_before_err6", ref_end=good.ref_end + 1), 2, qs(3))
    low, high = Q_LO - 1, Q_LO + 93 + 1                                      # 32 and 127
    q = qs(2 + nA + 3); q[5] = low                                           # noqa: E702
    add(replace(good, name="err7_aligned_low"), 2, q)
    q = qs(2 + nA + 3); q[0] = high                                          # noqa: E702
    add(replace(good, name="err7_leading_clip_only"), 2, q)
    q = qs(2 + nA + 3); q[-1] = low                                          # noqa: E702
    add(replace(good, name="err7_trailing_clip_only"), 2, q)
    q = qs(2 + nA + 3); q[0] = low                                           # noqa: E702  (the sequenced read's first byte is q's last)
    add(replace(rev, name="err7_reverse_clip_only"), 2, q)
    q = qs(2 + nA - 1); q[0] = low                                           # noqa: E702
    add(replace(good, name="err6_before_err7"), 2, q)
    q = qs(2 + nA + 3); q[3], q[4] = Q_LO, Q_LO + 93                        # noqa: E702  the two ends of the range are fine: Q = 0 and 93
    add(replace(good, name="range_ends_ok"), 2, q)
    longe = pi.on_text("long", runs(("=", 150)), text, 100, rng)
    q = qs(150 + 21); q[150 + 20] = high                                     # noqa: E702  the third 64-byte step of the sweep, its last byte
    add(replace(longe, name="err7_third_step_of_clip"), 0, q)
    add(replace(longe, name="long_ok", flags=pi.MAPPED | pi.REVERSE), 21, qs(150 + 21))
    q = qs(8); q[2] = low                                                    # noqa: E702
    add(pi.Entry("unmapped_bad_quality", "", b"", b"", 0, 0, flags=0), 0, q)
    q = qs(2 + nA + 3); q[1] = high                                          # noqa: E702
    add(replace(good, name="low_mapq_bad_quality", mapq=19), 2, q)
    add(pi.Entry("err3_before_err6", "", b"", b"", 9, 9), 5, b"")
    return QualSet("quality_errs", tuple(ents), tuple(starts), tuple(quals), text, pi._settings({}, dict(min_mapq=20)))


# ---- the read index crossing a 64-column step inside a run, both strands ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crossing() -> QualSet:
    rng = np.random.default_rng(SEED + 101)
    text = pi.random_text(rng, 700)
    ents, starts, quals = [], [], []
    for k, (c, strand) in enumerate((c, s) for c in "ID" for s in (0, pi.REVERSE)):
        cl = runs(("=", 50), ("D" if c == "I" else "I", 7), ("=", 3), (c, 20), ("=", 60), ("X", 1), ("=", 40))   # the run holds columns 60..79
        e = pi.on_text(f"run_{c}_crosses_{'reverse' if strand else 'forward'}", cl, text, 5 + 160 * k, rng, flags=pi.MAPPED | strand)
        lead = 3 + k
        ents.append(e)
        starts.append(lead)
        quals.append(bytes(rng.integers(Q_LO, Q_HI + 1, lead + read_columns(e.A) + 2 * k, dtype=np.uint8)))
    return QualSet("crossing", tuple(ents), tuple(starts), tuple(quals), text, pi._settings({}, dict(region=(60, 400))))


@functools.lru_cache(maxsize=None)
def all_sets() -> tuple:
    return tuple(attach(s, k) for k, s in enumerate(pi.all_sets())) + (quality_errs(), crossing())


def pack(s: QualSet, rebase: int = 0) -> dict:
    """the arrays polyhip_pileup_qual takes; rebase: added to every quality byte (another Phred offset)"""
    p = pi.pack(s.entries)
    off = np.zeros(len(s.entries) + 1, np.uint64)
    off[1:] = np.cumsum([len(q) for q in s.quals], dtype=np.uint64)
    qual = np.frombuffer(b"".join(s.quals), np.uint8)
    p.update(read_start=np.array(s.read_start, np.uint32), qual=(qual + np.uint8(rebase)) if rebase else qual, qual_off=off)
    return p
