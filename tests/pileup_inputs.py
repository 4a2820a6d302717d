"""Hand-built inputs of polyhip_pileup (tests/test_pileup_cpu.py and tests/test_pileup_gpu.py share them): entries given as
strings of column classes ('=' X I D, '?' for the invalid column) with a ref_start, on a reference text that the b columns
equal.  What they hold -- every column count, run placement, region, threshold, err value and batch size the kernels take
another path at -- is asserted in tests/test_pileup_cpu.py.  Callers leave what they get unchanged."""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass, replace

import numpy as np

from aln_records_inputs import BATCH_SIZES, COLUMN_COUNTS, LONGEST, random_classes, runs, strings

SEED = 505
MAPPED, REVERSE = 1, 2
GAP = 45


@dataclass(frozen=True)
class Entry:
    name: str
    classes: str        # one character per column
    A: bytes
    B: bytes
    ref_start: int
    ref_end: int
    flags: int = MAPPED
    mapq: int = 60


@dataclass(frozen=True)
class InputSet:
    name: str
    entries: tuple
    ref: bytes
    settings: tuple     # dicts of region / min_mapq / min_depth / min_alt_count / min_alt_permille: at least two


def text_columns(B: bytes) -> int:
    return sum(1 for b in B if b != GAP)


def on_text(name, classes, text: bytes, ref_start: int, rng, read=b"ACGT", **kw) -> Entry:
    """an entry whose b columns are the text from ref_start on ('A' beyond its end); '=' copies the text byte, X and I draw
    from ``read`` a byte of another class than the text's"""
    a, b, p = bytearray(), bytearray(), ref_start
    for c in classes:
        t = text[p] if p < len(text) else 65
        x = next(z for z in read[int(rng.integers(0, len(read))):] + read if z | 32 != t | 32)
        a.append(GAP if c in "D?" else t if c == "=" else x)
        b.append(GAP if c in "I?" else t)
        p += c in "=XD"
    return Entry(name, classes, bytes(a), bytes(b), ref_start, kw.pop("ref_end", p), **kw)


def random_text(rng, n: int) -> bytes:
    return bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, n))


DEFAULTS = dict(region=None, min_mapq=0, min_depth=0, min_alt_count=0, min_alt_permille=0)
STRICT = dict(region=None, min_mapq=20, min_depth=2, min_alt_count=2, min_alt_permille=300)


def _settings(*changes):
    return tuple(dict(DEFAULTS, **c) for c in changes)


# ---- 1. shapes: one entry after another on a text assembled from their b columns -------------------------------------------------
def shape_classes() -> dict:
    rng = np.random.default_rng(SEED)
    out = {f"cols{n}": random_classes(rng, n) for n in COLUMN_COUNTS + (LONGEST,)}
    for end in (63, 64, 65):
        for c in "ID":
            out[f"run_{c}_ends{end}"] = runs(("=", end - 5), (c, 5), ("=", 70 - end))
    for c in "ID":
        out[f"run_{c}_three_steps"] = runs(("=", 60), (c, 140), ("=", 10))
        out[f"run_{c}_starts_lane0"] = runs(("=", 64), (c, 3), ("=", 5))      # the anchor is the last column of the step before
    out["run_D_lane0_after_I"] = runs(("=", 60), ("I", 4), ("D", 3), ("=", 5))   # ... and that step ended in the other class
    out["run_I_lane0_after_D"] = runs(("=", 60), ("D", 4), ("I", 3), ("=", 5))
    out["run_I_lane0_of_third_step"] = runs(("=", 100), ("X", 28), ("I", 70), ("=", 3))
    out.update(d_i_d="===DID===", i_d_i="==IDI==", x_then_d="==XD==", i_last="====I", d_last="===DD", one_match="=", one_x="X")
    return out


@functools.lru_cache(maxsize=None)
def shapes() -> InputSet:
    rng = np.random.default_rng(SEED + 1)
    text, ents = bytearray(b"GA"), []
    for k, (name, cl) in enumerate(shape_classes().items()):
        A, B = strings(cl, rng)
        ents.append(Entry(name, cl, A, B, len(text), len(text) + text_columns(B), MAPPED | (REVERSE if k % 2 else 0), 10 + 7 * k % 50))
        text += bytes(b for b in B if b != GAP) + b"TC"[:k % 3]               # some entries touch, some stand apart
    return InputSet("shapes", tuple(ents), bytes(text), _settings({}, STRICT))


# ---- 2. events at the very start of the text ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edges() -> InputSet:
    rng = np.random.default_rng(SEED + 2)
    text = random_text(rng, 40)
    ents = (on_text("i_first_at_0", "II====", text, 0, rng), on_text("d_first_at_0", "D=====", text, 0, rng, flags=MAPPED | REVERSE),
            on_text("i_first_at_1", "II====", text, 1, rng), on_text("d_first_at_1", "DD====", text, 1, rng),
            on_text("i_only_at_0", "III", text, 0, rng), on_text("i_d_at_0", "ID==", text, 0, rng))
    return InputSet("edges", ents, text, _settings({}, dict(min_alt_count=2), dict(region=(0, 1)), dict(region=(1, 40))))


# ---- 3. regions ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def regions() -> InputSet:
    rng = np.random.default_rng(SEED + 3)
    text = random_text(rng, 120)
    ents = (on_text("del", "====DDD===", text, 10, rng),                                  # anchor 13, deleted 14..16
            on_text("ins", "====II====", text, 30, rng, flags=MAPPED | REVERSE),         # anchor 33
            on_text("long", random_classes(rng, 90), text, 20, rng),
            on_text("snv", "===X===", text, 100, rng))
    regs = [None, (13, 14), (14, 15), (10, 14), (14, 20), (33, 34), (34, 40), (25, 60), (0, 0), (57, 57), (120, 120), (12, 18), (28, 35), (103, 104)]
    return InputSet("regions", ents, text, _settings(*[dict(region=r) for r in regs]))


# ---- 4. many entries on the same cells ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contention() -> InputSet:
    rng = np.random.default_rng(SEED + 4)
    text = random_text(rng, 90)
    e = on_text("same", runs(("=", 30), ("X", 1), ("=", 9), ("D", 2), ("=", 10), ("I", 3), ("=", 18)), text, 10, rng)
    assert e.ref_end - e.ref_start == 70
    return InputSet("contention", (e,) * 257, text, _settings({}, dict(min_alt_permille=1000, min_depth=257), dict(min_depth=258)))


# ---- 5. random entries, both strands ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_set() -> InputSet:
    rng = np.random.default_rng(SEED + 5)
    text = random_text(rng, 300)
    ents = []
    for k in range(5000):
        cl = random_classes(rng, int(rng.integers(1, 131)))
        used = sum(c != "I" for c in cl)
        ents.append(on_text(f"r{k}", cl, text, int(rng.integers(0, 300 - used + 1)), rng, flags=MAPPED | (REVERSE if rng.integers(0, 2) else 0),
                            mapq=int(rng.integers(0, 61))))
    return InputSet("random", tuple(ents), text, _settings({}, STRICT, dict(region=(37, 263), min_alt_permille=100, min_depth=900)))


# ---- 6. bytes: lower case, IUPAC, a lower-case text -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def byte_set() -> InputSet:
    rng = np.random.default_rng(SEED + 6)
    text = random_text(rng, 30) + random_text(rng, 30).lower() + b"NNRY" + random_text(rng, 26)
    ents = [on_text("upper_on_lower", "=" * 20 + "X" + "=" * 9, text, 30, rng),
            on_text("lower_read", "==X==I==X==", text, 2, rng, read=b"acgt"),
            on_text("iupac_read", "=XXXX=IIXD=", text, 5, rng, read=b"RYKMSWBDHVNn", flags=MAPPED | REVERSE),
            on_text("on_n", "=" * 12, text, 56, rng), on_text("x_on_n", "==XXXXX==", text, 58, rng)]
    e = on_text("e", "=" * 10, text, 30, rng)
    ents.append(replace(e, name="same_class_other_case", A=e.A.upper()))      # a is 'A' where the text says 'a': class A, no SNV
    return InputSet("bytes", tuple(ents), text, _settings({}, dict(min_alt_permille=500), dict(min_depth=2)))


# ---- 7. err values ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def errs() -> InputSet:
    rng = np.random.default_rng(SEED + 7)
    text = random_text(rng, 150)
    good = on_text("good", "=" * 12, text, 4, rng)
    differs = bytes([good.B[0]]) + bytes(b"CGTA"[b"ACGT".index(good.B[1])] for _ in (0,)) + good.B[2:]
    ents = [good,
            on_text("err1", "====?===", text, 20, rng), on_text("err1_second_step", "=" * 100 + "?" + "=" * 5, text, 3, rng),
            replace(good, name="err2_end_short", ref_end=good.ref_end - 1), replace(good, name="err2_end_long", ref_end=good.ref_end + 1),
            on_text("err2_beyond_text", "=" * 12, text, 145, rng),                          # the symbols agree, ref_end = 157 > 150
            on_text("ends_at_text_end", "=" * 12, text, 138, rng),
            Entry("err3", "", b"", b"", 9, 9), Entry("err2_before_err3", "", b"", b"", 9, 10),
            replace(good, name="err5", B=differs), replace(good, name="err5_read_agrees", A=differs, B=differs),
            replace(on_text("e", "==?==", text, 40, rng), name="err1_before_err2", ref_end=99),
            replace(good, name="err2_before_err5", B=differs, ref_end=good.ref_end + 3),
            on_text("err5_second_step", "=" * 80, text[:70] + bytes([text[70] ^ 6]) + text[71:], 0, rng),
            Entry("unmapped_invalid", "?????", b"-----", b"-----", 0, 0, flags=0), Entry("unmapped_reverse", "", b"", b"", 0, 0, flags=REVERSE),
            replace(on_text("e", "==?==", text, 60, rng), name="low_mapq_invalid", mapq=19),
            replace(good, name="low_mapq_err5", B=differs, mapq=0), replace(good, name="mapq_at_threshold", mapq=20)]
    return InputSet("errs", tuple(ents), text, _settings({}, STRICT, dict(min_mapq=20)))


# ---- 8. thresholds and consensus ties ------------------------------------------------------------------------------------------------
THRESHOLD_DEPTH = 8


@functools.lru_cache(maxsize=None)
def thresholds() -> InputSet:
    """8 reads on positions 10..39 of a text of A's: position 15 has 2 reads saying C (250 permille exactly), position 20 has 1
    (125), position 25 has 4 saying C (a tie between two bases), position 30 is deleted in 4 (a tie between a base and '*')"""
    text = b"A" * 50
    ents = []
    for k in range(THRESHOLD_DEPTH):
        a = bytearray(text[10:40])
        if k < 2:
            a[5] = 67
        if k == 0:
            a[10] = 67
        if k % 2:
            a[15] = 67
        else:
            a[20] = GAP
        ents.append(Entry(f"t{k}", "", bytes(a), text[10:40], 10, 40, MAPPED | (REVERSE if k in (1, 2) else 0)))
    d = THRESHOLD_DEPTH
    sets = [dict(min_alt_permille=250), dict(min_alt_permille=251), dict(min_alt_permille=125), dict(min_alt_count=2), dict(min_alt_count=3),
            dict(min_depth=d - 1), dict(min_depth=d), dict(min_depth=d + 1), dict(min_alt_permille=500, min_alt_count=4)]
    return InputSet("thresholds", tuple(ents), text, _settings(*sets))


# ---- 9. batch sizes --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch(n: int) -> InputSet:
    """n entries: the shapes in turn (the longest one only once), every third entry unmapped"""
    s = shapes()
    pool = [e for e in s.entries if len(e.A) <= 300]
    out = [e for e in s.entries if len(e.A) == LONGEST] if n > 200 else []
    it = itertools.cycle(pool)
    while len(out) < n:
        out.append(Entry(f"unmapped{len(out)}", "", b"--" * (len(out) % 2), b"--" * (len(out) % 2), 0, 0, flags=0) if len(out) % 3 == 1
                   else next(it))
    return InputSet(f"batch{n}", tuple(out), s.ref, _settings({}, STRICT))


def all_sets() -> tuple:
    return (shapes(), edges(), regions(), contention(), random_set(), byte_set(), errs(), thresholds()) + tuple(batch(n) for n in BATCH_SIZES)


def pack(entries) -> dict:
    """the arrays polyhip_pileup takes"""
    off = np.zeros(len(entries) + 1, np.uint64)
    off[1:] = np.cumsum([len(e.A) for e in entries], dtype=np.uint64)
    u32 = lambda f: np.array([getattr(e, f) for e in entries], np.uint32)    # noqa: E731
    return dict(flags=u32("flags"), mapq=np.array([e.mapq for e in entries], np.uint8), ref_start=u32("ref_start"), ref_end=u32("ref_end"),
                alnA=np.frombuffer(b"".join(e.A for e in entries), np.uint8), alnB=np.frombuffer(b"".join(e.B for e in entries), np.uint8),
                aln_off=off)


# ---- planted variants: what a user checks a construct for ---------------------------------------------------------------------------
PLANTED_SNV, PLANTED_DEL, PLANTED_INS = 500, 999, 1500       # the SNV's position; the anchors of the deletion and the insertion
PLANTED_SITES = ((PLANTED_SNV, 1), (PLANTED_DEL, 3), (PLANTED_INS, 2))


@functools.lru_cache(maxsize=None)
def planted() -> dict:
    """-> T: a 2 kb text; sample: T with one SNV, 3 bases deleted and 2 inserted; reads: 200 reads of 100 bases drawn evenly
    from the sample, every second one reverse-complemented.  The bytes around the two indels are fixed so that neither can
    be shifted to a neighbouring position without a mismatch."""
    rng = np.random.default_rng(SEED + 9)
    T = bytearray(random_text(rng, 2000))
    T[998:1005] = b"GACGTAC"            # deleted: CGT at 1000..1002, anchored at 999
    T[1499:1503] = b"TACT"              # inserted: GG between 1500 and 1501
    T = bytes(T)
    snv = b"CGTA"[b"ACGT".index(T[PLANTED_SNV])]
    sample = T[:PLANTED_SNV] + bytes([snv]) + T[PLANTED_SNV + 1:1000] + T[1003:1501] + b"GG" + T[1501:]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    reads = []
    for k in range(200):
        at = k * (len(sample) - 100) // 199
        r = sample[at:at + 100]
        reads.append(r.translate(comp)[::-1] if k % 2 else r)
    return dict(T=T, sample=sample, reads=reads, snv=snv)
