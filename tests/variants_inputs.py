"""Inputs of polyhip_call_variants (tests/test_variants_cpu.py and tests/test_variants_gpu.py share them): entries spelled as
operations on a text -- ('=', n) copies n text bytes, ('X', bytes) base columns with those read bytes, ('I', bytes) an insertion of
those bytes, ('D', n) a deletion of n text bytes -- so that every inserted byte and every repeat is chosen, not drawn.  Each
entry has a leading clip, a trailing clip and a quality string as tests/pileup_qual_inputs.py attaches them.  What the sets
hold is asserted in tests/test_variants_cpu.py.  Callers leave what they get unchanged."""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace

import numpy as np

import pileup_inputs as pi
import pileup_qual_inputs as qi

SEED = 1111
MAPPED, REVERSE = pi.MAPPED, pi.REVERSE
DEFAULTS = dict(pi.DEFAULTS, min_base_qual=0, left_align=1, hom_permille=800, max_indel=0)


@dataclass(frozen=True)
class VarSet:
    name: str
    entries: tuple          # pileup_inputs.Entry
    read_start: tuple
    quals: tuple
    ref: bytes
    settings: tuple         # dicts of DEFAULTS' keys


def settings(*changes) -> tuple:
    return tuple(dict(DEFAULTS, **c) for c in changes)


BOTH = ({}, dict(left_align=0))


def make(name: str, text: bytes, rs: int, ops, flags: int = MAPPED, mapq: int = 60) -> pi.Entry:
    a, b, p = bytearray(), bytearray(), rs
    for op, arg in ops:
        if op == "=":
            assert p + arg <= len(text), name
            a += text[p:p + arg]
            b += text[p:p + arg]
            p += arg
        elif op == "X":
            a += arg
            b += text[p:p + len(arg)]
            p += len(arg)
        elif op == "I":
            a += arg
            b += b"-" * len(arg)
        elif op == "D":
            a += b"-" * arg
            b += text[p:p + arg]
            p += arg
        else:
            raise ValueError(op)
    cls = "".join("D" if x == pi.GAP else "I" if y == pi.GAP else "=" if x == y else "X" for x, y in zip(a, b))
    return pi.Entry(name, cls, bytes(a), bytes(b), rs, p, flags, mapq)


def attach(name: str, entries, ref: bytes, sets: tuple, seed: int, quals=None) -> VarSet:
    """quality strings over '!'..'J' with the clips of pileup_qual_inputs.clips; quals: {entry index: bytes} fixes some"""
    rng = np.random.default_rng(SEED + seed)
    starts, qs = [], []
    for k, e in enumerate(entries):
        lead, trail = qi.clips(k)
        q = bytes(rng.integers(qi.Q_LO, qi.Q_HI + 1, lead + qi.read_columns(e.A) + trail, dtype=np.uint8))
        if quals and k in quals:
            lead, q = 0, quals[k]
        starts.append(lead)
        qs.append(q)
    return VarSet(name, tuple(entries), tuple(starts), tuple(qs), ref, sets)


def other(byte: int) -> int:
    """a base of another class"""
    return b"CGTA"[b"ACGT".index(byte & ~32)]


def not_these(*bytes_) -> int:
    return next(x for x in b"ACGT" if x not in [y & ~32 for y in bytes_])


# ---- 1. step edges: where a run starts in its entry --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def steps() -> VarSet:
    rng = np.random.default_rng(SEED + 1)
    text = pi.random_text(rng, 2400)
    ents, at = [], 5
    ins = lambda p, n: bytes(not_these(text[p - 1], text[p]) for _ in range(n))     # noqa: E731  an insertion in front of p that cannot move
    for start in (63, 64, 65):
        ents.append(make(f"i_starts{start}", text, at, (("=", start), ("I", ins(at + start, 3)), ("=", 20)), MAPPED | (REVERSE if start & 1 else 0)))
        ents.append(make(f"d_starts{start}", text, at + 7, (("=", start), ("D", 3), ("=", 20))))
        at += 110
    ents.append(make("i_three_steps", text, at, (("=", 60), ("I", ins(at + 60, 140)), ("=", 10))))
    ents.append(make("d_three_steps", text, at + 100, (("=", 60), ("D", 140), ("=", 10)), MAPPED | REVERSE))
    at += 420
    ents.append(make("i_first", text, at, (("I", ins(at, 2)), ("=", 30))))
    ents.append(make("d_first", text, at + 40, (("D", 2), ("=", 30))))
    ents.append(make("i_last", text, at + 80, (("=", 30), ("I", ins(at + 110, 2)))))
    ents.append(make("d_last", text, at + 120, (("=", 30), ("D", 2))))
    ents.append(make("i_then_d_first", text, at + 160, (("I", b"GG"), ("D", 2), ("=", 30))))
    ents.append(make("x_before_i_at64", text, at + 200, (("=", 63), ("X", bytes([other(text[at + 263])])), ("I", ins(at + 264, 5)), ("=", 9))))
    return attach("steps", ents, text, settings(*BOTH, dict(region=(300, 900)), dict(region=(300, 900), left_align=0)), 1)


# ---- 2. lengths: the sort-word and max_indel edges ---------------------------------------------------------------------------------
LENGTHS = (1, 7, 8, 9, 16, 17, 254, 255, 256)


@functools.lru_cache(maxsize=None)
def lengths() -> VarSet:
    rng = np.random.default_rng(SEED + 2)
    text = pi.random_text(rng, 3000)
    ents, at = [], 3
    for l in LENGTHS + (3, 4):
        body = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, l))
        ents.append(make(f"ins{l}", text, at, (("=", 25), ("I", body), ("=", 12))))
        ents.append(make(f"ins{l}_again", text, at + 2, (("=", 23), ("I", body), ("=", 15)), MAPPED | REVERSE))
        ents.append(make(f"del{l}", text, at + 45, (("=", 20), ("D", l), ("=", 15))))
        at += 85 + l
    assert at < len(text)
    return attach("lengths", ents, text, settings(*BOTH, dict(max_indel=3), dict(max_indel=3, left_align=0), dict(max_indel=255), dict(max_indel=254)),
                  2)


# ---- 3. grouping: what is one allele and what is two -------------------------------------------------------------------------------
GROUP_AT = 60                                   # the anchor of every event of the set
GROUP_BASE = b"CGTTGCCTGGTC"                    # 12 bytes over C, G, T: behind an A it cannot move


@functools.lru_cache(maxsize=None)
def grouping() -> VarSet:
    rng = np.random.default_rng(SEED + 3)
    text = bytearray(pi.random_text(rng, 200))
    text[GROUP_AT:GROUP_AT + 8] = b"ACGTCGTA"   # anchor A; text[p] != text[p + l] for the deletions of 2 and 5 used below
    text = bytes(text)
    base = GROUP_BASE

    def change(k):
        return base[:k] + (b"G" if base[k] != 71 else b"T") + base[k + 1:]
    ents = []

    def add(name, ops, count, strands=(0,)):
        for k in range(count):
            s = strands[k % len(strands)]
            ents.append(make(f"{name}_{k}", text, 20 + k % 7, (("=", GROUP_AT + 1 - 20 - k % 7),) + ops + (("=", 30),), MAPPED | s))
    add("base", (("I", base),), 70, (0, REVERSE))                 # more than a wave of one allele, both strands
    add("lower", (("I", base.lower()),), 3)                       # letter case only: the same allele
    add("first_byte", (("I", change(0)),), 2)
    add("last_byte", (("I", change(11)),), 2, (REVERSE,))
    add("byte8", (("I", change(8)),), 3)                          # the first byte of the second sort word
    add("byte7", (("I", change(7)),), 1)
    add("non_acgt", (("I", base[:5] + b"N" + base[6:]),), 2)
    add("shorter", (("I", base[:11]),), 2)
    add("ins_and_del", (("I", b"GG"), ("D", 2)), 2)               # the deletion's anchor is GROUP_AT too
    add("del2", (("D", 2),), 3, (0, REVERSE))
    add("del5", (("D", 5),), 2)
    add("plain", (), 5)
    sets = settings(*BOTH, dict(min_alt_count=3), dict(min_alt_permille=30, hom_permille=700), dict(region=(GROUP_AT, GROUP_AT + 1)),
                    dict(region=(GROUP_AT + 1, 200)))
    return attach("grouping", ents, text, sets, 3)


# ---- 4. left alignment ----------------------------------------------------------------------------------------------------------------
REP_AT, REP_UNITS = 100, 40                      # (AC) x 40 at 100..179, G in front, T behind
HOMO_AT, HOMO_LEN = 300, 200                     # A x 200 at 300..499, C in front, G behind


@functools.lru_cache(maxsize=None)
def repeats() -> VarSet:
    rng = np.random.default_rng(SEED + 4)
    text = bytearray(pi.random_text(rng, 600))
    text[REP_AT - 1:REP_AT + 2 * REP_UNITS + 1] = b"G" + b"AC" * REP_UNITS + b"T"
    text[HOMO_AT - 1:HOMO_AT + HOMO_LEN + 1] = b"C" + b"A" * HOMO_LEN + b"G"
    text = bytes(text)
    ents = []
    for d in range(0, 2 * REP_UNITS - 1, 3):     # the same 2-base deletion written at every third column of the repeat
        ents.append(make(f"del_at{d}", text, 80, (("=", 20 + d), ("D", 2), ("=", 2 * REP_UNITS - 2 - d + 10)), MAPPED | (REVERSE if d % 2 else 0)))
    ents.append(make("ins_at_far_end", text, 80, (("=", 20 + 2 * REP_UNITS), ("I", b"AC"), ("=", 10))))
    ents.append(make("homopolymer_ins", text, 290, (("=", 10 + HOMO_LEN), ("I", b"A"), ("=", 12))))
    ents.append(make("homopolymer_ins_lower", text, 285, (("=", 15 + HOMO_LEN), ("I", b"a"), ("=", 9)), MAPPED | REVERSE))
    ents.append(make("homopolymer_del", text, 290, (("=", 10 + 130), ("D", 1), ("=", 69 + 12))))
    ents.append(make("mismatch_stops", text, 80, (("=", 20 + 30), ("X", b"T"), ("=", 29), ("D", 2), ("=", 28))))
    ents.append(make("i_before_d", text, 80, (("=", 20 + 40), ("I", b"AC"), ("D", 2), ("=", 48))))
    ents.append(make("begins_inside", text, REP_AT + 20, (("=", 30), ("D", 2), ("=", 38))))
    ents.append(make("begins_inside_ins", text, HOMO_AT + 50, (("=", 100), ("I", b"A"), ("=", 62))))
    ents.append(make("begins_at_repeat", text, REP_AT, (("=", 10), ("D", 2), ("=", 78))))     # the walk reaches column 0: open
    ents.append(make("begins_one_before", text, REP_AT - 1, (("=", 11), ("D", 2), ("=", 78))))
    sets = settings(*BOTH, dict(region=(130, 600)), dict(region=(130, 600), left_align=0), dict(region=(90, 120)),
                    dict(region=(90, 120), left_align=0), dict(min_alt_count=5), dict(min_alt_count=5, left_align=0))
    return attach("repeats", ents, text, sets, 4)


@functools.lru_cache(maxsize=None)
def text_start() -> VarSet:
    """shifts at ref_start == 0: to anchor -1 behind a leading insertion, and into the entry's first column"""
    text = b"AAAAAC" + b"GTCAGTTGCA" * 3
    ents = (make("shift_to_minus1", text, 0, (("I", b"G"), ("=", 5), ("I", b"A"), ("=", 20))),
            make("shift_to_minus1_del", text, 0, (("I", b"G"), ("=", 4), ("D", 1), ("=", 20))),
            make("open_at_0", text, 0, (("=", 5), ("I", b"A"), ("=", 20))),
            make("stops_at_1", text, 1, (("X", b"C"), ("=", 3), ("I", b"A"), ("=", 20))),
            make("d_first_at_0", text, 0, (("D", 2), ("=", 20))),
            make("plain", text, 0, (("=", 30),), MAPPED | REVERSE))
    return attach("text_start", ents, text, settings(*BOTH, dict(region=(0, 1)), dict(region=(0, 1), left_align=0)), 5)


# ---- 5. thresholds and counts ------------------------------------------------------------------------------------------------------
THR_AT, THR_DEPTH, THR_WITH = 40, 20, 5          # 5 of 20 reads carry the insertion: 250 permille exactly


@functools.lru_cache(maxsize=None)
def thresholds() -> VarSet:
    rng = np.random.default_rng(SEED + 6)
    text = bytearray(pi.random_text(rng, 160))
    text[THR_AT:THR_AT + 2] = b"AC"
    text[100:104] = b"ACGT"
    text = bytes(text)
    ents, quals = [], {}
    for k in range(THR_DEPTH):
        ops = (("=", THR_AT + 1 - 10),) + ((("I", b"GT"),) if k < THR_WITH else ()) + (("=", 30),)
        ents.append(make(f"t{k}", text, 10, ops, MAPPED | (REVERSE if k % 2 else 0)))
    # ref_count at 0: one read covers 100, three begin behind it with a deletion (anchored at 100 without left alignment)
    quals[len(ents)] = b"I" * 30
    ents.append(make("covers", text, 90, (("=", 30),)))
    for k in range(3):
        ents.append(make(f"d_first{k}", text, 101, (("D", 2), ("=", 25))))
    # min_base_qual takes the depth away under an insertion: 4 reads, the anchor base of 3 of them is of quality 2
    for k in range(4):
        e = make(f"low_anchor{k}", text, 130, (("=", 10), ("I", b"TT" if text[139] != 84 else b"GG"), ("=", 15)), MAPPED | (REVERSE if k == 3 else 0))
        q = bytearray(b"I" * qi.read_columns(e.A))
        if k < 3:
            q[9] = ord("#")
        quals[len(ents)] = bytes(q[::-1] if k == 3 else q)
        ents.append(e)
    sets = settings(dict(min_alt_permille=250), dict(min_alt_permille=251), dict(min_alt_count=5), dict(min_alt_count=6),
                    dict(hom_permille=250), dict(hom_permille=251), dict(hom_permille=0), dict(hom_permille=1000), dict(left_align=0),
                    dict(min_base_qual=20), dict(min_base_qual=20, left_align=0, min_alt_permille=1000), dict(min_depth=21),
                    dict(min_depth=20, min_alt_permille=250, min_alt_count=5))
    return attach("thresholds", ents, text, sets, 6, quals)


# ---- 6. everything else ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def errs() -> VarSet:
    """tests/pileup_qual_inputs.quality_errs(): every err 1..7 beside good entries that carry an insertion and a deletion"""
    s = qi.quality_errs()
    rng = np.random.default_rng(SEED + 7)
    more = (pi.on_text("err1_with_events", "==II==?==DD==", s.ref, 200, rng),             # err 4 needs 2^28 columns: the pileup's tests have it
            replace(pi.on_text("e", "==II====DD==", s.ref, 220, rng), name="err2_with_events", ref_end=0),
            pi.on_text("good_beside_them", "==II====DD==", s.ref, 200, rng, flags=MAPPED | REVERSE))
    quals = tuple(bytes(rng.integers(qi.Q_LO, qi.Q_HI + 1, qi.read_columns(e.A), dtype=np.uint8)) for e in more)
    return VarSet("errs", s.entries + more, s.read_start + (0,) * len(more), s.quals + quals, s.ref,
                  settings(*BOTH, dict(min_mapq=20), dict(min_mapq=20, min_base_qual=20)))


@functools.lru_cache(maxsize=None)
def plain_errs() -> VarSet:
    s = pi.errs()
    return attach("plain_errs", s.entries, s.ref, settings({}, dict(min_mapq=20, left_align=0)), 7)


@functools.lru_cache(maxsize=None)
def no_events() -> VarSet:
    rng = np.random.default_rng(SEED + 8)
    text = pi.random_text(rng, 120)
    ents = [make(f"m{k}", text, 5 * k, (("=", 20), ("X", bytes([other(text[5 * k + 20])])), ("=", 30)), MAPPED | (REVERSE if k % 2 else 0))
            for k in range(12)]
    return attach("no_events", ents, text, settings(*BOTH, dict(region=(40, 41)), dict(region=(7, 7))), 8)


@functools.lru_cache(maxsize=None)
def none_passing() -> VarSet:
    s = steps()
    return VarSet("none_passing", s.entries, s.read_start, s.quals, s.ref, settings(dict(min_alt_count=2), dict(min_depth=5), dict(region=(9, 9))))


@functools.lru_cache(maxsize=None)
def empty() -> VarSet:
    return VarSet("empty", (), (), (), pi.random_text(np.random.default_rng(SEED + 9), 50), settings(*BOTH, dict(region=(20, 20))))


@functools.lru_cache(maxsize=None)
def shapes() -> VarSet:
    """tests/pileup_inputs.shapes() and .edges(): the pileup's own column counts and run placements, their bytes drawn"""
    s = pi.shapes()
    return attach("shapes", s.entries, s.ref, settings(*BOTH, dict(max_indel=100, min_mapq=20)), 10)


@functools.lru_cache(maxsize=None)
def pileup_edges() -> VarSet:
    s = pi.edges()
    return attach("pileup_edges", s.entries, s.ref, settings(*BOTH, dict(region=(0, 1)), dict(region=(1, 40), left_align=0)), 11)


def random_entries(n: int, text_len: int, seed: int, max_cols: int = 60) -> VarSet:
    """n entries of random classes on a text of two letters, so that shifts are common"""
    rng = np.random.default_rng(SEED + seed)
    text = bytes(b"AC"[int(x)] for x in rng.integers(0, 2, text_len))
    ents = []
    for k in range(n):
        cl = pi.random_classes(rng, int(rng.integers(1, max_cols + 1)))
        cl = "".join(c if rng.integers(0, 4) else "=" for c in cl)      # one column in four becomes a match: shorter runs
        used = sum(c != "I" for c in cl)
        ents.append(pi.on_text(f"r{k}", cl, text, int(rng.integers(0, text_len - used + 1)), rng, read=b"AC",
                               flags=MAPPED | (REVERSE if rng.integers(0, 2) else 0), mapq=int(rng.integers(0, 61))))
    return attach(f"random{n}", ents, text, settings(dict(min_alt_count=2, min_alt_permille=20), dict(left_align=0, min_mapq=20, min_base_qual=10)),
                  seed)


@functools.lru_cache(maxsize=None)
def random_small() -> VarSet:
    return replace(random_entries(600, 150, 12), name="random")


SET_NAMES = ("steps", "lengths", "grouping", "repeats", "text_start", "thresholds", "errs", "plain_errs", "no_events", "none_passing", "empty",
             "shapes", "pileup_edges", "random")


@functools.lru_cache(maxsize=None)
def all_sets() -> tuple:
    return (steps(), lengths(), grouping(), repeats(), text_start(), thresholds(), errs(), plain_errs(), no_events(), none_passing(), empty(),
            shapes(), pileup_edges(), random_small())


# ---- planted variants: a 3 kb construct sequenced at 30x ----------------------------------------------------------------------------
# (anchor or position, kind, bytes): an SNV's new base, the inserted bytes, the deleted length.  The bytes around each indel are
# fixed so that the anchor given is the leftmost one: the (AC) x 6 and T x 8 repeats start right behind their anchors.
PLANTED = ((300, 1, b"*"), (600, 2, b"GGT"), (900, 1, b"*"), (1200, 3, 3), (1500, 1, b"*"), (1800, 2, b"CATTG"), (2100, 3, 4), (2400, 1, b"*"),
           (2599, 3, 2), (2749, 2, b"T"))
PLANTED_LEN, PLANTED_READ, PLANTED_READS = 3000, 100, 900
PLANTED_CALL = dict(min_alt_permille=300, min_depth=4, hom_permille=700)


@functools.lru_cache(maxsize=None)
def planted() -> dict:
    """-> T: the designed text; sample: T with PLANTED put in; variants: PLANTED with each SNV's base filled in; reads: 900 reads of
    100 bases drawn evenly from the sample, every second one reverse-complemented; fastq: the same as a FASTQ image, quality 'I'"""
    rng = np.random.default_rng(SEED + 20)
    T = bytearray(pi.random_text(rng, PLANTED_LEN))
    T[600:602] = b"AC"                           # GGT behind the A: its last byte differs from the anchor
    T[1800:1802] = b"CA"                         # CATTG behind the C
    T[1200:1205] = b"GACTT"                      # ACT goes: G != T
    T[2100:2106] = b"CAGTTA"                     # AGTT goes: C != T
    T[2599:2613] = b"G" + b"AC" * 6 + b"T"       # one AC of six goes: wherever the mapper writes it, it belongs behind the G
    T[2749:2759] = b"G" + b"T" * 8 + b"A"        # one more T
    T = bytes(T)
    variants, sample, at = [], bytearray(), 0
    for p, kind, what in PLANTED:
        if kind == 1:
            what = bytes([other(T[p])])
            sample += T[at:p] + what
            at = p + 1
        elif kind == 2:
            sample += T[at:p + 1] + what
            at = p + 1
        else:
            sample += T[at:p + 1]
            at = p + 1 + what
        variants.append((p, kind, what))
    sample = bytes(sample + T[at:])
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    reads = []
    for k in range(PLANTED_READS):
        start = k * (len(sample) - PLANTED_READ) // (PLANTED_READS - 1)
        r = sample[start:start + PLANTED_READ]
        reads.append(r.translate(comp)[::-1] if k % 2 else r)
    fastq = b"".join(b"@r%d\n" % k + r + b"\n+\n" + b"I" * len(r) + b"\n" for k, r in enumerate(reads))
    return dict(T=T, sample=sample, variants=tuple(variants), reads=tuple(reads), fastq=fastq)


def called(rows) -> list:
    """vcf Rows -> [(anchor or position, kind, bytes or deleted length)] as PLANTED spells them"""
    out = []
    for r in rows:
        if len(r.ref) == len(r.alt) == 1:
            out.append((r.pos, 1, r.alt))
        elif len(r.ref) == 1:
            out.append((r.pos, 2, r.alt[1:]))
        else:
            out.append((r.pos, 3, len(r.ref) - 1))
    return out


def pack(s: VarSet) -> dict:
    """the arrays polyhip_call_variants takes"""
    p = pi.pack(s.entries)
    off = np.zeros(len(s.entries) + 1, np.uint64)
    off[1:] = np.cumsum([len(q) for q in s.quals], dtype=np.uint64)
    p.update(read_start=np.array(s.read_start, np.uint32), qual=np.frombuffer(b"".join(s.quals), np.uint8), qual_off=off)
    return p


def oracle_args(s: VarSet, with_qual: bool = True) -> tuple:
    p = pack(s)
    return (p["flags"], p["mapq"], p["ref_start"], p["ref_end"], p["read_start"], p["alnA"], p["alnB"], p["aln_off"],
            p["qual"] if with_qual else None, p["qual_off"], s.ref)
