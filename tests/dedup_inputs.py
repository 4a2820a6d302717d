"""Hand-built inputs of polyhip_mark_duplicates and polyhip_coord_order (tests/test_dedup_cpu.py and tests/test_dedup_gpu.py
share them): arrays only, no text, no index, no mapping.  What each set holds is asserted in tests/test_dedup_cpu.py.  Callers
leave what they get unchanged."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

SEED = 808
MAPPED, REVERSE = 1, 2
SIZES = (1, 2, 255, 256, 257, 4095, 4096, 4097)             # block and radix-tile edges
SET_SIZES = (1, 2, 63, 64, 65, 257, 4097)                   # members of one end set; 4097 spans a radix tile
QUAL_LENGTHS = (0, 1, 63, 64, 65, 1000)
TOP = (1 << 32) - 1


@dataclass(frozen=True)
class Set:
    name: str
    flags: np.ndarray
    rid: np.ndarray | None
    ref_start: np.ndarray
    ref_end: np.ndarray
    read_start: np.ndarray
    read_end: np.ndarray
    read_len: np.ndarray
    weight: np.ndarray | None
    qual: np.ndarray | None
    qual_off: np.ndarray | None
    modes: tuple                 # of dicts: paired, and min_weight_qual / qual_offset where the set has quality strings

    def kwargs(self, mode: dict) -> dict:
        """what both ``dedup.mark_packed`` and ``dedup_oracle.mark`` take"""
        return dict(flags=self.flags, ref_start=self.ref_start, ref_end=self.ref_end, read_start=self.read_start,
                    read_end=self.read_end, read_len=self.read_len, rid=self.rid, weight=self.weight, qual=self.qual,
                    qual_off=self.qual_off, **mode)

    def u(self) -> list:
        """the signed end position of every entry, whatever its flags"""
        return [int(fe) - 1 + int(rl) - int(re) if f & REVERSE else int(fs) - int(rs)
                for f, fs, fe, rs, re, rl in zip(self.flags, self.ref_start, self.ref_end, self.read_start, self.read_end, self.read_len)]


SINGLE, PAIRED, BOTH = ({"paired": False},), ({"paired": True},), ({"paired": False}, {"paired": True})


class Rows:
    def __init__(self):
        self.rows, self.quals = [], []

    def add(self, flags, rid, fs, fe, rs, re, rl, w=0, q=None):
        self.rows.append((flags, rid, fs, fe, rs, re, rl, w))
        self.quals.append(q)
        return self

    def fwd(self, u, clip=0, length=50, w=0, rid=0, q=None):
        """a forward entry whose unclipped 5' end is u: the first ``clip`` bases are soft-clipped"""
        return self.add(MAPPED, rid, u + clip, u + length, clip, length, length, w, q)

    def rev(self, u, clip=0, length=50, w=0, rid=0, q=None):
        """a reverse entry whose unclipped 5' end is u (>= length - 1): the last ``clip`` bases of the oriented read are clipped"""
        return self.add(MAPPED | REVERSE, rid, u + 1 - length, u + 1 - clip, 0, length - clip, length, w, q)

    def unmapped(self, w=0, q=None, length=50):
        return self.add(0, 7, 9, 3, 8, 2, length, w, q)             # arrays that would be err 2 if they were judged

    def bad2(self, u, w=0, strand=0, q=None, length=50):
        """mapped at the forward end u, but read_start > read_end"""
        return self.add(MAPPED | (REVERSE if strand else 0), 0, u + 5, u + length, 5, 4, length, w, q)

    def done(self, name, modes, with_rid=True, with_weight=True) -> Set:
        c = list(zip(*self.rows)) if self.rows else [[]] * 8
        a = lambda k: np.array(c[k], dtype=np.uint64).astype(np.uint32)       # noqa: E731
        qual = qual_off = None
        if any(q is not None for q in self.quals):
            qs = [q if q is not None else b"" for q in self.quals]
            qual = np.frombuffer(b"".join(qs), np.uint8)
            qual_off = np.zeros(len(qs) + 1, np.uint64)
            qual_off[1:] = np.cumsum([len(q) for q in qs])
            with_weight = False
        return Set(name, a(0), a(1) if with_rid else None, a(2), a(3), a(4), a(5), a(6), a(7) if with_weight else None, qual, qual_off,
                   tuple(modes))


def _random_rows(rng, n, positions=50, contigs=3, bad=True) -> Rows:
    r = Rows()
    for _ in range(n):
        x = rng.random()
        u, w, clip = 100 + int(rng.integers(0, positions)), int(rng.integers(0, 40)), int(rng.integers(0, 4))
        rid = int(rng.integers(0, contigs))
        if bad and x < 0.05:
            r.unmapped(w)
        elif bad and x < 0.07:
            r.bad2(u, w, int(rng.integers(0, 2)))
        elif rng.random() < 0.5:
            r.fwd(u, clip, 50, w, rid)
        else:
            r.rev(u, clip, 50, w, rid)
    return r


@functools.lru_cache(maxsize=None)
def sized(n: int) -> Set:
    rng = np.random.default_rng(SEED + n)
    return _random_rows(rng, n, positions=7, contigs=2).done(f"n{n}", SINGLE if n % 2 else BOTH)


@functools.lru_cache(maxsize=None)
def end_set(k: int) -> Set:
    """k entries at one end among 40 others; the greatest weight sits in the middle of the k"""
    rng = np.random.default_rng(SEED + 100 + k)
    r = _random_rows(rng, 20, positions=5, contigs=1, bad=False)
    for j in range(k):
        r.fwd(300, j % 4, 50, 1000 if j == k // 2 else int(rng.integers(0, 999)))
    for j in range(20):
        r.rev(300 + j % 3, 0, 50, j)
    return r.done(f"end_set{k}", SINGLE)


@functools.lru_cache(maxsize=None)
def one_set() -> Set:
    """10,000 entries that are one end set: every digit of every pass is the same for all of them"""
    rng = np.random.default_rng(SEED + 1)
    r = Rows()
    for j in range(10000):
        r.fwd(5000, j % 3, 100, int(rng.integers(0, 3)))
    return r.done("one_set_10000", BOTH)


@functools.lru_cache(maxsize=None)
def weights() -> tuple:
    eq = Rows()
    for j in range(5):
        eq.fwd(100, j, w=9)
    bit0 = Rows().fwd(100, w=6).fwd(100, w=7).fwd(100, w=6).rev(100, w=1).rev(100, w=0)
    bit31 = Rows().fwd(100, w=5).fwd(100, w=1 << 31).fwd(100, w=(1 << 31) - 1).rev(100, w=TOP).rev(100, w=TOP - 1)
    last = Rows()
    for j in range(300):
        last.fwd(100, w=j)
    # two pairs at the same two ends: W = 2^32 + 1 against 2^32 + 2 (bit 32 and bit 0 or 1), and one lighter pair
    big = Rows().fwd(100, w=TOP).rev(400, w=2).fwd(100, w=TOP).rev(400, w=3).fwd(100, w=TOP).rev(400, w=0)
    nul = Rows().fwd(100).fwd(100, clip=2).fwd(100)
    return (eq.done("w_equal", SINGLE), bit0.done("w_bit0", SINGLE), bit31.done("w_bit31", SINGLE), last.done("w_winner_last", BOTH),
            big.done("w_pair_sum_bit32", PAIRED), nul.done("w_null", SINGLE, with_weight=False))


@functools.lru_cache(maxsize=None)
def ends() -> tuple:
    neg = Rows().fwd(-5, clip=10, w=1).fwd(-5, clip=7, w=2).fwd(-4, clip=10, w=3).fwd(0, w=1)
    strands = Rows().fwd(100, w=1).rev(100, w=2).fwd(100, w=3).rev(100, w=4)
    # reverse entries with different ref_end and clips, the same u: one set;  forward entries with the same ref_start and
    # different read_start: different u
    merge = Rows().rev(200, clip=0, w=1).rev(200, clip=3, w=2).rev(200, clip=9, length=70, w=3)
    nomerge = Rows().add(MAPPED, 0, 100, 150, 0, 50, 50, 1).add(MAPPED, 0, 100, 147, 3, 50, 50, 2).add(MAPPED, 0, 100, 150, 0, 50, 50, 3)
    wide = Rows()
    for w in (1, 2):
        wide.add(MAPPED | REVERSE, 0, 0, TOP, 0, 10, TOP, w)                # u = 2^33 - 13: the biased u needs bit 33
        wide.add(MAPPED, 0, TOP, TOP, 0, 0, 0, w)                            # u = 2^32 - 1: the biased u needs bit 32
        wide.add(MAPPED, 0, 0, 1, TOP - 1, TOP, TOP, w)                      # u = -(2^32 - 2)
        wide.add(MAPPED | REVERSE, 0, 0, 0, 0, 0, 0, w)                      # u = -1
    ridonly = Rows().fwd(100, w=1, rid=0).fwd(100, w=2, rid=1).fwd(100, w=3, rid=0).fwd(100, w=4, rid=1).fwd(100, w=1, rid=2)
    extremes = Rows().fwd(100, w=1, rid=TOP).fwd(100, w=2, rid=0).fwd(100, w=3, rid=TOP).rev(100, w=4, rid=0).fwd(100, w=0, rid=0).rev(100, w=9, rid=TOP)
    null = Rows().fwd(100, w=1, rid=5).fwd(100, w=2, rid=6).rev(100, w=1, rid=5)
    return (neg.done("u_negative", SINGLE), strands.done("strands_equal_u", SINGLE), merge.done("reverse_clips_merge", SINGLE),
            nomerge.done("forward_clips_differ", SINGLE), wide.done("u_wide", BOTH), ridonly.done("rid_only", SINGLE),
            extremes.done("rid_extremes", BOTH), null.done("rid_null", SINGLE, with_rid=False))


@functools.lru_cache(maxsize=None)
def pairs() -> tuple:
    # read 1 left in the first pair, read 2 left in the second: one key
    swapped = Rows().fwd(100, w=5).rev(400, w=5).rev(400, w=1).fwd(100, w=1)
    same_e = Rows().fwd(100, w=1).fwd(100, clip=2, w=1).fwd(100, w=4).fwd(100, w=4).fwd(100, w=4).fwd(100, clip=1, w=4)
    cross = Rows().fwd(100, rid=1, w=1).rev(400, rid=0, w=1).rev(400, rid=0, w=2).fwd(100, rid=1, w=2).fwd(100, rid=0, w=9).rev(400, rid=0, w=9)
    orient = Rows()
    for rep in range(2):
        orient.fwd(100, w=rep).rev(400, w=1)           # FR
        orient.rev(100, w=rep).fwd(400, w=1)           # RF
        orient.fwd(100, w=rep).fwd(400, w=1)           # FF
        orient.rev(100, w=rep).rev(400, w=1)           # RR
    # a fragment (its mate is unmapped) at the end of a pair that is itself a duplicate, with the greatest weight there
    frag = Rows().fwd(100, w=9).rev(400, w=9).fwd(100, w=1).rev(400, w=1).fwd(100, w=1000).unmapped().unmapped().rev(400, w=1000)
    alone = Rows().fwd(100, w=3).unmapped().fwd(100, w=8).unmapped().unmapped().fwd(100, w=8).rev(100, w=1).bad2(100)
    broken = Rows().fwd(100, w=1).unmapped().fwd(100, w=2).bad2(400).fwd(100, w=3).rev(400, w=3).fwd(100, w=1).rev(400, w=1).unmapped().unmapped()
    return (swapped.done("pair_read2_left", PAIRED), same_e.done("pair_mates_same_end", PAIRED), cross.done("pair_two_contigs", PAIRED),
            orient.done("pair_orientations", PAIRED), frag.done("fragment_at_duplicate_pair", PAIRED),
            alone.done("fragments_alone", PAIRED), broken.done("pair_mate_unmapped_or_err2", BOTH))


def _q(rng, length, lo=0, hi=93, offset=33) -> bytes:
    return bytes(int(x) + offset for x in rng.integers(lo, hi + 1, length))


@functools.lru_cache(maxsize=None)
def qualities() -> tuple:
    rng = np.random.default_rng(SEED + 2)
    modes = tuple({"paired": p, "min_weight_qual": m, "qual_offset": 33} for p in (False, True) for m in (0, 15, 93))
    r = Rows()
    for length in QUAL_LENGTHS:
        for copy in range(4):
            r.fwd(1000 + length, length=length, q=_q(rng, length))
    r.fwd(50, length=64, q=bytes([33 + 93]) * 64).fwd(50, length=64, q=bytes([33 + 14]) * 64 + b"")     # 93 and 14: the two thresholds
    r.fwd(50, length=64, q=bytes([33 + 15]) * 64).fwd(50, length=64, q=bytes([33]) * 64)
    lengths = r.done("qual_lengths", modes)
    e = Rows()
    good = _q(rng, 70)
    e.fwd(100, length=70, q=good).fwd(100, length=70, q=good[:69]).fwd(100, length=70, q=good + b"I")           # 0, 6, 6
    e.fwd(100, length=70, q=good[:65] + bytes([32]) + good[66:]).fwd(100, length=70, q=bytes([33 + 94]) + good[1:])   # 7, 7
    e.bad2(100, length=70, q=good[:3]).unmapped(length=70, q=b"\x00\x01").fwd(100, length=70, q=good)          # 2 before 6; never read
    e.fwd(100, length=0, q=b"x").fwd(100, length=70, q=_q(rng, 70, 90, 93))
    errs = e.done("qual_errs", modes)
    o = Rows().fwd(100, length=10, q=bytes(range(64, 74))).fwd(100, length=10, q=bytes([64 + 93]) * 10).fwd(100, length=10, q=bytes([63]) * 10)
    offset = o.done("qual_offset64", ({"paired": False, "min_weight_qual": 5, "qual_offset": 64},
                                      {"paired": False, "min_weight_qual": 0, "qual_offset": 162}))
    return lengths, errs, offset


@functools.lru_cache(maxsize=None)
def errs() -> Set:
    """err 2 in each of its three forms; one of them sits between two duplicates of each other"""
    r = Rows().fwd(100, w=1).bad2(100, w=50).fwd(100, w=2)
    r.add(MAPPED, 0, 100, 150, 0, 51, 50, 60)                   # read_end > read_len
    r.add(MAPPED, 0, 151, 150, 0, 50, 50, 70)                   # ref_start > ref_end
    r.add(MAPPED | REVERSE, 0, 100, 150, 0, 51, 50, 80).unmapped(w=90).fwd(100, w=2)
    return r.done("errs", BOTH)


@functools.lru_cache(maxsize=None)
def random_set() -> Set:
    """20,000 entries over 50 positions and 3 contigs, as reads and as pairs"""
    return _random_rows(np.random.default_rng(SEED), 20000).done("random_20000", BOTH)


@functools.lru_cache(maxsize=None)
def empty() -> Set:
    return Rows().done("empty", BOTH)


@functools.lru_cache(maxsize=None)
def all_sets() -> tuple:
    return (tuple(sized(n) for n in SIZES) + tuple(end_set(k) for k in SET_SIZES) + (one_set(),) + weights() + ends() + pairs() +
            qualities() + (errs(), random_set(), empty()))


def by_name(name: str) -> Set:
    return {s.name: s for s in all_sets()}[name]


PLANTED_TEMPLATES, PLANTED_COPIES, PLANTED_READ, PLANTED_MIN_ALT = 20, 5, 100, 3
PLANTED_GAPS = 1       # of map_affine_inputs.GAPS: open -12, extend -2; with a cheap gap the aligner reaches into the junk bases


@functools.lru_cache(maxsize=None)
def planted(seed: int = SEED + 3) -> dict:
    """-> T: a 4 kb text; reads: 300 reads of 100 bases as sequenced.  Reads 0..199 are drawn every 19 bases, every second
    one from the reverse strand; read ``template[t]`` = 10 t + t % 2 (t < 20) is a template and carries one planted error, at
    ``sites[t]``.  Reads 200 + 5 t .. 204 + 5 t are copies of template t: the same window and strand, the planted error, one
    substitution of their own, and the first 1..5 bases as sequenced replaced by bases that match neither the text there nor
    its neighbours, which a local alignment clips (tests/test_dedup_cpu.py asserts that the mapper's oracle does)."""
    rng = np.random.default_rng(seed)
    T = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, 4000))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    other = lambda b: b"CGTA"[b"ACGT".index(b)]                            # noqa: E731
    starts = [50 + 19 * k for k in range(200)]
    windows, sites, alts = [bytearray(T[s:s + PLANTED_READ]) for s in starts], [], []
    for t in range(PLANTED_TEMPLATES):
        k = 10 * t + t % 2
        windows[k][50] = other(windows[k][50])
        sites.append(starts[k] + 50)
        alts.append(windows[k][50])
    sequenced = lambda w, k: bytes(w).translate(comp)[::-1] if k % 2 else bytes(w)      # noqa: E731
    reads = [sequenced(w, k) for k, w in enumerate(windows)]
    for t in range(PLANTED_TEMPLATES):
        k = 10 * t + t % 2
        for j in range(PLANTED_COPIES):
            w = bytearray(windows[k])
            at = int(rng.choice([x for x in range(20, 80) if x != 50]))
            w[at] = other(w[at])
            for x in (range(PLANTED_READ - 1 - j, PLANTED_READ) if k % 2 else range(j + 1)):      # the first j + 1 bases as sequenced
                p = starts[k] + x
                w[x] = next(b for b in b"ACGT" if b not in T[p - 1:p + 2])
            reads.append(sequenced(w, k))
    return dict(T=T, reads=reads, starts=starts, sites=sites, alts=alts, template=[10 * t + t % 2 for t in range(PLANTED_TEMPLATES)])


def sam_flags(s: Set) -> np.ndarray:
    """a SAM FLAG word per entry for polyhip_coord_order: 0x4 on the unmapped entries, 0x10 on the reverse ones"""
    return np.where(s.flags & MAPPED, (s.flags & REVERSE) << 3, 4).astype(np.uint32)
