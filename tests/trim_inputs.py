"""Hand-built inputs of the trimming tests.  A set names its reads (for pairs: both mates), their quality strings, the adapters
and the parameter sets (``modes``) it is run with; what each set promises is asserted on the oracle in tests/test_trim_cpu.py
and the GPU is held to the oracle on every set in tests/test_trim_gpu.py."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

SEED = 4242
ADAPTER = b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"       # 33 bytes: the TruSeq read-1 adapter
ADAPTER2 = b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT"      # 33 bytes: the TruSeq read-2 adapter
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 300, 5000)
ADAPTER_LENGTHS = (1, 3, 32, 63, 64)
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def rc(s: bytes) -> bytes:
    return s.translate(_RC)[::-1]


def dna(rng, n: int) -> bytes:
    return bytes(b"ACGT"[x] for x in rng.integers(0, 4, n))


def tc(rng, n: int) -> bytes:
    """only T and C: no byte of it starts one of the adapters"""
    return bytes(b"TC"[x] for x in rng.integers(0, 2, n))


def phred(Q, offset: int = 33) -> bytes:
    return bytes(q + offset for q in Q)


def spoil(s: bytes, at) -> bytes:
    out = bytearray(s)
    for i in at:
        out[i] = {65: 67, 67: 71, 71: 84, 84: 65}[out[i]]
    return bytes(out)


def pack(strings, lead: int = 0):
    """(bytes, offsets): the strings back to back behind `lead` bytes that belong to no read"""
    offs = np.zeros(len(strings) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in strings], dtype=np.uint64)
    return np.frombuffer(b"#" * lead + b"".join(strings) + b"#", np.uint8).copy(), offs + np.uint64(lead)


def _set(name, reads, quals, adapters, modes, **more):
    return SimpleNamespace(name=name, reads=list(reads), quals=None if quals is None else list(quals), adapters=list(adapters),
                           modes=list(modes), **more)


def _pairs(name, reads1, reads2, quals1, quals2, adapters, modes, **more):
    return SimpleNamespace(name=name, reads1=list(reads1), reads2=list(reads2), quals1=None if quals1 is None else list(quals1),
                           quals2=None if quals2 is None else list(quals2), adapters=list(adapters), modes=list(modes), **more)


def _noisy_quals(rng, reads):
    """high in the middle, a low run of random length at each end, a tenth of everything low"""
    out = []
    for r in reads:
        m = len(r)
        Q = rng.integers(25, 41, m)
        Q[rng.random(m) < 0.1] = 8
        lo5, lo3 = (int(x) for x in rng.integers(0, 12, 2))
        Q[:min(lo5, m)] = rng.integers(2, 15, min(lo5, m))
        if lo3 and m:
            Q[max(m - lo3, 0):] = rng.integers(2, 15, m - max(m - lo3, 0))
        out.append(phred(int(q) for q in Q))
    return out


@functools.lru_cache(maxsize=None)
def lengths():
    """every length of LENGTHS, three reads each: as it is, ending in a whole adapter, ending in a 9-byte prefix of it"""
    rng = np.random.default_rng(SEED)
    reads = []
    for m in LENGTHS:
        reads.append(dna(rng, m))
        reads.append((dna(rng, max(m - 33, 0)) + ADAPTER)[:m] if m >= 33 else dna(rng, m))
        reads.append(dna(rng, max(m - 9, 0)) + ADAPTER[:min(9, m)])
    return _set("lengths", reads, _noisy_quals(rng, reads), [ADAPTER],
                [dict(min_qual_3p=20, min_qual_5p=20), dict(min_qual_3p=20), dict(), dict(min_qual_5p=30, min_len=50, adapter_err_pct=0)])


@functools.lru_cache(maxsize=None)
def adapter_lengths():
    """adapters of 1, 3, 32, 63 and 64 bytes; per adapter a read that holds all of it at 40, one that ends in its first half,
    one that holds it with a tenth of its bytes changed"""
    rng = np.random.default_rng(SEED + 1)
    ads = [dna(rng, p) for p in ADAPTER_LENGTHS]
    reads = []
    for a in ads:
        p = len(a)
        reads.append(dna(rng, 40) + a + dna(rng, 97))
        reads.append(dna(rng, 150) + a[:(p + 1) // 2])
        reads.append(dna(rng, 70) + spoil(a, range(3, p, 10)) + dna(rng, 20))
    reads.append(dna(rng, 200))
    return _set("adapter_lengths", reads, None, ads, [dict(min_overlap=1, adapter_err_pct=0), dict(min_overlap=3, adapter_err_pct=10),
                                                         dict(min_overlap=32, adapter_err_pct=10), dict(min_overlap=64, adapter_err_pct=100)])


@functools.lru_cache(maxsize=None)
def adapter_places():
    """0: the read starts with the adapter (an empty read).  1, 2: the adapter straddles the first and the second step edge.
    3: adapter 0 at 70 while adapter 1 all but matches at 10.  4: the other way round.  5: both adapters match at 30.  6: lower
    case and N inside the adapter.  7: a hit behind a quality cut at the 5' end, in the step that starts at a."""
    rng = np.random.default_rng(SEED + 2)
    A, B = ADAPTER, ADAPTER2
    near = lambda x: spoil(x, range(0, 33, 6))             # noqa: E731  six of 33 changed: 18 %
    low = bytearray(A.lower())
    low[5], low[20] = ord("N"), ord("n")
    reads = [A + dna(rng, 60), dna(rng, 50) + A + dna(rng, 30), dna(rng, 120) + A + dna(rng, 10),
             dna(rng, 10) + near(B) + dna(rng, 27) + A + dna(rng, 20), dna(rng, 10) + near(A) + dna(rng, 27) + B + dna(rng, 20),
             dna(rng, 30) + A[:13], dna(rng, 45) + bytes(low) + dna(rng, 30), dna(rng, 90) + A + dna(rng, 5)]
    assert A[:13] == B[:13] and A[13] != B[13]            # the read ends in what both adapters start with: both match at 30
    quals = [phred([35] * len(r)) for r in reads]
    quals[7] = phred([5] * 20 + [35] * (len(reads[7]) - 20))
    return _set("adapter_places", reads, quals, [A, B], [dict(min_qual_5p=20), dict(min_qual_5p=20, adapter_err_pct=0, min_overlap=5)])


@functools.lru_cache(maxsize=None)
def budgets():
    """a read that ends in the first L bytes of the adapter with x of them changed: L = 9, 10, 19, 20 at 10 %"""
    rng = np.random.default_rng(SEED + 3)
    reads, want = [], []
    for L, x in ((9, 0), (9, 1), (10, 1), (10, 2), (19, 1), (19, 2), (20, 2), (20, 3)):
        reads.append(tc(rng, 60) + spoil(ADAPTER[:L], range(1, 1 + 3 * x, 3)))
        want.append(100 * x <= 10 * L)
    return _set("budgets", reads, None, [ADAPTER], [dict(min_overlap=9, adapter_err_pct=10)], hit=want)


@functools.lru_cache(maxsize=None)
def many_adapters():
    """255 adapters of 12 bytes; read i ends in adapter (17 * i) % 255 from byte 60 on, the last read in none"""
    rng = np.random.default_rng(SEED + 4)
    ads = []
    while len(ads) < 255:
        a = dna(rng, 12)
        if a not in ads:
            ads.append(a)
    which = [(17 * i) % 255 for i in range(40)]
    which[3] = 254
    reads = [dna(rng, 60) + ads[t] + dna(rng, 8) for t in which] + [dna(rng, 80)]
    return _set("many_adapters", reads, None, ads, [dict(min_overlap=12, adapter_err_pct=0)], which=which)


@functools.lru_cache(maxsize=None)
def quality_edges():
    """reads of 200 bytes of Q 35 with a run of Q 2 of c bytes at one end, c around the edges of the 64-column steps; then the
    walks' own cases: a dip that goes negative and would recover, ties of the greatest sum, all low, all high"""
    cuts = (1, 63, 64, 65, 127, 128, 129)
    reads, quals = [], []
    for c in cuts:
        quals.append(phred([35] * (200 - c) + [2] * c))
        quals.append(phred([2] * c + [35] * (200 - c)))
    # a good base inside the low run, one step in: the walk goes on over it (sum stays >= 0)
    quals.append(phred([35] * 120 + [2] * 10 + [30] + [2] * 69))
    quals.append(phred([2] * 69 + [30] + [2] * 10 + [35] * 120))
    quals.append(phred([2] * 200))
    quals.append(phred([40] * 200))
    quals.append(phred([20] * 200))
    reads = [b"ACGT" * 50] * len(quals)
    return _set("quality_edges", reads, quals, [], [dict(min_qual_3p=20, min_qual_5p=20), dict(min_qual_3p=3), dict(min_qual_5p=93)], cuts=cuts)


@functools.lru_cache(maxsize=None)
def errs():
    """err 1 and err 2 next to good reads; the bad ones also hold an adapter and low ends, which nobody looks at"""
    r = b"ACGTACGTAC" + ADAPTER + b"GG"
    m = len(r)
    good = phred([30] * m)
    quals = [good, good[:-1], good, good + b"I", phred([30] * (m - 1)) + bytes([32]), good, phred([30] * (m - 1)) + bytes([33 + 94]),
             b"", bytes([33 + 93]) * m, bytes([33]) * m]
    return _set("errs", [r] * len(quals), quals, [ADAPTER], [dict(min_qual_3p=20, min_qual_5p=20, min_len=5)])


@functools.lru_cache(maxsize=None)
def no_qual():
    rng = np.random.default_rng(SEED + 5)
    reads = [dna(rng, 70) + ADAPTER[:k] for k in (0, 2, 3, 10, 33)] + [b"", b"acgtn" * 10 + ADAPTER.lower()]
    return _set("no_qual", reads, None, [ADAPTER], [dict(), dict(min_len=71)])


@functools.lru_cache(maxsize=None)
def phred64():
    """Q 40 with a tail of Q 3 at offset 64; at offset 33 the same bytes are Q 71 and Q 34, at 162 they are out of range"""
    rng = np.random.default_rng(SEED + 6)
    reads = [dna(rng, m) for m in (30, 100, 150)]
    quals = [phred([40] * (len(r) - 8) + [3] * 8, 64) for r in reads]
    return _set("phred64", reads, quals, [], [dict(qual_offset=64, min_qual_3p=20), dict(qual_offset=33, min_qual_3p=20),
                                               dict(qual_offset=162, min_qual_3p=20)])


@functools.lru_cache(maxsize=None)
def min_len_edges():
    """what is kept is 40 bytes: min_len 40 keeps it, 41 does not"""
    rng = np.random.default_rng(SEED + 7)
    reads = [tc(rng, 40) + ADAPTER, tc(rng, 50), tc(rng, 40)]
    quals = [phred([35] * len(reads[0])), phred([2] * 6 + [35] * 40 + [2] * 4), phred([35] * 40)]
    return _set("min_len_edges", reads, quals, [ADAPTER], [dict(min_qual_3p=20, min_qual_5p=20, min_len=40),
                                                           dict(min_qual_3p=20, min_qual_5p=20, min_len=41)])


@functools.lru_cache(maxsize=None)
def many_small():
    """70,000 reads of 5 bytes: more reads than resident waves, more than one tile of the scan"""
    rng = np.random.default_rng(SEED + 8)
    codes = rng.integers(0, 4, (70_000, 5))
    Q = rng.integers(2, 41, (70_000, 5))
    reads = [bytes(b"ACGT"[x] for x in row) for row in codes]
    quals = [phred(int(q) for q in row) for row in Q]
    return _set("many_small", reads, quals, [b"ACG"], [dict(min_qual_3p=15, min_overlap=2, adapter_err_pct=0, min_len=2)])


@functools.lru_cache(maxsize=None)
def shifted():
    """the batch of `lengths`, behind 17 bytes (sequences) and 5 bytes (qualities) that belong to no read"""
    s = lengths()
    return _set("shifted", s.reads, s.quals, s.adapters, s.modes[:1], lead=(17, 5))


def single_sets():
    return [lengths(), adapter_lengths(), adapter_places(), budgets(), many_adapters(), quality_edges(), errs(), no_qual(), phred64(),
            min_len_edges(), shifted()]


# ---------------------------------------------------------------- pairs
def mates(T: bytes, start: int, insert: int, m1: int, m2: int, rng, ad1=ADAPTER, ad2=ADAPTER2):
    """the two reads of the fragment T[start, start + insert): past its end a read runs into the adapter, then into noise"""
    frag = T[start:start + insert]
    return (frag + ad1 + dna(rng, m1))[:m1], (rc(frag) + ad2 + dna(rng, m2))[:m2]


@functools.lru_cache(maxsize=None)
def pairs():
    """0: insert 20 = pair_min_overlap.  1: insert 19, one less: nothing found.  2: insert 100 = both lengths, nothing is cut.
    3: mates of 100 and 60 bytes, insert 60 = min(m1, m2): only mate 1 is cut.  4: mates of 100 and 60, insert 45.  5: mate 2
    has err 2.  6: mate 1 has err 1.  7: a tandem repeat, inserts 40 and 64 both qualify: 64 wins.  8: insert 70 with two
    mismatches and an N.  9: a 5' quality cut beyond the insert empties the mate.  10: two empty mates."""
    rng = np.random.default_rng(SEED + 9)
    T = dna(rng, 4000)
    r1, r2, q1, q2 = [], [], [], []

    def add(a, b, qa=None, qb=None):
        r1.append(a)
        r2.append(b)
        q1.append(phred([35] * len(a)) if qa is None else qa)
        q2.append(phred([35] * len(b)) if qb is None else qb)

    add(*mates(T, 100, 20, 100, 100, rng))
    add(*mates(T, 300, 19, 100, 100, rng))
    add(*mates(T, 500, 100, 100, 100, rng))
    add(*mates(T, 700, 60, 100, 60, rng))
    add(*mates(T, 900, 45, 100, 60, rng))
    a, b = mates(T, 1100, 50, 100, 100, rng)
    add(a, b, qb=phred([35] * 99) + b" ")
    a, b = mates(T, 1300, 50, 100, 100, rng)
    add(a, b, qa=phred([35] * 99))
    unit = dna(rng, 24)
    frag = unit + unit + unit[:16]                        # 64 bytes of period 24: its prefix of 40 is also its own suffix
    add((frag + dna(rng, 100))[:100], (rc(frag) + dna(rng, 100))[:100])
    a, b = mates(T, 1500, 70, 100, 100, rng)
    a = bytearray(spoil(a, (10, 40)))
    a[55] = ord("N")
    add(bytes(a), b)
    a, b = mates(T, 1700, 30, 100, 100, rng)
    add(a, b, qa=phred([3] * 35 + [35] * 65))
    add(b"", b"", b"", b"")
    return _pairs("pairs", r1, r2, q1, q2, [], [dict(pair_min_overlap=20, pair_err_pct=10, min_qual_5p=20),
                                                 dict(pair_min_overlap=20, pair_err_pct=0), dict(pair_min_overlap=0)], T=T, frag=frag)


@functools.lru_cache(maxsize=None)
def pairs_with_adapters():
    """the pairs of `pairs` with both adapters known: a mate with an adapter hit switches step P off for its pair"""
    s = pairs()
    return _pairs("pairs_with_adapters", s.reads1, s.reads2, s.quals1, s.quals2, [ADAPTER, ADAPTER2],
                  [dict(pair_min_overlap=20, pair_err_pct=10, min_overlap=5), dict(pair_min_overlap=20, pair_err_pct=10, min_overlap=5, min_len=30)])


@functools.lru_cache(maxsize=None)
def pairs_no_qual():
    s = pairs()
    long1, long2 = mates(s.T, 2000, 260, 300, 280, np.random.default_rng(SEED + 10))
    return _pairs("pairs_no_qual", s.reads1 + [long1], s.reads2 + [long2], None, None, [], [dict(pair_min_overlap=25, pair_err_pct=5)])


def pair_sets():
    return [pairs(), pairs_with_adapters(), pairs_no_qual()]


# ---------------------------------------------------------------- planted inserts: what the definition recovers
PLANTED_N, PLANTED_READ, PLANTED_TEXT = 400, 100, 20_000
PLANTED_PARAMS = dict(min_qual_3p=0, min_overlap=3, adapter_err_pct=10, pair_min_overlap=20, pair_err_pct=10, min_len=20)


@functools.lru_cache(maxsize=None)
def planted():
    """400 pairs of 100-byte reads drawn from a text of 20,000 bytes, inserts 30..160 (more than half shorter than the reads),
    one base in a hundred misread.  -> T, reads1, reads2, quals1, quals2, insert, start (of the fragment in T)"""
    rng = np.random.default_rng(SEED + 11)
    T = dna(rng, PLANTED_TEXT)
    out = dict(T=T, reads1=[], reads2=[], quals1=[], quals2=[], insert=[], start=[])
    for _ in range(PLANTED_N):
        insert = int(rng.integers(30, 161))
        start = int(rng.integers(0, PLANTED_TEXT - insert))
        a, b = mates(T, start, insert, PLANTED_READ, PLANTED_READ, rng)
        a = spoil(a, np.nonzero(rng.random(PLANTED_READ) < 0.01)[0])
        b = spoil(b, np.nonzero(rng.random(PLANTED_READ) < 0.01)[0])
        out["reads1"].append(a)
        out["reads2"].append(b)
        out["quals1"].append(phred(int(q) for q in rng.integers(25, 41, PLANTED_READ)))
        out["quals2"].append(phred(int(q) for q in rng.integers(25, 41, PLANTED_READ)))
        out["insert"].append(insert)
        out["start"].append(start)
    return out


def fastq_image(reads, quals, prefix: str = "r") -> bytes:
    return b"".join(b"@%s%d x=1\n%s\n+\n%s\n" % (prefix.encode(), i, r, q) for i, (r, q) in enumerate(zip(reads, quals)))
