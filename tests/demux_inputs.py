"""Hand-built inputs of the demultiplexer's tests: the smallest shapes at which its kernels can go wrong.  A set holds reads (and
qualities), its barcodes and the modes (keyword arguments of the oracle's calls) it is run under; `lead` bytes of filler go in
front of the packed batch, so that off[0] != 0.  Everything is drawn from fixed seeds."""
import random
from types import SimpleNamespace

import numpy as np

NONE = 0xFFFFFFFF


def dna(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def hamming(a, b):
    return sum(x != y for x, y in zip(a, b))


def spoil(s, places):
    """s with the bytes at `places` changed to another base"""
    out = bytearray(s)
    for k in places:
        out[k] = b"CGTA"[b"ACGT".index(out[k])]
    return bytes(out)


def barcode_set(rng, n, length, min_dist=1):
    """n barcodes of `length` bytes, pairwise at Hamming distance >= min_dist"""
    out = []
    while len(out) < n:
        c = dna(rng, length)
        if all(hamming(c, x) >= min_dist for x in out):
            out.append(c)
    return out


def quals_for(rng, reads):
    return [bytes(rng.randrange(35, 74) for _ in r) for r in reads]


def pack(strings, lead=0):
    """(bytes, offsets) as the calls take them, the first string `lead` bytes in"""
    off = np.zeros(len(strings) + 1, np.uint64)
    off[0] = lead
    off[1:] = lead + np.cumsum([len(s) for s in strings], dtype=np.uint64) if strings else lead
    return np.frombuffer(b"#" * lead + b"".join(strings) + b"\0", np.uint8)[:-1].copy(), off


def _single(name, reads, barcodes, modes, seed=1, quals=True, lead=0, **extra):
    rng = random.Random(seed)
    return SimpleNamespace(name=name, reads=reads, quals=quals_for(rng, reads) if quals else None, barcodes=barcodes, modes=modes,
                           lead=lead, **extra)


def lengths():
    """reads of 0 bytes, shorter than the barcode, exactly p, p + 1 .. p + max_shift; the barcode at every start that fits"""
    rng = random.Random(11)
    bc = barcode_set(rng, 3, 8, 3)
    reads = [b"", bc[0][:3], bc[1][:7], bc[0], bc[2], dna(rng, 1) + bc[1], dna(rng, 2) + bc[1], b"TT" + bc[0] + b"G",
             b"TTT" + bc[2], b"GGG" + bc[0], bc[1] + b"ACG", b"GGGG" + bc[0] + dna(rng, 20)]
    return _single("lengths", reads, bc, [dict(max_shift=3), dict(max_shift=0), dict(max_shift=3, clip=0), dict(max_shift=63)])


def long_at_63():
    """a 64-byte barcode at start 63: byte 126 is the last one touched; one byte short of it; a tail behind it"""
    rng = random.Random(12)
    bc = barcode_set(rng, 2, 64, 20)
    head = b"T" * 63
    reads = [head + bc[0], head + bc[1] + dna(rng, 30), head[:62] + bc[1], head + bc[0][:63], head + spoil(bc[0], (0, 63)),
             bc[1] + dna(rng, 70), head + spoil(bc[1], (5,)) + b"ACGT", b"T" * 64 + bc[0]]
    return _single("long_at_63", reads, bc, [dict(max_shift=63, max_mismatches=2), dict(max_shift=63, max_mismatches=0),
                                              dict(max_shift=63, max_mismatches=64, min_margin=0), dict(max_shift=62, max_mismatches=2)])


def four_byte():
    bc = [b"ACGT", b"TGCA", b"GGTT", b"CCAA"]
    rng = random.Random(13)
    reads = [b + dna(rng, 12) for b in bc] + [b"A" + bc[1] + b"GG", b"ACG", b"ACGT", b"ACGA" + dna(rng, 5), b"TTTTTTTT"]
    return _single("four_byte", reads, bc, [dict(max_shift=1, max_mismatches=0), dict(max_shift=0, max_mismatches=1),
                                            dict(max_shift=1, max_mismatches=1, min_margin=2)])


MIXED = (4, 6, 8, 12, 33, 64)


def mixed_lengths():
    """barcodes of 4 .. 64 bytes in one set, each at starts 0, 1 and 2, whole and one byte short"""
    rng = random.Random(14)
    bc = [dna(rng, p) for p in MIXED]
    reads = []
    for b in bc:
        for s in range(3):
            reads += [dna(rng, s) + b + dna(rng, 9), dna(rng, s) + b, dna(rng, s) + b[:-1]]
    return _single("mixed_lengths", reads, bc, [dict(max_shift=2, max_mismatches=0, min_margin=0), dict(max_shift=2, max_mismatches=3),
                                                dict(max_shift=0, max_mismatches=64, min_margin=0)])


def case_and_n():
    """lower case matches, N and n are mismatches"""
    bc = [b"ACGTACGT", b"TTGGCCAA", b"GATCGATC"]
    tail = b"GGATTACA"
    reads = [b"acgtacgt" + tail, b"AcGtAcGt" + tail, b"ACGNACGT" + tail, b"acgnacgt" + tail, b"NNNNNNNN" + tail, b"ttggccaN" + tail,
             b"GATCGATC" + tail.lower(), b"nACGTACGT" + tail, b"ACGTACG-" + tail, b"ACGTAC\x00\xff" + tail]
    return _single("case_and_n", reads, bc, [dict(max_mismatches=0), dict(max_mismatches=1), dict(max_shift=1, max_mismatches=2)])


def two_starts():
    """one barcode equally good at two starts (the smallest wins), and better at the later one"""
    bc = [b"ACACACAC", b"GGTTGGTT"]
    reads = [b"ACACACACACAC" + b"TTT", b"TCACACACACTT", b"ACACACTCACACAC", b"GTTGGTTGGTTGGTT", b"CACACACACACA"]
    return _single("two_starts", reads, bc, [dict(max_shift=4, max_mismatches=1), dict(max_shift=4, max_mismatches=1, min_margin=0),
                                             dict(max_shift=1, max_mismatches=2)])


def ties():
    """two barcodes at equal distance, and the runner-up exactly min_margin behind"""
    bc = [b"AAAACCCC", b"AAAACCGG", b"TTTTGGGG"]
    tail = b"GATTACAGATTACA"
    reads = [b"AAAACCCG" + tail,      # 1 and 1
             b"AAAACCGC" + tail,      # 1 and 1
             b"AAAACCCC" + tail,      # 0 and 2
             b"AAAACCGG" + tail,      # 2 and 0: the later barcode wins
             b"AAAACCTT" + tail,      # 2 and 2
             b"TAAACCCC" + tail,      # 1 and 3
             b"TTTTGGGG" + tail]      # 8, 8 and 0
    margins = [dict(max_mismatches=2, min_margin=g) for g in (0, 1, 2, 3)]
    swapped = SimpleNamespace(barcodes=[bc[1], bc[0], bc[2]])
    return _single("ties", reads, bc, margins + [dict(max_mismatches=0, min_margin=2)], swapped=swapped)


def single_barcode():
    """one barcode: d2 is none, so no margin makes a read ambiguous; every assigned read is in sample 0"""
    bc = [b"GATTACAG"]
    rng = random.Random(17)
    reads = [bc[0] + dna(rng, 10), spoil(bc[0], (2,)) + dna(rng, 10), spoil(bc[0], (2, 5)) + dna(rng, 10), dna(rng, 3), bc[0]]
    return _single("single_barcode", reads, bc, [dict(max_mismatches=1, min_margin=5), dict(max_mismatches=64, min_margin=64)])


COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 4096)


def count(nb):
    """nb barcodes: reads that carry the first, the last and some between, whole and with a substitution"""
    rng = random.Random(100 + nb)
    if nb == 4096:                                   # every 6-mer, shuffled
        bc = [bytes(b"ACGT"[x >> 2 * k & 3] for k in range(6)) for x in range(4096)]
        rng.shuffle(bc)
    else:
        bc = barcode_set(rng, nb, 8, 3 if nb <= 65 else 2)
    picks = sorted({0, nb - 1, nb // 2, min(63, nb - 1), min(64, nb - 1), nb // 3})
    reads = []
    for t in picks:
        reads += [bc[t] + dna(rng, 12), b"G" + bc[t] + dna(rng, 12), spoil(bc[t], (3,)) + dna(rng, 12)]
    reads.append(dna(rng, 24))
    modes = [dict(max_shift=0), dict(max_shift=1, min_margin=0), dict(max_shift=2, max_mismatches=0)]
    if nb <= 65:
        modes.append(dict(max_shift=63, max_mismatches=2))
    return _single(f"count_{nb}", reads, bc, modes, seed=nb)


def one_sample():
    """every read in sample 2 of 5"""
    rng = random.Random(18)
    bc = barcode_set(rng, 5, 8, 3)
    reads = [bc[2] + dna(rng, rng.randrange(0, 30)) for _ in range(70)]
    return _single("one_sample", reads, bc, [dict(), dict(clip=0)])


def all_unassigned():
    bc = [b"AAAAAAAA", b"CCCCCCCC", b"GGGGGGGG"]
    rng = random.Random(19)
    reads = [b"T" * rng.randrange(0, 40) for _ in range(70)] + [b"AAAACCCC" + b"T" * 9]
    return _single("all_unassigned", reads, bc, [dict(max_shift=2, max_mismatches=1)])


def empty_samples():
    """eight samples of which 0, 3, 4, 6 and 7 get nothing; the reads of the others interleaved"""
    rng = random.Random(20)
    bc = barcode_set(rng, 8, 8, 3)
    reads = [bc[(1, 5, 2, 5, 1, 2, 2)[i % 7]] + dna(rng, 15 + i % 4) for i in range(40)] + [dna(rng, 20)]
    return _single("empty_samples", reads, bc, [dict()])


def clip_edges():
    """clip_extra inside the read, exactly at its end and beyond it; clip = 0"""
    rng = random.Random(21)
    bc = barcode_set(rng, 4, 8, 3)
    reads = [bc[i % 4] + dna(rng, i) for i in range(12)] + [b"AC" + bc[1] + dna(rng, 5), dna(rng, 30)]
    return _single("clip_edges", reads, bc, [dict(max_shift=2, clip_extra=3), dict(max_shift=2, clip_extra=1000), dict(max_shift=2, clip=0),
                                             dict(max_shift=2, clip_extra=(1 << 24) - 1)], lead=5)


def no_qual():
    rng = random.Random(22)
    bc = barcode_set(rng, 6, 7, 3)
    reads = [dna(rng, i % 2) + bc[i % 6] + dna(rng, 20) for i in range(30)] + [dna(rng, 25), b""]
    return _single("no_qual", reads, bc, [dict(max_shift=1)], quals=False, lead=3)


def errs():
    """reads whose quality string has another length between good ones"""
    rng = random.Random(23)
    bc = barcode_set(rng, 3, 8, 3)
    reads = [bc[i % 3] + dna(rng, 12) for i in range(10)]
    s = _single("errs", reads, bc, [dict(), dict(clip=0)], lead=2)
    for i, q in ((1, b""), (3, s.quals[3][:-1]), (4, s.quals[4] + b"I"), (8, b"I" * 40)):
        s.quals[i] = q
    s.bad = [1, 3, 4, 8]
    return s


def random_many():
    """20,000 short reads: the grid stride of the wave-per-read kernels and several blocks of the sort"""
    rng = random.Random(24)
    bc = barcode_set(rng, 12, 6, 3)
    reads = []
    for i in range(20_000):
        x = rng.random()
        tail = dna(rng, rng.randrange(4, 16))
        t = rng.randrange(12)
        if x < 0.6:
            reads.append(bc[t] + tail)
        elif x < 0.75:
            reads.append(spoil(bc[t], (rng.randrange(6),)) + tail)
        elif x < 0.85:
            reads.append(dna(rng, 1) + bc[t] + tail)
        elif x < 0.9:
            reads.append(spoil(bc[t], (0, 4)) + tail)
        else:
            reads.append(tail)
    return _single("random_many", reads, bc, [dict(max_shift=1)], seed=25)


def single_sets():
    return [lengths(), long_at_63(), four_byte(), mixed_lengths(), case_and_n(), two_starts(), ties(), single_barcode(), one_sample(),
            all_unassigned(), empty_samples(), clip_edges(), no_qual(), errs()] + [count(nb) for nb in COUNTS]


# ---------------------------------------------------------------- pairs
def _pairs(name, reads1, reads2, barcodes1, barcodes2, pair_sample, nsamples, modes, seed=2, quals=True, lead=0, **extra):
    rng = random.Random(seed)
    return SimpleNamespace(name=name, reads1=reads1, reads2=reads2, quals1=quals_for(rng, reads1) if quals else None,
                           quals2=quals_for(rng, reads2) if quals else None, barcodes1=barcodes1, barcodes2=barcodes2,
                           pair_sample=pair_sample, nsamples=nsamples, modes=modes, lead=lead, **extra)


def pairs_one_set():
    """nbarcodes2 == 0: mate 1's barcode is the sample, mate 2 is not judged (it even starts with a barcode of the set)"""
    rng = random.Random(31)
    bc = barcode_set(rng, 5, 8, 3)
    reads1 = [bc[i % 5] + dna(rng, 20) for i in range(14)] + [dna(rng, 28), spoil(bc[0], (1,)) + dna(rng, 20)]
    reads2 = [bc[(i + 1) % 5] + dna(rng, 10 + i) for i in range(16)]
    return _pairs("pairs_one_set", reads1, reads2, bc, [], None, 5, [dict(), dict(clip=0), dict(max_mismatches=0, clip_extra=2)])


def pairs_holes():
    """a 3 x 4 table with holes; pairs of which one mate has no barcode, an ambiguous one, or a bad quality string"""
    rng = random.Random(32)
    bc1, bc2 = barcode_set(rng, 3, 8, 3), barcode_set(rng, 4, 6, 3)
    table = [0, 1, NONE, 2,
             NONE, 3, 4, 0,
             5, NONE, NONE, 6]
    reads1, reads2 = [], []
    for i in range(12):                                             # every cell once
        reads1.append(bc1[i // 4] + dna(rng, 18))
        reads2.append(bc2[i % 4] + dna(rng, 14))
    reads1 += [dna(rng, 26), bc1[0] + dna(rng, 18), spoil(bc1[1], (2, 6)) + dna(rng, 18), bc1[2] + dna(rng, 18), bc1[0] + dna(rng, 18)]
    reads2 += [bc2[1] + dna(rng, 14), dna(rng, 20), bc2[0] + dna(rng, 14), b"AC", bc2[1] + dna(rng, 14)]
    s = _pairs("pairs_holes", reads1, reads2, bc1, bc2, table, 7, [dict(), dict(clip=0), dict(max_shift=1, clip_extra=4)], lead=4)
    s.quals2[16] = s.quals2[16][:-2]                               # the last pair: mate 2 is bad, mate 1 fine
    return s


def pairs_no_qual():
    rng = random.Random(33)
    bc1, bc2 = barcode_set(rng, 2, 8, 3), barcode_set(rng, 2, 8, 3)
    reads1 = [bc1[i % 2] + dna(rng, 11) for i in range(9)]
    reads2 = [bc2[i // 2 % 2] + dna(rng, 13) for i in range(9)]
    return _pairs("pairs_no_qual", reads1, reads2, bc1, bc2, [1, 0, 0, NONE], 2, [dict()], quals=False)


TABLE_SAMPLES = (1, 256, 257, 65536)


def pairs_table(nsamples):
    """nsamples through a pair table: 1 (every cell the one sample), 256 and 257 (one and two passes of the sort's digits on
    either side), 65536 (every 4-mer on either mate: the table is the identity)"""
    rng = random.Random(200 + nsamples)
    if nsamples == 65536:
        bc1 = [bytes(b"ACGT"[x >> 2 * k & 3] for k in range(4)) for x in range(256)]
        bc2 = list(reversed(bc1))
        table = list(range(65536))
        modes = [dict(max_mismatches=0)]
    else:
        bc1, bc2 = barcode_set(rng, 16, 8, 3), barcode_set(rng, 17, 8, 3)
        table = [c % nsamples if c % 11 else NONE for c in range(16 * 17)]
        modes = [dict()]
    reads1, reads2 = [], []
    for i in range(300):
        reads1.append(bc1[rng.randrange(len(bc1))] + dna(rng, 8))
        reads2.append(bc2[rng.randrange(len(bc2))] + dna(rng, 8))
    reads1[0], reads2[0] = bc1[-1] + b"ACGTACGT", bc2[-1] + b"ACGTACGT"          # the last cell of the table
    return _pairs(f"pairs_table_{nsamples}", reads1, reads2, bc1, bc2, table, nsamples, modes, seed=nsamples)


def pair_sets():
    return [pairs_one_set(), pairs_holes(), pairs_no_qual()] + [pairs_table(k) for k in TABLE_SAMPLES]


# ---------------------------------------------------------------- the pooled constructs of the end-to-end test
POOL_READ, POOL_PER_SAMPLE, POOL_CONSTRUCT = 90, 240, 1000
POOL_PARAMS = dict(max_shift=0, max_mismatches=1, min_margin=1, clip=1, clip_extra=0)


def pooled():
    """Three constructs of about 1 kb, POOL_PER_SAMPLE reads each, every read an 8-byte barcode followed by POOL_READ bases of its
    construct (either strand, one base in a hundred misread).  The barcodes are pairwise at Hamming distance >= 3; one read in
    ten has one substitution in its barcode, one in twenty carries no barcode at all.  The reads are shuffled into one FASTQ
    image.  `truth[i]` is read i's construct, NONE for a read without a barcode; `subst[i]` its barcode substitutions."""
    rng = random.Random(41)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    constructs = [dna(rng, POOL_CONSTRUCT + 40 * k) for k in range(3)]
    bc = barcode_set(rng, 3, 8, 3)
    recs = []
    for k in range(3):
        for _ in range(POOL_PER_SAMPLE):
            at = rng.randrange(len(constructs[k]) - POOL_READ)
            body = constructs[k][at:at + POOL_READ]
            if rng.random() < 0.5:
                body = body.translate(comp)[::-1]
            body = spoil(body, [j for j in range(POOL_READ) if rng.random() < 0.01])
            x = rng.random()
            if x < 0.05:
                recs.append((NONE, 0, b"TTTTTTTT"[:rng.randrange(0, 8)] + body))
            elif x < 0.15:
                recs.append((k, 1, spoil(bc[k], (rng.randrange(8),)) + body))
            else:
                recs.append((k, 0, bc[k] + body))
    rng.shuffle(recs)
    fq, quals = bytearray(), []
    for i, (_, _, r) in enumerate(recs):
        quals.append(bytes(rng.randrange(53, 74) for _ in r))
        fq += b"@r%d\n%s\n+\n%s\n" % (i, r, quals[i])
    return dict(fastq=bytes(fq), reads=[r for _, _, r in recs], quals=quals, truth=[k for k, _, _ in recs],
                subst=[s for _, s, _ in recs], barcodes=bc, constructs=constructs)
