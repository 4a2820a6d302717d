"""The named inputs of the primer-dimer tests (tests/test_dimers_cpu.py says what each holds, tests/test_dimers_gpu.py runs them
on the device).  Everything is seeded: the same bytes in every run.

The sets that exist for the index arithmetic (``sized``, ``wide``) use short primers: what they can break -- a lane past the end
of Y, a wave or a block boundary, a chunk boundary, the lowest index among equals across chunks -- does not depend on the
primers' length, the plain-Python oracle's time does, and short primers tie far more often, which is what the index rules are
about.  The sets that exist for the masks (``hand``, ``grid_pairs``, ``random_pool``) use the lengths the masks care about."""
from __future__ import annotations

import numpy as np

import dimers_oracle as do

ACGT = b"ACGT"
GRID = (1, 2, 3, 31, 32, 33, 63, 64)
SIZED_NX, SIZED_NY = (1, 2, 65), (1, 63, 64, 65, 127, 128, 129, 1000)
WIDE_NY = 70_000


def _dna(rng, n) -> bytes:
    return bytes(ACGT[c] for c in rng.integers(0, 4, n))


def _pool(rng, count, lo, hi):
    return [_dna(rng, int(rng.integers(lo, hi + 1))) for _ in range(count)]


# ---------------------------------------------------------------- answers written out by hand, table at 310150 mK
def hand():
    """(x, y, (dg_any, shift, pos, pairs), (dg_end, shift, pairs)); the sums are re-derived in tests/test_dimers_cpu.py"""
    long64 = _dna(np.random.default_rng(64), 64)
    t = do.stack_table()
    whole = sum(t[4 * do.code(a) + do.code(b)] for a, b in zip(long64, long64[1:]))
    return [
        (b"ACGTTGCA", b"TGCAACGT", (-11216, 7, 0, 8), (-11216, 7, 8)),           # its own reverse complement
        (b"AAAAAAAAAA", b"TTTTTTTTTT", (-8946, 9, 0, 10), (-8946, 9, 10)),
        (b"GGGCCC", b"GGGCCC", (-9544, 5, 0, 6), (-9544, 5, 6)),
        (b"acgtNACGT", b"ACGTNACGT", (-5070, 3, 0, 4), (-5070, 8, 4)),            # the same run at s = -5, 0 and 5: the smallest s
        (b"ACGTNACGT", b"ACGTNACGT", (-5070, 3, 0, 4), (-5070, 8, 4)),
        (long64, do.revcomp(long64), (whole, 63, 0, 64), (whole, 63, 64)),
        (b"AAAAAA", b"AAAAAA", (0, 0, 0, 0), (0, 0, 0)),                          # nothing pairs
        (b"ACACAC", b"GAGAGA", (0, 0, 0, 0), (0, 0, 0)),                          # single pairs only: no stack, no run
        (b"GGGGAAAA", b"CCCC", (-5484, 3, 0, 4), (0, 0, 0)),                      # x's 3' end stays single
        (b"AAAAGGGG", b"CCCC", (-5484, 7, 4, 4), (-5484, 7, 4)),
    ]


# ---------------------------------------------------------------- every mask edge: lengths around 32 and 64, shifts to +-63
def grid_pairs(m: int, n: int):
    """three pairs (x of m bytes, y of n bytes), y carrying the reverse complement of a piece of x: the whole overlap min(m, n)
    from both starts; x's last two bases against y's last two (the largest shift with a stack, m - 2); x's first two against y's
    first two (the smallest, 2 - n).  Pieces of two need m, n >= 2; with less the pair simply has no run."""
    rng = np.random.default_rng(1000 * m + n)
    out = []
    L = min(m, n)
    x, y = _dna(rng, m), bytearray(_dna(rng, n))
    y[:L] = do.revcomp(x[:L])
    out.append((x, bytes(y)))
    if L >= 2:
        x, y = _dna(rng, m), bytearray(_dna(rng, n))
        y[n - 2:] = do.revcomp(x[m - 2:])
        out.append((x, bytes(y)))
        x, y = _dna(rng, m), bytearray(_dna(rng, n))
        y[:2] = do.revcomp(x[:2])
        out.append((x, bytes(y)))
    return out


# ---------------------------------------------------------------- sizes of X and Y around the wave, the block and the chunk
def sized_pool():
    """65 x and 1000 y of 6..14 bytes; ``sized`` cuts prefixes of them, so one oracle plane serves every size"""
    rng = np.random.default_rng(77)
    return _pool(rng, max(SIZED_NX), 6, 14), _pool(rng, max(SIZED_NY), 6, 14)


def wide():
    """3 x of 18..30 bytes against 70,000 y of 4..6 bytes: more y than a chunk, a launch's worth of blocks per row, and so many
    equal energies that the lowest index has to win across chunks.  (At most 5,376 different y: the oracle works each out once.)"""
    rng = np.random.default_rng(70)
    X = _pool(rng, 3, 18, 30)
    lens = rng.integers(4, 7, WIDE_NY)
    codes = rng.integers(0, 4, (WIDE_NY, 6))
    return X, [bytes(ACGT[c] for c in codes[j, :lens[j]]) for j in range(WIDE_NY)]


# ---------------------------------------------------------------- primers that are no primers, bytes that are no bases
def bad_lengths():
    """empty, 65-byte and 200-byte primers among valid ones (a 64-byte one too), on both sides.  errX = [0, 1, 0, 2, 2, 0], errY
    = [2, 0, 1, 0, 2]"""
    rng = np.random.default_rng(5)
    a, b, c = _dna(rng, 24), _dna(rng, 64), _dna(rng, 20)
    X = [a, b"", b, _dna(rng, 65), _dna(rng, 200), c]
    Y = [do.revcomp(a) + b"A" * 176, do.revcomp(a), b"", do.revcomp(b), do.revcomp(c) * 4]
    return X, Y


def odd_bytes():
    """lower case pairs like upper case; N, U, '-', 0x00, 0xff, '{' and '[' ('{' without its case bit), 0xc1 and 0xe1 ('A' and
    'a' with the top bit set) pair with nothing and end a run"""
    X = [b"acgtacgtacgt", b"ACGTNNNNACGT", b"ACGUACGUACGU", b"AC-GT\x00ACGT\xff", b"aCgTaCgTaCgT", b"ACGT[ACGT{ACGT!"]
    Y = [b"ACGTACGTACGT", b"acgtacgtacgt", b"NNNNNNNNNNNN", b"ACGTnnnnACGT", b"UUUUAAAAUUUU", b"ACGT\xc1\xe1ACGT"]
    return X, Y


def duplicates():
    """row 0's best partner, its whole reverse complement, stands at 1, 3 and 4 of Y: 1 wins.  Row 1's best stands at 2 and 5."""
    rng = np.random.default_rng(9)
    x0, x1 = _dna(rng, 22), _dna(rng, 19)
    Y = [_dna(rng, 20), do.revcomp(x0), do.revcomp(x1), do.revcomp(x0), do.revcomp(x0), do.revcomp(x1), _dna(rng, 25)]
    return [x0, x1], Y


def no_partner():
    """row 0 (all A) meets no T; row 1 meets single pairs only; row 2 has a partner, so the set is not trivially empty"""
    X = [b"AAAAAAAAAAAAAAAAAA", b"ACACACACACAC", b"GGGGTTTT"]
    Y = [b"AAAAAAAACCCC", b"GAGAGAGAGAGA", b"CACACAGGGAAA"]
    return X, Y


def random_pool(count: int = 100):
    """count primers of 18..30 bytes: count^2 ordered pairs in pool mode"""
    return _pool(np.random.default_rng(1830), count, 18, 30)


# ---------------------------------------------------------------- a pool with exactly one 3' dimer
END_A, END_B = 2, 5
END_THRESHOLD = -5000


def end_dimer_pool():
    """8 primers of 20 bytes.  The last six bases of primer 2, CGGACC, are the reverse complement of the last six of primer 5,
    GGTCCG.  For every other ordered pair (x, y), the pair of a primer with itself included, the reverse complement of x's last
    four bases occurs nowhere in y: no shift pairs x's 3' end over four bases, and three pairs are two stacks, at least 2 * -2232
    = -4464 cal/mol, which is above the threshold.  Drawn until that holds."""
    rng = np.random.default_rng(8)
    while True:
        pool = _pool(rng, 8, 20, 20)
        pool[END_A] = pool[END_A][:14] + b"CGGACC"
        pool[END_B] = pool[END_B][:14] + b"GGTCCG"
        if all(do.revcomp(x[-4:]) not in y for i, x in enumerate(pool) for j, y in enumerate(pool)
               if (i, j) not in ((END_A, END_B), (END_B, END_A))):
            return pool
