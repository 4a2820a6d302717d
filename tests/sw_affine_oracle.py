"""Smith-Waterman with affine gaps in plain Python, with the full matrices: the definition above polyhip_sw_affine_batch
in include/polyhip.h, restated.  Also builds the named inputs that tests/test_sw_affine_cpu.py (no GPU: the inputs really
hold what they are meant to exercise) and tests/test_sw_affine_gpu.py (the kernels equal this oracle) share.

    E[i][j] = max(H[i][j-1] + go, E[i][j-1] + ge)      gap in A (alignA gets '-')
    F[i][j] = max(H[i-1][j] + go, F[i-1][j] + ge)      gap in B (alignB gets '-')
    H[i][j] = max(0, H[i-1][j-1] + S(a_i, b_j), F[i][j], E[i][j])
"""
import functools
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -(1 << 60)

Result = namedtuple("Result", "score endA endB err alignA alignB")


class Mat:
    """A substitution matrix over single-byte symbols: first / second alphabet (str), scores[len(first)][len(second)]."""

    def __init__(self, first, second, scores):
        self.first, self.second = first, second
        self.scores = [[int(v) for v in row] for row in scores]
        assert len(self.scores) == len(first) and all(len(r) == len(second) for r in self.scores)
        self.validA = [False] * 256
        self.validB = [False] * 256
        self.lut = [[0] * 256 for _ in range(256)]
        for x, ca in enumerate(first):
            self.validA[ord(ca)] = True
            for y, cb in enumerate(second):
                self.validB[ord(cb)] = True
                self.lut[ord(ca)][ord(cb)] = self.scores[x][y]
        self.smax = max(max(r) for r in self.scores)
        self.smin = min(min(r) for r in self.scores)

    def reference(self):
        """the same matrix for the linear oracle (oracle.smith_waterman)"""
        import oracle
        return oracle.SubstitutionMatrix(self.first, self.second, self.scores)

    def scoring(self, gap=-1):
        """the same matrix as a poly_amd scoring handle (its own gap is ignored by the affine calls)"""
        from poly_amd import align, alphabet, matrix
        return align.NewScoring(matrix.NewSubstitutionMatrix(alphabet.NewAlphabet(list(self.first)),
                                                             alphabet.NewAlphabet(list(self.second)), self.scores), gap)


def simple(symbols, match, mismatch):
    return Mat(symbols, symbols, [[match if x == y else mismatch for y in range(len(symbols))] for x in range(len(symbols))])


def _bytes(x):
    return x.encode("latin-1") if isinstance(x, str) else bytes(x)


def matrices(a, b, mat, go, ge):
    """the full H, E, F ((m + 1) x (n + 1) lists)"""
    m, n = len(a), len(b)
    H = [[0] * (n + 1) for _ in range(m + 1)]
    E = [[NEG] * (n + 1) for _ in range(m + 1)]
    F = [[NEG] * (n + 1) for _ in range(m + 1)]
    for i in range(1, m + 1):
        row = mat.lut[a[i - 1]]
        Hi, Hp, Ei, Fi, Fp = H[i], H[i - 1], E[i], F[i], F[i - 1]
        hl, el = 0, NEG
        for j in range(1, n + 1):
            e = hl + go
            if el + ge > e:
                e = el + ge
            f = Hp[j] + go
            if Fp[j] + ge > f:
                f = Fp[j] + ge
            h = Hp[j - 1] + row[b[j - 1]]
            if f > h:
                h = f
            if e > h:
                h = e
            if h < 0:
                h = 0
            Hi[j], Ei[j], Fi[j] = h, e, f
            hl, el = h, e
    return H, E, F


def error_of(a, b, mat):
    """err as polyhip_sw_batch: a[0], then the first invalid b[j], then the first invalid a[i]; 0 when a side is empty"""
    if not a or not b:
        return 0
    if not mat.validA[a[0]]:
        return (1 << 8) | a[0]
    for x in b:
        if not mat.validB[x]:
            return (2 << 8) | x
    for x in a[1:]:
        if not mat.validA[x]:
            return (1 << 8) | x
    return 0


def detail(a, b, mat, go, ge):
    """(Result, H, E, F, walk): walk = [(state, i, j)] of every cell the traceback visits, state in 'HFE'"""
    a, b = _bytes(a), _bytes(b)
    assert go <= ge <= -1
    err = error_of(a, b, mat)
    if err or not a or not b:
        return Result(0, 0, 0, err, b"", b""), None, None, None, []
    H, E, F = matrices(a, b, mat, go, ge)
    best, bi, bj = 0, 0, 0
    for i in range(1, len(a) + 1):
        Hi = H[i]
        rowmax = max(Hi)
        if rowmax > best:                      # strict: the first maximum in row-major order
            best, bi, bj = rowmax, i, Hi.index(rowmax)
    if best == 0:
        return Result(0, 0, 0, 0, b"", b""), H, E, F, []
    i, j, state = bi, bj, "H"
    outA, outB, walk = bytearray(), bytearray(), []
    while True:
        walk.append((state, i, j))
        if state == "H":
            h = H[i][j]
            if h == 0:
                break
            if h == H[i - 1][j - 1] + mat.lut[a[i - 1]][b[j - 1]]:
                outA.append(a[i - 1])
                outB.append(b[j - 1])
                i, j = i - 1, j - 1
            elif h == F[i][j]:
                state = "F"
            else:
                assert h == E[i][j]
                state = "E"
        elif state == "F":
            outA.append(a[i - 1])
            outB.append(ord("-"))
            if F[i][j] == H[i - 1][j] + go:    # open is preferred over extend
                state = "H"
            i -= 1
        else:
            outA.append(ord("-"))
            outB.append(b[j - 1])
            if E[i][j] == H[i][j - 1] + go:
                state = "H"
            j -= 1
    return Result(best, bi, bj, 0, bytes(outA[::-1]), bytes(outB[::-1])), H, E, F, walk


def align(a, b, mat, go, ge):
    """(score, endA, endB, err, alignA, alignB)"""
    return detail(a, b, mat, go, ge)[0]


def rescore(alignA, alignB, mat, go, ge):
    """the score of an alignment under the gap model: a run of k gap symbols on one side costs go + (k - 1) * ge"""
    assert len(alignA) == len(alignB)
    total, prev = 0, None
    for x, y in zip(alignA, alignB):
        assert not (x == 45 and y == 45)
        kind = "A" if x == 45 else "B" if y == 45 else None
        if kind is None:
            total += mat.lut[x][y]
        else:
            total += ge if kind == prev else go
        prev = kind
    return total


def window(res, mat, ge):
    """(W_p, columns of the traceback window, bound on the strings' bytes) of a pair with score >= 1"""
    W = res.endA + (mat.smax * res.endA - res.score) // -ge
    return W, min(res.endB, W), res.endA + min(res.endB, W - res.endA)


def rows_per_band():
    """RB of the kernels as the source states it (the GPU tests read it from sw_affine_last_info)"""
    src = open(os.path.join(ROOT, "poly_amd", "csrc", "sw_affine.hip")).read()
    return int(re.search(r"constexpr int RB = (\d+);", src).group(1))


# ------------------------------------------------------------------------------------------------- matrices of the cases
AB = simple("AB", 2, -1)            # two letters: ties everywhere
ACGT = simple("ACGT", 2, -1)
NUC5 = simple("ACGT", 5, -4)        # smax = 5: wide windows with ge = -1
S127 = simple("ACGT", 127, -127)
NUC_4 = Mat("-ACGT", "-ACGT", [[0, 0, 0, 0, 0], [0, 5, -4, -4, -4], [0, -4, 5, -4, -4], [0, -4, -4, 5, -4], [0, -4, -4, -4, 5]])


@functools.lru_cache(maxsize=None)
def big_matrix():
    """126 x 126 symbols (bytes 1..126): the compact table, 127 x 127 x 4 bytes, does not fit the 60 KB of LDS"""
    rng = np.random.default_rng(126)
    sym = "".join(chr(c) for c in range(1, 127))
    sc = rng.integers(-4, 3, (126, 126))
    sc[np.arange(126), np.arange(126)] = rng.integers(3, 7, 126)
    return Mat(sym, sym, sc.tolist())


@functools.lru_cache(maxsize=None)
def asym_matrix():
    """two alphabets, asymmetric scores"""
    rng = np.random.default_rng(77)
    return Mat("ACGT", "acgtn", rng.integers(-5, 6, (4, 5)).tolist())


Case = namedtuple("Case", "name mat go ge A B shared")   # A: list of bytes; B: list of bytes, or one bytes when shared


def _rand(rng, symbols, n):
    s = symbols.encode("latin-1")
    return bytes(s[int(x)] for x in rng.integers(0, len(s), n))


@functools.lru_cache(maxsize=None)
def expect(case):
    """the oracle's results of a case, computed once"""
    return tuple(align(a, case.B if case.shared else case.B[p], case.mat, case.go, case.ge) for p, a in enumerate(case.A))


KNOWN = (
    # A, B, match, mismatch, go, ge, score, alignA, alignB, endA, endB
    ("AAAAAAAATTTTTTTTCCCCCCCC", "AAAAAAAACCCCCCCC", 2, -3, -5, -1, 20, "AAAAAAAATTTTTTTTCCCCCCCC", "AAAAAAAA--------CCCCCCCC", 24, 16),
    ("GGTTGACTA", "TGTTACGG", 3, -3, -4, -1, 11, "GTTGAC", "GTT-AC", 7, 6),
    ("ACACACTA", "AGCACACA", 2, -1, -3, -1, 10, "ACACA", "ACACA", 5, 8),
)


@functools.lru_cache(maxsize=None)
def band_cases(rb):
    """A lengths around the band edges x B lengths around the wave's 64 columns, two alphabets, per-pair and shared B"""
    out = []
    lensA, lensB = (rb - 1, rb, rb + 1, 2 * rb, 2 * rb + 1, 1), (1, 2, 63, 64, 65)
    for mat, name in ((AB, "AB"), (ACGT, "ACGT")):
        rng = np.random.default_rng(len(name) * 1000 + rb)
        A, B = [], []
        for la in lensA:
            for lb in lensB:
                A.append(_rand(rng, mat.first, la))
                B.append(_rand(rng, mat.first, lb))
        out.append(Case(f"band-{name}-pairs", mat, -3, -1, tuple(A), tuple(B), False))
        for lb in lensB:
            out.append(Case(f"band-{name}-shared{lb}", mat, -3, -1, tuple(_rand(rng, mat.first, la) for la in lensA),
                            _rand(rng, mat.first, lb), True))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mixed_case(rb, n=300):
    """A lengths 0..3 rb shuffled, B of 20..70 per pair, some empty sides, invalid symbols at each place the err order
    distinguishes (a[0]; b[j] with a later a[i] invalid too; a[i] alone)"""
    rng = np.random.default_rng(4242 + rb)
    lens = np.arange(n) % (3 * rb + 1)
    rng.shuffle(lens)
    A, B = [], []
    for p in range(n):
        a = bytearray(_rand(rng, "ACGT", int(lens[p])))
        b = bytearray(_rand(rng, "ACGT", int(rng.integers(20, 71))))
        kind = p % 25
        if kind == 3:
            b = bytearray()
        elif kind == 7:
            a = bytearray()
        elif kind == 11 and len(a) >= 3:
            a[0] = ord("x")
            b[4] = ord("y")
        elif kind == 13 and len(a) >= 3:
            b[int(rng.integers(0, len(b)))] = ord("y")
            a[len(a) - 1] = ord("x")
        elif kind == 17 and len(a) >= 3:
            a[int(rng.integers(1, len(a)))] = ord("z")
        A.append(bytes(a))
        B.append(bytes(b))
    return Case(f"mixed-{rb}", ACGT, -4, -1, tuple(A), tuple(B), False)


def prefix(case, n):
    return Case(f"{case.name}[:{n}]", case.mat, case.go, case.ge, case.A[:n], case.B if case.shared else case.B[:n], case.shared)


@functools.lru_cache(maxsize=None)
def tie_case():
    """short pairs over two letters with go == 2 * ge: every tie rule occurs (tie_conditions says where)"""
    rng = np.random.default_rng(99)
    A, B = [], []
    for t in range(256):                                 # a run of 1..3 letters inserted on one side: gaps on the path
        base = _rand(rng, "AB", int(rng.integers(8, 20)))
        pos = int(rng.integers(2, len(base) - 2))
        long = base[:pos] + _rand(rng, "AB", int(rng.integers(1, 4))) + base[pos:]
        A.append(long if t % 2 else base)
        B.append(base if t % 2 else long)
    for _ in range(128):                                 # unrelated short pairs: the maximum occurs more than once
        A.append(_rand(rng, "AB", int(rng.integers(4, 15))))
        B.append(_rand(rng, "AB", int(rng.integers(4, 15))))
    return Case("ties", AB, -2, -1, tuple(A), tuple(B), False)


def tie_conditions(a, b, mat, go, ge):
    """which tie rules the traceback of this pair meets: a set of 'max-twice', 'diag-and-F', 'F-and-E', 'open-and-extend'"""
    res, H, E, F, walk = detail(a, b, mat, go, ge)
    found = set()
    if res.score == 0:
        return found
    if sum(row.count(res.score) for row in H) >= 2:
        found.add("max-twice")
    for state, i, j in walk:
        if state == "H" and H[i][j] > 0:
            d = H[i - 1][j - 1] + mat.lut[a[i - 1]][b[j - 1]]
            if H[i][j] == d and H[i][j] == F[i][j]:
                found.add("diag-and-F")
            if H[i][j] != d and H[i][j] == F[i][j] and H[i][j] == E[i][j]:
                found.add("F-and-E")
        if state == "F" and F[i][j] == H[i - 1][j] + go and F[i][j] == F[i - 1][j] + ge:
            found.add("open-and-extend")
        if state == "E" and E[i][j] == H[i][j - 1] + go and E[i][j] == E[i][j - 1] + ge:
            found.add("open-and-extend")
    return found


@functools.lru_cache(maxsize=None)
def gap_cases():
    """inserts of 1..40 bases on either side (wide windows: ge = -1, smax = 5; narrow ones: ge = -4), pairs whose path
    starts at column 1 so that endB clips the window, and identical pairs, which meet W_p exactly"""
    out = []
    for name, go, ge in (("wide", -6, -1), ("narrow", -8, -4)):
        rng = np.random.default_rng(len(name))
        A, B = [], []
        for k in range(1, 41):
            base = _rand(rng, "ACGT", 60)
            ins = _rand(rng, "ACGT", k)
            long = base[:30] + ins + base[30:]
            if k % 2:
                A.append(long)
                B.append(base)
            else:
                A.append(base)
                B.append(long)
        for k in range(6):                               # the path starts at column 1: B is the end of A
            b = _rand(rng, "ACGT", 30 + 5 * k)
            A.append(_rand(rng, "ACGT", 20 + 7 * k) + b)
            B.append(b + _rand(rng, "ACGT", 3 * k))
        for k in range(4):                               # identical: the path spans exactly W_p columns
            s = _rand(rng, "ACGT", 17 + 16 * k)
            A.append(s)
            B.append(s)
        out.append(Case(f"gaps-{name}", NUC5, go, ge, tuple(A), tuple(B), False))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def parity_batch(shared=True, n=300, read_len=150, ref_len=2000):
    """reads of 150 bp with 5 % substitutions and 1 % indels against a 2 kb reference (or each against its own piece)"""
    rng = np.random.default_rng(2024)
    ref = _rand(rng, "ACGT", ref_len)
    reads, pieces = [], []
    for _ in range(n):
        s = int(rng.integers(0, ref_len - read_len))
        q = bytearray()
        for x in ref[s:s + read_len]:
            u = rng.random()
            if u < 0.005:
                continue                                   # deletion
            if u < 0.010:
                q.append(b"ACGT"[int(rng.integers(0, 4))])  # insertion
            q.append(b"ACGT"[int(rng.integers(0, 4))] if rng.random() < 0.05 else x)
        reads.append(bytes(q))
        lo = max(0, s - int(rng.integers(0, 40)))
        pieces.append(ref[lo:s + read_len + int(rng.integers(0, 40))])
    return Case("parity-shared" if shared else "parity-pairs", NUC_4, -2, -2, tuple(reads), ref if shared else tuple(pieces), shared)


@functools.lru_cache(maxsize=None)
def table_cases():
    """a table too large for LDS, and two alphabets with an asymmetric table"""
    rng = np.random.default_rng(5)
    big = big_matrix()
    A = [_rand(rng, big.first[:12], int(rng.integers(1, 80))) for _ in range(70)]   # few letters: alignments exist
    B = [_rand(rng, big.first[:12], int(rng.integers(1, 80))) for _ in range(70)]
    A[5] = A[5] + bytes([127])                                                        # not in the alphabet
    asym = asym_matrix()
    A2 = [_rand(rng, "ACGT", int(rng.integers(1, 70))) for _ in range(70)]
    B2 = [_rand(rng, "acgtn", int(rng.integers(1, 70))) for _ in range(70)]
    return (Case("table-global-pairs", big, -5, -2, tuple(A), tuple(B), False),
            Case("table-global-shared", big, -5, -2, tuple(A[:20]), B[0] + B[1], True),
            Case("table-asym", asym, -6, -2, tuple(A2), tuple(B2), False))


@functools.lru_cache(maxsize=None)
def range_case():
    """a score beyond 32767: identical sequences of 300 symbols at 127 a match"""
    rng = np.random.default_rng(8)
    s = _rand(rng, "ACGT", 300)
    return Case("range", S127, -127, -1, (s, s[:280] + s[285:]), (s, s), False)


def gpu_cases(rb):
    """every case the GPU file compares with the oracle"""
    return band_cases(rb) + (mixed_case(rb), tie_case()) + gap_cases() + table_cases() + (range_case(),)
