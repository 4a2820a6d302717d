"""NeedlemanWunsch inputs aimed at each of the nine kernels polyhip_nw_align_batch can run -- nw_reg_kernel<64>,
nw_wave_kernel<R> for R = 2, 3, 4, 8, 16, 32, 64 rows per lane, the generic nw_kernel -- at their edges and tie rules
(tests/test_nw_shapes_cpu.py asserts that each input has the property it is named for, tests/test_nw_shapes_gpu.py
compares the GPU with the oracle on them).  Builders only: fixed seeds, no GPU, every batch cached.

Also here: dp() / walk(), a numpy restatement of the recurrence and of the reference's traceback (align.go:100-166) in
64-bit integers, which names the kind of every cell the walk visits."""
from __future__ import annotations

import dataclasses
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrices.json")
DNA = b"ACGT"


# ---------------------------------------------------------------- which kernel runs (sw_traceback.hip nw_wave_r + the entry point)
def wave_r(max_a: int) -> int:
    """rows per lane of the one-wave-per-pair kernel for a longest A of max_a (0: another kernel)"""
    return 0 if max_a <= 64 or max_a > 4096 else -(-max_a // 64) if max_a <= 256 else 8 << sum(max_a > c for c in (512, 1024, 2048))


def path(max_a: int, generic: bool = False) -> int:
    """polyhip_nw_last_path(): 1 = nw_reg_kernel<64>, 3 = nw_wave_kernel<wave_r>, 2 = nw_kernel"""
    return 2 if generic or max_a > 4096 or max_a == 0 else 1 if max_a <= 64 else 3


def unit(max_a: int) -> int:
    """the rows that share one piece of a kernel's bookkeeping: a lane's rows in the wave kernel, the 32 rows of one
    G / L word in the register-tiled kernel, the 16 rows of one 2-bit word in the generic one"""
    return wave_r(max_a) or (32 if max_a <= 64 else 16)


# ---------------------------------------------------------------- scorings
@dataclasses.dataclass(frozen=True)
class Scoring:
    first: str
    second: str
    scores: tuple   # rows of the table, first x second
    gap: int

    def lut(self) -> np.ndarray:
        """256 x 256 int64; dp() is only given valid symbols"""
        t = np.zeros((256, 256), np.int64)
        for i, a in enumerate(self.first):
            for j, b in enumerate(self.second):
                t[ord(a), ord(b)] = self.scores[i][j]
        return t


# twelve different off-diagonal entries: a transposed lookup, or one with the two codes swapped, scores differently
ASYM = ((5, -1, -2, -3), (-4, 4, -5, -6), (-7, -8, 6, -9), (1, -10, 2, 3))


def asym(gap: int) -> Scoring:
    return Scoring("ACGT", "ACGT", ASYM, gap)


def simple(match: int, mismatch: int, gap: int) -> Scoring:
    return Scoring("ACGT", "ACGT", tuple(tuple(match if i == j else mismatch for j in range(4)) for i in range(4)), gap)


@functools.lru_cache(maxsize=None)
def blosum62(gap: int) -> Scoring:
    with open(GOLDEN) as f:
        t = json.load(f)["BLOSUM62"]
    return Scoring(t["alphabet"], t["alphabet"], tuple(tuple(r) for r in t["scores"]), gap)


def protein_letters() -> bytes:
    return blosum62(-4).first.replace("-", "").replace("*", "").encode()


# ---------------------------------------------------------------- sequences
def rand(rng, letters: bytes, n: int) -> bytes:
    return bytes(np.frombuffer(letters, np.uint8)[rng.integers(0, len(letters), n)].tolist())


def mutate(rng, seq: bytes, letters: bytes, sub=0.06, indel=0.04) -> bytes:
    """substitutions, deletions and insertions"""
    out = bytearray()
    for c in seq:
        r = rng.random()
        if r < indel / 2:
            continue
        if r < indel:
            out.append(letters[int(rng.integers(0, len(letters)))])
        out.append(letters[int(rng.integers(0, len(letters)))] if rng.random() < sub else c)
    return bytes(out)


def fit(rng, seq: bytes, letters: bytes, n: int, back: bool = False) -> bytes:
    """seq cut (at its end, or at its start when `back`) or extended with random letters to n symbols"""
    if len(seq) >= n:
        return seq[len(seq) - n:] if back else seq[:n]
    return seq + rand(rng, letters, n - len(seq))


@dataclasses.dataclass(frozen=True)
class Batch:
    A: tuple
    B: tuple
    note: dict = dataclasses.field(default_factory=dict, compare=False)

    @property
    def max_a(self):
        return max(len(a) for a in self.A)

    @property
    def max_b(self):
        return max(len(b) for b in self.B)

    @property
    def cells(self):
        return sum(len(a) * len(b) for a, b in zip(self.A, self.B))


# ---------------------------------------------------------------- 1. the ladder
LADDER = (64, 65, 128, 129, 192, 193, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097)
LADDER_R = dict(zip(LADDER, (0, 2, 2, 3, 3, 4, 4, 8, 8, 16, 16, 32, 32, 64, 64, 0)))
LADDER_GENERIC = (65, 2049)   # these also run with POLYHIP_NW_GENERIC=1
B_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 62, 63, 64, 65, 66, 127, 128, 129, 190)
MAX_CELLS = 5 * 10**7       # the oracle's cells per parametrised case


def ladder_a_lengths(max_a: int):
    u = unit(max_a)
    return sorted({n for n in (1, 2, u - 1, u, u + 1, 2 * u, 63 * u, 63 * u + 1, max_a) if 1 <= n <= max_a})


def ladder_scorings(max_a: int):
    s = [(asym(-2), False), (asym(0), False)]
    if max_a <= 256:
        s.append((asym(1), False))
    if max_a > 1024:
        s.append((blosum62(-4), True))
    return s


@functools.lru_cache(maxsize=None)
def ladder(max_a: int, protein: bool = False) -> Batch:
    """every A length of ladder_a_lengths() against a mutated copy of itself cut or extended to every length of
    B_LENGTHS; an empty A, an empty B; unrelated pairs.  The first pair holds the longest A."""
    rng = np.random.default_rng(2 * max_a + protein)
    letters = protein_letters() if protein else DNA
    A, B = [], []
    for ia, la in enumerate(reversed(ladder_a_lengths(max_a))):
        a = rand(rng, letters, la)
        for ib, lb in enumerate(B_LENGTHS):
            A.append(a)
            B.append(fit(rng, mutate(rng, a, letters), letters, lb, back=(ia + ib) % 2 == 1))
    A += [b"", rand(rng, letters, min(max_a, 65))]
    B += [rand(rng, letters, 64), b""]
    for la, lb in ((max_a, 190), (max_a, 129), (max_a, 63), (min(max_a, 2 * unit(max_a) + 1), 66), (1, 1), (2, 5)):
        A.append(rand(rng, letters, la))
        B.append(rand(rng, letters, lb))
    return Batch(tuple(A), tuple(B))


# ---------------------------------------------------------------- the recurrence and the reference's walk, in numpy
def dp(a: bytes, b: bytes, sc: Scoring):
    """H of align.go:112-134 as (len(a) + 1) x (len(b) + 1) int64 and the substitution scores len(a) x len(b), one
    anti-diagonal at a time"""
    m, n = len(a), len(b)
    H = np.zeros((m + 1, n + 1), np.int64)
    H[:, 0] = np.arange(m + 1, dtype=np.int64) * sc.gap
    H[0, :] = np.arange(n + 1, dtype=np.int64) * sc.gap
    sub = sc.lut()[np.frombuffer(a, np.uint8)[:, None], np.frombuffer(b, np.uint8)[None, :]]
    for k in range(2, m + n + 1):
        i = np.arange(max(1, k - n), min(m, k - 1) + 1)
        j = k - i
        H[i, j] = np.maximum(H[i - 1, j - 1] + sub[i - 1, j - 1], np.maximum(H[i - 1, j], H[i, j - 1]) + sc.gap)
    return H, sub


KINDS = ("diag", "diag_tie", "up", "up_tie", "left")


def walk(a: bytes, b: bytes, sc: Scoring):
    """(score, alignA, alignB, kinds): the reference's traceback (:141-160) on dp(), and how often the walk stood on a
    cell of each kind -- the diagonal strictly best, the diagonal tied with a gap move (the diagonal wins), and where a
    gap move is taken: up strictly over left, up tied with left (up wins), left"""
    H, sub = dp(a, b, sc)
    i, j = len(a), len(b)
    ra, rb = bytearray(), bytearray()
    kinds = dict.fromkeys(KINDS, 0)
    while i > 0 and j > 0:
        d, u, l = int(H[i - 1, j - 1] + sub[i - 1, j - 1]), int(H[i - 1, j]) + sc.gap, int(H[i, j - 1]) + sc.gap
        if d >= max(u, l):
            kinds["diag" if d > max(u, l) else "diag_tie"] += 1
            ra.append(a[i - 1]), rb.append(b[j - 1])
            i, j = i - 1, j - 1
        elif u >= l:
            kinds["up" if u > l else "up_tie"] += 1
            ra.append(a[i - 1]), rb.append(ord("-"))
            i -= 1
        else:
            kinds["left"] += 1
            ra.append(ord("-")), rb.append(b[j - 1])
            j -= 1
    return int(H[len(a), len(b)]), bytes(ra[::-1]), bytes(rb[::-1]), kinds


# ---------------------------------------------------------------- 2. ties
TIE_CLASSES = {"path1": (64, False), "R2": (128, False), "R8": (512, False), "R32": (2048, False), "generic": (128, True)}
TIE_TABLES = ((1, -1), (2, 0), (1, 0))
TIE_GAPS = (-1, 0, 1)
TIE_MIN = 20   # visited cells of each kind per class, over its nine scorings


@functools.lru_cache(maxsize=None)
def ties(cls: str) -> Batch:
    """homopolymers of unequal length, AC-repeats against CA-repeats, two-letter random strings, four-letter random
    strings with indels; the long ones reach the class's longest A, so that the tied cells lie in high lanes too"""
    M = TIE_CLASSES[cls][0]
    rng = np.random.default_rng(len(cls) * 1000 + M)
    A = [b"A" * M, b"A" * 40, b"A" * (M // 2), b"A" * 7]
    B = [b"A" * min(M - 9, 150), b"A" * 55, b"A" * 190, b"A" * 64]
    A += [(b"AC" * M)[:M], b"AC" * 20, b"CA" * 31 + b"C"]
    B += [b"CA" * 60, b"CA" * 33, b"AC" * 31]
    for la, lb in ((M, 120), (50, 80), (M - 1, 65), (33, 32)):
        A.append(rand(rng, b"AC", la))
        B.append(rand(rng, b"AC", lb))
    for la in (M, min(M, 180), 64, 61):
        a = rand(rng, DNA, la)
        b = mutate(rng, a[-150:], DNA, sub=0.1, indel=0.2)
        A.append(a)
        B.append(b[:190])
        A.append(mutate(rng, b, DNA, sub=0.05, indel=0.3)[:M])   # B carries insertions against this A: left moves
        B.append(b[:190])
    return Batch(tuple(A), tuple(B))


# ---------------------------------------------------------------- 3. error order
ERR_CLASSES = {"path1": (64, False), "R2": (128, False), "R16": (1000, False), "generic": (128, True)}


def _put(seq: bytes, *at) -> bytes:
    s = bytearray(seq)
    for idx, sym in at:
        s[idx] = ord(sym)
    return bytes(s)


@functools.lru_cache(maxsize=None)
def errors(cls: str):
    """(Batch, expected err per pair, what each pair is): the reference names the first failing Score() in row-major
    order -- a[0], then the first invalid b[j], then the first invalid a[i] (align.go:126-129, matrix.go:29-36) -- and
    never looks at a symbol whose partner is empty"""
    M = ERR_CLASSES[cls][0]
    rng = np.random.default_rng(7 * M + len(cls))
    a0, b0 = rand(rng, DNA, M), rand(rng, DNA, 150)
    A, B, want, what = [a0], [b0], [0], ["valid"]

    def add(a, b, side, sym, name):
        A.append(a), B.append(b), what.append(name)
        want.append((side << 8) | ord(sym) if side else 0)

    for idx, sym in zip((0, 1, 63, 64, 65, M - 1), "NXZnxz"):
        if idx < M:
            add(_put(a0, (idx, sym)), b0, 1, sym, f"A[{idx}]")
    short = rand(rng, DNA, min(M, 66))
    add(_put(short, (len(short) - 1, "J")), b0[:70], 1, "J", "A[last] of a short A")
    for idx, sym in zip((0, 63, 64, 149), "NXZn"):
        add(a0, _put(b0, (idx, sym)), 2, sym, f"B[{idx}]")
    add(a0[:40], _put(b0[:65], (64, "U")), 2, "U", "B[64] = B[last] of 65")
    hi = min(70, M - 1)
    add(_put(a0, (1, "X"), (hi, "Y")), _put(b0, (100, "Z")), 2, "Z", "both sides, a[0] valid: B named")
    add(_put(a0, (5, "X")), _put(b0, (149, "z")), 2, "z", "both sides, a[0] valid, B's at its end: B named")
    add(_put(a0, (0, "X")), _put(b0, (0, "Z")), 1, "X", "both sides, a[0] invalid: A named")
    add(_put(a0, (0, "Y"), (hi, "X")), _put(b0, (64, "Z")), 1, "Y", "both sides, a[0] invalid: A named")
    add(_put(a0, (M // 2, "X"), (M - 1, "Y")), b0, 1, "X", "two in A: the first")
    add(_put(a0, (M - 1, "X"), (M // 2, "Y")), b0, 1, "Y", "two in A: the first")
    add(a0, _put(b0, (3, "Y"), (70, "X")), 2, "Y", "two in B: the first")
    add(a0, _put(b0, (70, "X"), (130, "Y")), 2, "X", "two in B: the first")
    add(_put(a0, (0, "N"), (M - 1, "X")), b"", 0, "", "invalid A, empty B: no error")
    add(b"", _put(b0, (0, "N"), (64, "X")), 0, "", "empty A, invalid B: no error")
    return Batch(tuple(A), tuple(B)), tuple(want), tuple(what)


# ---------------------------------------------------------------- 4. the device entry point in three launches
DEV_CLASSES = {"path1": (60, 90, False), "R2": (100, 100, False), "R8": (300, 320, False), "generic": (100, 100, True)}
DEV_PAIRS = 600
DEV_CHUNK = 256   # pairs per launch with a workspace of DEV_CHUNK pairs


@functools.lru_cache(maxsize=None)
def dev_batch(cls: str) -> Batch:
    """600 ragged pairs (the first three A: empty, one symbol, the longest), B a copy of A with a few indels, cut to the
    class's longest B; every 97th pair carries an invalid symbol, every 101st an empty B"""
    max_a, max_b, _ = DEV_CLASSES[cls]
    rng = np.random.default_rng(max_a + max_b + len(cls))
    lens = rng.integers(0, max_a + 1, DEV_PAIRS)
    lens[:3] = (0, 1, max_a)
    A, B = [], []
    for p, n in enumerate(lens):
        a = rand(rng, DNA, int(n))
        b = bytearray(a)
        for _ in range(int(rng.integers(0, 6)) + len(a) // 40):
            if b and rng.random() < 0.5:
                del b[int(rng.integers(0, len(b)))]
            else:
                b.insert(int(rng.integers(0, len(b) + 1)), DNA[int(rng.integers(0, 4))])
        b = bytes(b[:max_b])
        if p % 97 == 50 and a:
            a = _put(a, (len(a) // 2, "N"))
        if p % 101 == 60:
            b = b""
        A.append(a)
        B.append(b)
    B[2] = fit(rng, B[2], DNA, max_b)   # the longest B next to the longest A
    return Batch(tuple(A), tuple(B))


# ---------------------------------------------------------------- 5. shared B
SHARED_CLASSES = {"path1": (64, False), "R2": (128, False), "R16": (1024, False), "generic": (128, True)}
SHARED_B_LENGTHS = (1, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def shared(cls: str):
    """(reads, shared Bs): reads cut from mutated copies of the longest B, unrelated reads, an empty one, one with an
    invalid first symbol; B of 1, 63, 64, 65 and 200 symbols, and the 200 with an invalid symbol at index 64"""
    M = SHARED_CLASSES[cls][0]
    rng = np.random.default_rng(3 * M + len(cls))
    b200 = rand(rng, DNA, 200)
    Bs = [b200[:n] for n in SHARED_B_LENGTHS] + [_put(b200, (64, "N"))]
    A = [fit(rng, mutate(rng, b200, DNA), DNA, M), rand(rng, DNA, M), b"", _put(rand(rng, DNA, 30), (0, "X")), b"A", b"CG"]
    for k in range(30):
        n = int(rng.integers(1, M + 1))
        src = mutate(rng, b200 * (M // 200 + 1), DNA, sub=0.1)
        s = int(rng.integers(0, 64))
        A.append(fit(rng, src[s:], DNA, n) if k % 3 else rand(rng, DNA, n))
    return tuple(A), tuple(Bs)


# ---------------------------------------------------------------- 6. the int32 guard
BIG = 1 << 24   # the largest |score| and |gap| polyhip_scoring_create takes
GUARD_CASES = {"path1": (64, 63, False), "R2": (65, 62, False), "generic": (65, 62, True)}   # max_lenA + lenB = 127
GUARD_REFUSED = ((64, 64), (65, 63))                                                     # ... = 128: BIG * 128 = 2^31


def big(gap: int) -> Scoring:
    return simple(BIG, -BIG, gap)


@functools.lru_cache(maxsize=None)
def guard_batch(max_a: int, max_b: int) -> Batch:
    """identical strings, strings without a common letter, random ones: H runs towards both ends of the int32 range"""
    rng = np.random.default_rng(max_a * 1000 + max_b)
    a = rand(rng, DNA, max_a)
    A = [a, a, b"A" * max_a, b"AC" * (max_a // 2) + b"A" * (max_a % 2), rand(rng, DNA, max_a), a[:max_a // 2], a[:1], b"G" * max_a]
    B = [a[:max_b], a[-max_b:], b"C" * max_b, (b"GT" * max_b)[:max_b], rand(rng, DNA, max_b), a[:max_b], b"T" * max_b, b"G" * max_b]
    return Batch(tuple(A), tuple(B))
