"""The oracle of the search with mismatches (polyhip_bwt_count_mismatch / _locate_mismatch), straight from the definition

    hits(P, k) = { (p, d) : 0 <= p <= n - m,  d = #{ j : S[p + j] != P[j] } <= k }

as a sliding compare in numpy -- no index, no suffix array -- and the inputs the CPU and the GPU tests share (the CPU test
asserts on the oracle what makes them non-vacuous, the GPU test runs them)."""
import functools
import itertools

import numpy as np

DNA = np.frombuffer(b"ACGT", np.uint8)


def _b(s) -> bytes:
    return s.encode("latin-1") if isinstance(s, str) else bytes(s)


def distances(seq, pat) -> np.ndarray:
    """d[p] = mismatches of pat against seq[p : p + m] for every p in [0, n - m]; empty for m == 0 or m > n"""
    S, P = np.frombuffer(_b(seq), np.uint8), np.frombuffer(_b(pat), np.uint8)
    n, m = len(S), len(P)
    if m == 0 or m > n:
        return np.zeros(0, np.int64)
    d = np.zeros(n - m + 1, np.int64)
    for j in range(m):
        d += S[j:n - m + 1 + j] != P[j]
    return d


def hits(seq, pat, k):
    """(positions uint32 ascending, mismatches uint8) of every hit with at most k mismatches"""
    d = distances(seq, pat)
    pos = np.flatnonzero(d <= k)
    return pos.astype(np.uint32), d[pos].astype(np.uint8)


class Case:
    """One text and its patterns; the distances are computed once, every k is read off them."""

    def __init__(self, seq, pats):
        self.seq, self.pats = seq, list(pats)

    @functools.cached_property
    def dist(self):
        return [distances(self.seq, p) for p in self.pats]

    @functools.lru_cache(maxsize=None)
    def expect(self, k):
        """(counts int64[npat, k + 1], first uint64[npat + 1], pos uint32[], mm uint8[])"""
        counts = np.zeros((len(self.pats), k + 1), np.int64)
        first = np.zeros(len(self.pats) + 1, np.uint64)
        pos, mm = [], []
        for i, d in enumerate(self.dist):
            at = np.flatnonzero(d <= k)
            counts[i] = np.bincount(d[at], minlength=k + 1)[:k + 1]
            first[i + 1] = first[i] + np.uint64(len(at))
            pos.append(at.astype(np.uint32))
            mm.append(d[at].astype(np.uint8))
        cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)
        return counts, first, cat(pos, np.uint32), cat(mm, np.uint8)


# ---------------------------------------------------------------- shared inputs
def dna(rng, n) -> bytes:
    return DNA[rng.integers(0, 4, n)].tobytes()


def mutate(rng, frag: bytes, subs: int, alphabet: bytes) -> bytes:
    """`subs` substitutions at distinct positions, each to another symbol of `alphabet`"""
    q = bytearray(frag)
    for j in rng.choice(len(q), size=subs, replace=False):
        q[j] = rng.choice([c for c in alphabet if c != q[j]])
    return bytes(q)


def cut(rng, seq: bytes, m: int, count: int, max_subs_plus_1: int, alphabet: bytes, pinned=()):
    """`count` m-mers cut from seq; pattern i gets i mod max_subs_plus_1 substitutions; the first len(pinned) are cut at the
    pinned positions"""
    out = []
    for i in range(count):
        at = pinned[i] if i < len(pinned) else int(rng.integers(0, len(seq) - m + 1))
        out.append(mutate(rng, seq[at:at + m], i % max_subs_plus_1, alphabet))
    return out


TINY_SYMBOLS = "ACGTN$"   # N: absent from every tiny text; '$': never in a sequence


@functools.lru_cache(maxsize=None)
def tiny_texts():
    rng = np.random.default_rng(20260101)
    return {"banana": "banana", "A": "A", "AC": "AC", "ACGTx3": "ACGT" * 3,
            "dna7": dna(rng, 7).decode(), "dna31": dna(rng, 31).decode()}


@functools.lru_cache(maxsize=None)
def tiny_case(name) -> Case:
    text = tiny_texts()[name]
    n = len(text)
    pats = ["".join(t) for m in range(1, 5) for t in itertools.product(TINY_SYMBOLS, repeat=m)]
    # lengths n, n + 1 and 2n: the text itself, with one symbol changed, extended, doubled
    changed = ("C" if text[0] != "C" else "G") + text[1:]
    pats += [text, changed, text[:-1] + "$", text + text[0], text + "$", "N" + text, text + text, changed + text]
    return Case(text, pats)


BOUNDARY_N = (63, 64, 65, 447, 448, 449, 895, 897, 4097)


@functools.lru_cache(maxsize=None)
def boundary_case(n, leading_a) -> Case:
    rng = np.random.default_rng(1000 * n + leading_a)
    text = (b"A" * 40 + dna(rng, n - 40)) if leading_a else dna(rng, n)
    pats = cut(rng, text, 8, 200, 4, b"ACGT", pinned=(0, n - 8))
    pats += [dna(rng, 8) for _ in range(50)]
    return Case(text, pats)


AT_SIZE_N = 100_003


@functools.lru_cache(maxsize=None)
def at_size_text() -> bytes:
    return dna(np.random.default_rng(77), AT_SIZE_N)


@functools.lru_cache(maxsize=None)
def at_size_case() -> Case:
    """500 20-mers, pattern i with i mod 6 substitutions; run at k = 4"""
    text = at_size_text()
    return Case(text, cut(np.random.default_rng(78), text, 20, 500, 6, b"ACGT", pinned=(0, AT_SIZE_N - 20)))


@functools.lru_cache(maxsize=None)
def at_size_sort_case() -> Case:
    """300 12-mers, pattern i with i mod 4 substitutions; run at k = 3: tens of hits per pattern, the leg of the sort"""
    text = at_size_text()
    return Case(text, cut(np.random.default_rng(79), text, 12, 300, 4, b"ACGT"))


PROTEIN = b"ACDEFGHIKLMNPQRSTVWY"


@functools.lru_cache(maxsize=None)
def protein_case() -> Case:
    rng = np.random.default_rng(81)
    text = np.frombuffer(PROTEIN, np.uint8)[rng.integers(0, 20, 50_000)].tobytes()
    return Case(text, cut(rng, text, 6, 300, 4, PROTEIN))


@functools.lru_cache(maxsize=None)
def bytes_case() -> Case:
    """every byte but '$' (255 symbols), n = 4096; 100 5-mers at k = 1, among them one with 0x00 and one with a byte >= 0x80"""
    rng = np.random.default_rng(82)
    alphabet = bytes(b for b in range(256) if b != ord("$"))
    sym = np.frombuffer(alphabet, np.uint8)
    text = bytearray(sym[rng.integers(0, 255, 4096)].tobytes())
    text[:255] = alphabet                      # every symbol occurs
    text[1000:1005] = b"\x00ab\x00c"
    text[2000:2005] = b"x\x80\xffyz"
    text = bytes(text)
    pats = cut(rng, text, 5, 98, 2, alphabet, pinned=(1000, 1001, 2000, 2001))
    pats += [b"\x00ab\x00c", b"x\x80\xfeyz"]
    return Case(text, pats)


@functools.lru_cache(maxsize=None)
def seven_case() -> Case:
    rng = np.random.default_rng(83)
    alphabet = b"ACGTNRY"
    text = np.frombuffer(alphabet, np.uint8)[rng.integers(0, 7, 1000)].tobytes()
    return Case(text, cut(rng, text, 7, 100, 4, alphabet, pinned=(0, 993)) + [b"ACGTNRY", b"AAAAAAA", b"$CGTNRY"])


@functools.lru_cache(maxsize=None)
def wide_case() -> Case:
    """AC at k = 2 on 10,000 random bases: every position is a hit, the leaves are thousands of rows wide"""
    return Case(dna(np.random.default_rng(84), 10_000), [b"AC"])


@functools.lru_cache(maxsize=None)
def exact_case() -> Case:
    """1,000 patterns without '$' and m <= n, for the agreement with the exact Count / Locate"""
    rng = np.random.default_rng(85)
    text = dna(rng, 5000)
    pats = []
    for i in range(1000):
        m = int(rng.integers(1, 31))
        at = int(rng.integers(0, len(text) - m + 1))
        pats.append(text[at:at + m] if i % 3 else dna(rng, m))
    pats[0], pats[1], pats[2] = text, text[:4999], b"N"
    return Case(text, pats)
