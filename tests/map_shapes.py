"""The read mapper's inputs for the shapes tests/map_inputs.py does not reach (tests/test_map_shapes_cpu.py asserts on the
oracle that each of them reaches the condition it is named for, tests/test_map_shapes_gpu.py compares the GPU with the
oracle on them): clusters at and beyond the 64 lanes of a wave, more clusters than lanes, the documented limits, every
traceback kernel the mapper can reach.  Builders only: fixed seeds, every shape and the oracle's answer to it cached."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import map_inputs as mi
import map_oracle as mo
import oracle

GAP = mi.GAP
NO_LIMIT = 0xFFFFFFFF
TOO_LONG = 0xFFFFFFFF   # err of a read longer than max_len
TB_PAIRS = 131072       # map_reads.hip MAP_TB_PAIRS: pairs whose traceback workspace the mapper holds at once
rc = oracle.reverse_complement


@dataclasses.dataclass
class Shape:
    T: bytes
    reads: list
    P: mo.Params
    max_len: int | None = None   # the caller's max_len (None: the longest read's length)
    matrix: str = "nuc4"         # "nuc4" or "case" (CASE_ALPHABET / case_scores())
    tile: int = 1                # the GPU runs `reads` repeated this many times
    note: dict = dataclasses.field(default_factory=dict)


# ---------------------------------------------------------------- the matrices
CASE_ALPHABET = "ACGTacgt"


def case_scores():
    """the same symbol 5, the same base in the other case 2, everything else -4"""
    s = CASE_ALPHABET
    return [[5 if a == b else 2 if a.upper() == b.upper() else -4 for b in s] for a in s]


def matrix(name: str):
    return mi.nuc4() if name == "nuc4" else oracle.SubstitutionMatrix(CASE_ALPHABET, CASE_ALPHABET, case_scores())


# ---------------------------------------------------------------- the oracle with the caller's max_len
def oracle_map(T, reads, mat, gap, P, max_len=None):
    """map_oracle.map_reads, plus the rule of a caller's max_len: a longer read has no seeds and err 0xFFFFFFFF"""
    hits, info = mo.map_reads(T, [r if max_len is None or len(r) <= max_len else b"" for r in reads], mat, gap, P)
    for h, r in zip(hits, reads):
        h.err = TOO_LONG if max_len is not None and len(r) > max_len else h.err
    return hits, info


# ---------------------------------------------------------------- texts
@functools.lru_cache(maxsize=None)
def text20k() -> bytes:
    return mi.dna(np.random.default_rng(101), 20_000)


@functools.lru_cache(maxsize=None)
def repeat_text(copies_at=(2000, 7000, 12000, 17000), unit=300, seed=102):
    """-> (T, R): 20 kb of DNA with the `unit`-base repeat R planted at `copies_at`"""
    rng = np.random.default_rng(seed)
    T = bytearray(mi.dna(rng, 20_000))
    R = mi.dna(rng, unit)
    for at in copies_at:
        T[at:at + unit] = R
    return bytes(T), R


def _mutated(rng, T, lengths):
    """one read per length: a mutated substring of T, every other one reverse-complemented"""
    reads = []
    for i, m in enumerate(lengths):
        at = int(rng.integers(0, len(T) - m + 1))
        r = mi.mutate(rng, T[at:at + m])
        reads.append(rc(r) if i % 2 else r)
    return reads


# ---------------------------------------------------------------- 1. cluster length at the ballot width
BALLOT_FWD = (78, 79, 80, 142, 143, 144)   # seed_len 16, stride 1: 63, 64, 65, 127, 128, 129 seeds on one diagonal
BALLOT_REV = (80, 143, 144, 79)            # 65, 128, 129 and, last in the batch, 64


def ballot(max_occ=4):
    T = text20k()
    rng = np.random.default_rng(111)
    reads = []
    for m in BALLOT_FWD + BALLOT_REV:
        at = int(rng.integers(0, len(T) - m + 1))
        reads.append(T[at:at + m] if len(reads) < len(BALLOT_FWD) else rc(T[at:at + m]))
    P = mo.Params(seed_len=16, seed_stride=1, max_occ=max_occ, band=4, max_cand=4, both_strands=True, min_score=1)
    return Shape(T, reads, P)


# ---------------------------------------------------------------- 2. clusters many ballots long, traceback path 7
def long_clusters():
    rng = np.random.default_rng(112)
    T = bytearray(text20k())
    unit = mi.dna(rng, 37)
    at, rep = 9000, unit * 8
    T[at:at + len(rep)] = rep
    T = bytes(T)
    reads = [T[at - 60:at + 90], rep, rc(T[at + len(rep) - 200:at + len(rep) + 70])]
    P = mo.Params(seed_len=12, seed_stride=2, max_occ=8, band=300, max_cand=4, both_strands=True, min_score=1)
    return Shape(T, reads, P, note=dict(at=at, rep=len(rep)))


# ---------------------------------------------------------------- 3. more clusters than lanes
def many_clusters(max_cand=64):
    T = text20k()
    n = len(T)
    rng = np.random.default_rng(113)
    reads = [T[0:60], T[7000:7060], T[n - 60:n], rc(T[13000:13060])] + [mi.dna(rng, 60) for _ in range(5)]
    P = mo.Params(seed_len=6, seed_stride=1, max_occ=64, band=0, max_cand=max_cand, both_strands=True, min_score=1)
    return Shape(T, reads, P, note=dict(substrings=4))


# ---------------------------------------------------------------- 4. text ends and the band limit
def short_text():
    rng = np.random.default_rng(114)
    T = mi.dna(rng, 60)
    reads = [mi.dna(rng, 20) + T + mi.dna(rng, 40), T[10:50], rc(mi.dna(rng, 5) + T)]
    P = mo.Params(seed_len=8, seed_stride=3, max_occ=8, band=1024, max_cand=4, both_strands=True, min_score=1)
    return Shape(T, reads, P, note=dict(diagonals=(-20, 10, -5)))


def band0_ends():
    T = text20k()
    n = len(T)
    reads = [T[0:100], T[n - 100:n], rc(T[0:90]), rc(T[n - 90:n])]
    P = mo.Params(seed_len=16, seed_stride=8, max_occ=8, band=0, max_cand=4, both_strands=True, min_score=1)
    return Shape(T, reads, P)


def limits(band=1024):
    """max_len 4096 and band 1024, the two documented limits, in one call"""
    T = text20k()
    rng = np.random.default_rng(115)
    reads = []
    for i, at in enumerate((3000, 11000)):
        r = mi.mutate(rng, T[at:at + 4200])[:4096]
        reads.append(rc(r) if i else r)
    P = mo.Params(seed_len=16, seed_stride=8, max_occ=8, band=band, max_cand=1, both_strands=True, min_score=1)
    return Shape(T, reads, P, max_len=4096)


# ---------------------------------------------------------------- 5. max_len given by the caller
def max_len_exceeded():
    T = text20k()
    reads = [T[500:600], T[4000:4150], rc(T[9000:9100])]
    return Shape(T, reads, dataclasses.replace(mi.PARAMS_A), max_len=120)


def max_len_generous():
    T = text20k()
    reads = _mutated(np.random.default_rng(116), T, [150, 100, 149, 120, 16, 15])
    reads = [r[:150] for r in reads]
    return Shape(T, reads, dataclasses.replace(mi.PARAMS_A), max_len=1000)


def max_len_below_seed():
    T = text20k()
    reads = [T[100:110], T[200:209], b"", T[300:301], rc(T[400:410])]
    return Shape(T, reads, dataclasses.replace(mi.PARAMS_A), max_len=10)


# ---------------------------------------------------------------- 6. off[0] != 0
OFFSET_BASE = 37


def offset_packed():
    """-> (buf, offs): max_len_generous()'s reads behind OFFSET_BASE foreign bytes (and before some more), the offsets not
    rebased"""
    reads = max_len_generous().reads
    lens = np.array([len(r) for r in reads], np.uint64)
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[0] = OFFSET_BASE
    offs[1:] = OFFSET_BASE + np.cumsum(lens)
    buf = np.frombuffer(b"G" * OFFSET_BASE + b"".join(reads) + b"T" * 64, np.uint8).copy()
    return buf, offs


def offset_base():
    s = max_len_generous()
    return Shape(s.T, s.reads, s.P)


# ---------------------------------------------------------------- 7. alphabet
def text_error_rank3():
    """four copies of a repeat, an N in the second copy only: for a read over the N's place that copy has the fewest votes
    (rank 3) and is the only candidate that errs"""
    T, R = repeat_text()
    T = bytearray(T)
    T[7000 + 150] = ord("N")
    reads = [R[80:220], rc(R[100:240]), R[170:295]]
    P = mo.Params(seed_len=16, seed_stride=8, max_occ=8, band=16, max_cand=4, both_strands=True, min_score=1)
    return Shape(bytes(T), reads, P)


def zero_bytes():
    """the reverse complement of a byte that is no IUPAC letter is 0x00: strand 1 of Z x 30 hits a run of zero bytes"""
    rng = np.random.default_rng(117)
    T = mi.dna(rng, 500) + b"\x00" * 40 + mi.dna(rng, 500)
    reads = [b"Z" * 30, b"\x00" * 30, T[100:160]]
    P = mo.Params(seed_len=16, seed_stride=4, max_occ=32, band=8, max_cand=4, both_strands=True, min_score=1)
    return Shape(T, reads, P)


def mixed_case():
    rng = np.random.default_rng(118)
    sym = np.frombuffer(CASE_ALPHABET.encode(), np.uint8)
    T = sym[rng.integers(0, 8, 3000)].tobytes()
    reads = []
    for i in range(12):
        m = int(rng.integers(60, 131))
        at = int(rng.integers(0, len(T) - m + 1))
        r = bytearray(T[at:at + m])
        for pos in rng.integers(30, m, 3):   # (the first seeds stay whole)
            r[pos] = int(sym[rng.integers(0, 8)])
        reads.append(rc(bytes(r)) if i % 2 else bytes(r))
    P = mo.Params(seed_len=12, seed_stride=4, max_occ=8, band=8, max_cand=4, both_strands=True, min_score=1)
    return Shape(T, reads, P, matrix="case")


# ---------------------------------------------------------------- 8. min_score on the boundary
def min_score(bound=700):
    T, R = repeat_text()
    P = mo.Params(seed_len=16, seed_stride=8, max_occ=8, band=16, max_cand=4, both_strands=True, min_score=bound)
    return Shape(T, [R[80:220]], P)


# ---------------------------------------------------------------- 9. a chunk without hits between two with hits
def empty_middle_chunk():
    T = text20k()
    rng = np.random.default_rng(119)
    first = _mutated(rng, T, rng.integers(100, 151, 256))
    middle = [mi.dna(rng, 120) if i % 3 else T[i:i + i % 16] for i in range(256)]
    last = _mutated(rng, T, rng.integers(100, 151, 256))
    return Shape(T, first + middle + last, dataclasses.replace(mi.PARAMS_A))


# ---------------------------------------------------------------- 10. more pairs than one traceback workspace
def traceback_fork(tile=72):
    """500 distinct reads of 153..170 bases with four candidates each; the GPU gets them `tile` times over.  (Not longer, and
    band 0: the one-wave-per-pair traceback takes (columns + 67) x 256 bytes per pair, columns = max_len + 3 x band, and the
    mapper holds that for 131,072 pairs -- beyond about 175 columns the whole workspace passes its 8 GiB cap and the mapper
    cuts the READS into chunks instead, each with fewer pairs than the traceback workspace holds.)"""
    T, R = repeat_text()
    rng = np.random.default_rng(120)
    reads = []
    for i in range(500):
        m = int(rng.integers(153, 171))
        at = int(rng.integers(0, len(R) - m + 1))
        r = bytearray(R[at:at + m])
        for pos in rng.integers(0, m, 4):
            r[pos] = int(mi.ACGT[rng.integers(0, 4)])
        reads.append(rc(bytes(r)) if i % 2 else bytes(r))
    P = mo.Params(seed_len=16, seed_stride=8, max_occ=4, band=0, max_cand=4, both_strands=True, min_score=1)
    return Shape(T, reads, P, tile=tile)


# ---------------------------------------------------------------- 12. the traceback kernel by read length
TB_CLASSES = {"le152": (6, 100, 146), "le256": (4, 160, 250), "le1024": (7, 300, 1000), "le2048": (4, 1100, 2000)}


def traceback_class(name):
    path, lo, hi = TB_CLASSES[name]
    T = text20k()
    rng = np.random.default_rng(121 + lo)
    lengths = [hi] + [int(x) for x in rng.integers(lo, hi + 1, 19)]
    P = mo.Params(seed_len=16, seed_stride=8, max_occ=8, band=32, max_cand=4, both_strands=True, min_score=1)
    return Shape(T, _mutated(rng, T, lengths), P, note=dict(path=path))


# ---------------------------------------------------------------- by name, cached
BUILDERS = dict(ballot=ballot, long_clusters=long_clusters, many_clusters=many_clusters, short_text=short_text,
                band0_ends=band0_ends, limits=limits, max_len_exceeded=max_len_exceeded, max_len_generous=max_len_generous,
                max_len_below_seed=max_len_below_seed, offset_base=offset_base, text_error_rank3=text_error_rank3,
                zero_bytes=zero_bytes, mixed_case=mixed_case, min_score=min_score, empty_middle_chunk=empty_middle_chunk,
                traceback_fork=traceback_fork, traceback_class=traceback_class)


@functools.lru_cache(maxsize=None)
def shape(name: str, *args) -> Shape:
    return BUILDERS[name](*args)


@functools.lru_cache(maxsize=None)
def expected(name: str, *args):
    """the oracle's (hits, info) for shape(name, *args), its reads taken once (callers tile); callers leave it unchanged"""
    s = shape(name, *args)
    return oracle_map(s.T, s.reads, matrix(s.matrix), GAP, s.P, s.max_len)
