"""The read mapper's test inputs (tests/test_map_cpu.py and tests/test_map_gpu.py share them): one fixed-seed text with
planted repeats, reads sampled from it with errors, unrelated reads and hand-made special cases; the oracle's answers are
computed once per parameter set and cached."""
from __future__ import annotations

import functools

import numpy as np

import map_oracle as mo
import oracle

SEED = 5
GAP = -2
ACGT = np.frombuffer(b"ACGT", np.uint8)

PARAMS_A = mo.Params(seed_len=16, seed_stride=8, max_occ=8, band=16, max_cand=4, both_strands=True, min_score=40)
PARAMS_B = mo.Params(seed_len=12, seed_stride=4, max_occ=2, band=8, max_cand=2, both_strands=False, min_score=1)


def nuc4():
    return oracle.SubstitutionMatrix("-ACGT", "-ACGT", oracle.NUC_4_SCORES)


def dna(rng, n) -> bytes:
    return ACGT[rng.integers(0, 4, n)].tobytes()


def mutate(rng, s: bytes, sub=0.05, ins=0.005, dele=0.005) -> bytes:
    out = bytearray()
    for c in s:
        u = rng.random()
        if u < dele:
            continue
        if u < dele + ins:
            out.append(int(ACGT[rng.integers(0, 4)]))
        if rng.random() < sub:
            c = int(rng.choice([x for x in b"ACGT" if x != c]))
        out.append(c)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def dataset():
    """-> dict: T, R, reads (list of bytes), origin [(start, end, reverse)] of the 600 sampled reads, index of every special"""
    rng = np.random.default_rng(SEED)
    T = bytearray(dna(rng, 20_000))
    R = dna(rng, 300)
    for at in (2000, 9000, 15000):
        T[at:at + 300] = R
    T[12000:12200] = b"A" * 200
    T = bytes(T)
    reads, origin = [], []
    for i in range(600):
        m = int(rng.integers(100, 151))
        at = int(rng.integers(0, len(T) - m + 1))
        r = mutate(rng, T[at:at + m])
        rev = i % 2 == 1
        reads.append(oracle.reverse_complement(r) if rev else r)
        origin.append((at, at + m, rev))
    reads += [dna(rng, 120) for _ in range(50)]
    special = {}

    def add(name, r):
        special[name] = len(reads)
        reads.append(bytes(r))

    add("short", dna(rng, 12))
    add("clip0", dna(rng, 30) + T[0:120])
    add("clipn", T[-120:] + dna(rng, 30))
    add("tie_fwd", R[50:200])
    add("tie_rev", oracle.reverse_complement(R[100:250]))
    add("polyA", b"A" * 120)
    withN = bytearray(T[5000:5120])
    withN[60] = ord("N")
    add("err", withN)
    return dict(T=T, R=R, reads=reads, origin=origin, special=special)


@functools.lru_cache(maxsize=None)
def expected(which: str):
    """the oracle's (hits, info) for parameter set 'a' or 'b'; callers leave it unchanged"""
    d = dataset()
    return mo.map_reads(d["T"], d["reads"], nuc4(), GAP, PARAMS_A if which == "a" else PARAMS_B)
