"""The refs mapper's test inputs (tests/test_map_refs_cpu.py and tests/test_map_refs_gpu.py share them): small hand-made
sets of contigs, one per property of the definition above polyhip_map_reads_refs, a set of 300 contigs with 200 sampled
reads, and the oracle's answers (tests/map_refs_oracle.py), computed once and cached.  Callers leave what they get unchanged.
Sizes are the smallest at which the property shows: seeds of 10 at stride 5, band 6, reads of 20..60, contigs of 1..300."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import map_inputs as mi
import map_oracle as mo
import map_pairs_inputs as mpi
import map_pairs_oracle as mpo
import map_refs_oracle as mro
import oracle
import sw_affine_oracle as ao

SEED = 606
MAT = ao.NUC_4                                   # match 5, mismatch -4
GO, GE = -5, -2
P = mo.Params(seed_len=10, seed_stride=5, max_occ=8, band=6, max_cand=4, both_strands=True, min_score=30)
P24 = mo.Params(seed_len=16, seed_stride=8, max_occ=8, band=24, max_cand=4, both_strands=True, min_score=30)
PP = dataclasses.replace(P, min_score=60)        # pairs: twelve matches, so that no chance alignment in a rescue window passes
PAIR = mpo.PairParams(60, 200, True)
rc = oracle.reverse_complement


def spoil(s: bytes) -> bytes:
    """a substitution every 8 bases: no 10-mer of s survives, on either strand"""
    return mpi.spoil(s, 8, 3)


def join(contigs) -> bytes:
    return b"".join(contigs)


def starts(contigs):
    return np.concatenate([[0], np.cumsum([len(c) for c in contigs])]).astype(np.int64)


@dataclasses.dataclass(frozen=True)
class Case:
    contigs: tuple
    reads: tuple
    P: mo.Params = P
    reads2: tuple | None = None        # pairs: the second mates


def _rng(k: int):
    return np.random.default_rng(SEED + k)


# ---- single reads ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def straddle() -> Case:
    """case 2: the read is X's tail and Y's head; its middle seed exists in C only across the junction"""
    rng = _rng(2)
    X, Y = mi.dna(rng, 100), mi.dna(rng, 100)
    return Case((X, Y), (X[-15:] + Y[:15],))


@functools.lru_cache(maxsize=None)
def max_occ_pair():
    """case 3: (with, without): a seed S with exactly max_occ = 2 occurrences inside contigs, and in `with` one more across
    the junction of the last two contigs"""
    rng = _rng(3)
    S = mi.dna(rng, 10)
    A = mi.dna(rng, 40) + S + mi.dna(rng, 40)
    B = mi.dna(rng, 25) + S + mi.dna(rng, 30)
    D, E = mi.dna(rng, 30), mi.dna(rng, 30)
    read = A[30:70]                                   # S is its seed at offset 10
    other = bytes([next(c for c in b"ACGT" if c != S[5])])
    Pm = dataclasses.replace(P, max_occ=2)
    return (Case((A, B, D + S[:5], S[5:] + E), (read,), Pm), Case((A, B, D + S[:5], other + S[6:] + E), (read,), Pm))


@functools.lru_cache(maxsize=None)
def short_contigs() -> Case:
    """case 4: two adjacent contigs shorter than the band (24) hold the same 16-mer, at local positions 2 and 0"""
    rng = _rng(4)
    M = mi.dna(rng, 16)
    return Case((mi.dna(rng, 50), b"AC" + M, M + b"GTA", mi.dna(rng, 50)), (M,), P24)


@functools.lru_cache(maxsize=None)
def overhang() -> Case:
    """case 5: one read overhangs Q's start by 10 bases, one its end; the neighbours supply the overhangs"""
    rng = _rng(5)
    Pc, Q, R = mi.dna(rng, 80), mi.dna(rng, 90), mi.dna(rng, 70)
    return Case((Pc, Q, R), (Pc[-10:] + Q[:30], Q[-30:] + R[:10]))


@functools.lru_cache(maxsize=None)
def duplicates() -> Case:
    """case 6: the same 60-mer in contigs 2 and 7 of nine"""
    rng = _rng(6)
    D = mi.dna(rng, 60)
    contigs = [mi.dna(rng, int(rng.integers(60, 120))) for _ in range(9)]
    contigs[2] = contigs[2][:20] + D + contigs[2][20:40]
    contigs[7] = contigs[7][:5] + D + contigs[7][5:30]
    return Case(tuple(contigs), (D, rc(D)))


MANY_REPEAT = (5, 50, 100, 150, 200, 250)


@functools.lru_cache(maxsize=None)
def many() -> Case:
    """case 7: 300 contigs of 40..90 bases, 200 reads of 20..60 from random contigs (the first and the last among them), both
    strands, 5 % substitutions"""
    rng = _rng(7)
    contigs = [mi.dna(rng, int(rng.integers(40, 91))) for _ in range(300)]
    R = mi.dna(rng, 50)                                # a repeat in six contigs: reads from it have six clusters, one per contig
    for c in MANY_REPEAT:
        contigs[c] = contigs[c][:10] + R + contigs[c][10:25]
    reads = []
    for i in range(200):
        c = 0 if i == 0 else 299 if i == 1 else MANY_REPEAT[i % 6] if i < 14 else 2 if i < 20 else int(rng.integers(0, 300))
        T = contigs[c]
        m = min(int(rng.integers(20, 61)), len(T))
        at = int(rng.integers(0, len(T) - m + 1))
        r = mi.mutate(rng, T[at:at + m], sub=0.05, ins=0.0, dele=0.0)
        reads.append(rc(r) if i % 2 else r)
    return Case(tuple(contigs), tuple(reads))


@functools.lru_cache(maxsize=None)
def with_n() -> Case:
    """case 8: a set with an N in it (the index takes the general layout); one read lies over the N"""
    rng = _rng(8)
    contigs = [mi.dna(rng, 120) for _ in range(4)]
    c1 = bytearray(contigs[1])
    c1[60] = ord("N")
    contigs[1] = bytes(c1)
    return Case(tuple(contigs), (contigs[0][10:50], contigs[1][40:80], rc(contigs[3][70:110]), contigs[1][70:110]))


@functools.lru_cache(maxsize=None)
def degenerate() -> Case:
    """case 9: a contig shorter than seed_len, a contig of one base, a read longer than its contig"""
    rng = _rng(9)
    K = mi.dna(rng, 25)
    contigs = (mi.dna(rng, 60), b"ACGTA", b"G", K, mi.dna(rng, 45))
    return Case(contigs, (mi.dna(rng, 5) + K + mi.dna(rng, 5), contigs[0][5:45], rc(contigs[4][:30]), b"ACGTAG"))


SINGLE = dict(straddle=straddle, short_contigs=short_contigs, overhang=overhang, duplicates=duplicates, with_n=with_n,
              degenerate=degenerate)


@functools.lru_cache(maxsize=None)
def expected(name: str, max_cand: int | None = None):
    """the refs oracle on a single-read case -> ([RHit], counters)"""
    case = many() if name == "many" else max_occ_pair()[int(name[-1])] if name.startswith("max_occ") else SINGLE[name]()
    Pc = case.P if max_cand is None else dataclasses.replace(case.P, max_cand=max_cand)
    return mro.map_reads(case.contigs, case.reads, MAT, GO, GE, Pc)


@functools.lru_cache(maxsize=None)
def single_text(name: str):
    """the existing single-text oracle (tests/map_affine_oracle.py) on the concatenation of the same case"""
    import map_affine_oracle as mao
    case = SINGLE[name]()
    return mao.map_reads(join(case.contigs), case.reads, MAT, GO, GE, case.P)


# ---- pairs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adjacent_pair() -> Case:
    """case 12: the mates lie on adjacent contigs, 120 apart in C, which fits the insert"""
    rng = _rng(12)
    X, Y = mi.dna(rng, 300), mi.dna(rng, 300)
    return Case((X, Y), (X[230:270],), PP, (rc(Y[10:50]),))


@functools.lru_cache(maxsize=None)
def rescue_clip() -> Case:
    """case 13: the anchor near X's end; the mate has no seed and its only copy is at Y's start, inside the unclipped window"""
    rng = _rng(13)
    X, Y = mi.dna(rng, 300), mi.dna(rng, 300)
    return Case((X, Y), (X[240:280],), PP, (rc(spoil(Y[5:45])),))


@functools.lru_cache(maxsize=None)
def rescue_inside() -> Case:
    """case 14: pairs on contigs k > 0: a rescue anchored on the forward mate and one on the reverse mate (contig 3), a proper
    pair (contig 2), and a pair whose fragment lies in contigs 1 and 4 alike"""
    rng = _rng(14)
    contigs = [mi.dna(rng, 260) for _ in range(5)]
    F = mi.dna(rng, 200)
    contigs[1] = contigs[1][:30] + F + contigs[1][30:60]
    contigs[4] = contigs[4][:10] + F + contigs[4][10:50]
    K2, K3 = contigs[2], contigs[3]
    r1 = (K3[50:90], spoil(K3[60:100]), K2[20:60], F[20:60])
    r2 = (rc(spoil(K3[150:190])), rc(K3[160:200]), rc(K2[120:160]), rc(F[120:160]))
    return Case(tuple(contigs), r1, PP, r2)


PAIRED = dict(adjacent_pair=adjacent_pair, rescue_clip=rescue_clip, rescue_inside=rescue_inside)


@functools.lru_cache(maxsize=None)
def expected_pairs(name: str):
    """the refs oracle on a paired case -> ([PairResult], counters)"""
    case = PAIRED[name]()
    return mro.map_pairs(case.contigs, case.reads, case.reads2, MAT, GO, GE, case.P, PAIR)


@functools.lru_cache(maxsize=None)
def single_text_pairs(name: str):
    case = PAIRED[name]()
    return mpo.map_pairs(join(case.contigs), case.reads, case.reads2, MAT, GO, GE, case.P, PAIR)


@functools.lru_cache(maxsize=None)
def many_pairs() -> Case:
    """case 10 for pairs: 300 pairs on six contigs of 300 bases, inserts of 80..180, mates of 30..50, 3 % substitutions"""
    rng = _rng(10)
    contigs = [mi.dna(rng, 300) for _ in range(6)]
    r1, r2 = [], []
    for i in range(300):
        T = contigs[int(rng.integers(0, 6))]
        ins = int(rng.integers(80, 181))
        at = int(rng.integers(0, len(T) - ins + 1))
        m1, m2 = int(rng.integers(30, 51)), int(rng.integers(30, 51))
        f = mi.mutate(rng, T[at:at + m1], sub=0.03, ins=0.0, dele=0.0)
        r = rc(mi.mutate(rng, T[at + ins - m2:at + ins], sub=0.03, ins=0.0, dele=0.0))
        if i % 7 == 3:
            r = spoil(r)
        if i % 2:
            f, r = r, f
        r1.append(f)
        r2.append(r)
    return Case(tuple(contigs), tuple(r1), PP, tuple(r2))


@functools.lru_cache(maxsize=None)
def many_pairs_expected():
    case = many_pairs()
    return mro.map_pairs(case.contigs, case.reads, case.reads2, MAT, GO, GE, case.P, PAIR)


def flat(results):
    """[PairResult] -> the 2n RHits in output order, the tlen per pair"""
    return [h for r in results for h in (r.h1, r.h2)], [r.tlen for r in results]
