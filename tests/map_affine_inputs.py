"""The affine read mapper's test inputs (tests/test_map_affine_cpu.py and tests/test_map_affine_gpu.py share them): the text
of tests/map_inputs.py's recipe plus two plants of a 150-mer X that tell linear from affine gaps apart, about 300 reads, and
the oracle's answers, computed once per gap setting and parameter set and cached.  Callers leave what they get unchanged."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import map_affine_oracle as mao
import map_inputs as mi
import map_oracle as mo
import oracle
import sw_affine_oracle as ao

SEED = 50
MAT = ao.NUC_4                      # the same table as map_inputs.nuc4()
PARAMS = mi.PARAMS_A                # seed_len 16, stride 8, max_occ 8, band 16, max_cand 4, both strands, min_score 40
GAPS = ((-5, -2), (-12, -2))        # the settings the GPU is compared with the oracle at
X_INS_AT, X_SUB_AT = 4000, 17000    # where the two copies of X start in the text
Z_AT = 7000
COUNTERS = ("seeds", "seeds_over_max_occ", "hits", "clusters", "pairs_aligned", "reads_mapped")


@functools.lru_cache(maxsize=None)
def dataset():
    """-> dict: T, X, reads (list of bytes), special: index of every named read"""
    rng = np.random.default_rng(SEED)
    T = bytearray(mi.dna(rng, 20_000))
    R = mi.dna(rng, 300)
    for at in (2000, 9000, 15000):
        T[at:at + 300] = R
    T[12000:12200] = b"A" * 200
    X = mi.dna(rng, 150)
    ins = X[:75] + mi.dna(rng, 6) + X[75:]              # one copy with 6 bases inserted at X[75]
    T[X_INS_AT:X_INS_AT + len(ins)] = ins
    sub = bytearray(X)                                  # one copy with two substitutions
    for pos in (40, 110):
        sub[pos] = next(c for c in b"ACGT" if c != X[pos])
    T[X_SUB_AT:X_SUB_AT + 150] = sub
    T = bytes(T)
    reads = []
    for i in range(240):
        m = int(rng.integers(100, 151))
        at = int(rng.integers(0, len(T) - m + 1))
        r = mi.mutate(rng, T[at:at + m], ins=0.02, dele=0.02) if i % 4 >= 2 else mi.mutate(rng, T[at:at + m])
        reads.append(oracle.reverse_complement(r) if i % 2 else r)
    reads += [mi.dna(rng, 120) for _ in range(50)]
    special = {}

    def add(name, r):
        special[name] = len(reads)
        reads.append(bytes(r))

    add("short", mi.dna(rng, 12))
    add("clip0", mi.dna(rng, 30) + T[0:120])
    add("clipn", T[-120:] + mi.dna(rng, 30))
    add("tie_fwd", R[50:200])
    add("tie_rev", oracle.reverse_complement(R[100:250]))
    add("polyA", b"A" * 120)
    withN = bytearray(T[5000:5120])
    withN[60] = ord("N")
    add("err", withN)
    add("X", X)
    add("rcX", oracle.reverse_complement(X))
    add("Z", T[Z_AT:Z_AT + 60] + T[Z_AT + 80:Z_AT + 140])
    return dict(T=T, X=X, reads=reads, special=special, unrelated=range(240, 290))


def total(infos):
    return {k: sum(i[k] for i in infos) for k in COUNTERS}


def affine_each(T, reads, go, ge, P, mat=MAT):
    """the affine oracle's ([Hit], [that read's counters])"""
    hits, infos = [], []
    for r in reads:
        info = dict.fromkeys(COUNTERS, 0)
        hits.append(mao.map_read(bytes(T), bytes(r), mat, go, ge, P, info))
        infos.append(info)
    return hits, infos


@functools.lru_cache(maxsize=None)
def expected_each(go: int, ge: int):
    """the affine oracle on the whole read set with PARAMS: ([Hit], [counters per read])"""
    d = dataset()
    return affine_each(d["T"], d["reads"], go, ge, PARAMS)


def expected(go: int, ge: int):
    hits, infos = expected_each(go, ge)
    return hits, total(infos)


@functools.lru_cache(maxsize=None)
def expected_linear(gap: int = -2):
    """tests/map_oracle.py (linear gaps) on the same read set with PARAMS"""
    d = dataset()
    return mo.map_reads(d["T"], d["reads"], mi.nuc4(), gap, PARAMS)


def z_scores():
    """Z's score under the linear gap -2 and under (-12, -2), with no threshold in the way"""
    z = dataset()["special"]["Z"]
    return expected_linear()[0][z].score, expected(-12, -2)[0][z].score


def z_params():
    """PARAMS with a min_score strictly between Z's two scores: mapped under linear gaps, unmapped under (-12, -2)"""
    lin, aff = z_scores()
    assert aff + 1 < lin
    return dataclasses.replace(PARAMS, min_score=(lin + aff) // 2)


def z_reads():
    """a few reads around Z for the threshold case"""
    d = dataset()
    s = d["special"]
    return [d["reads"][i] for i in (s["Z"], s["X"], s["rcX"], 0, 1, 2, 3, s["tie_fwd"])]


# ---- inputs without a winner -----------------------------------------------------------------------------------------------
NO_SCORE = dataclasses.replace(PARAMS, min_score=10 ** 6)   # above any score of 150 bases at 5 a match


@functools.lru_cache(maxsize=None)
def no_winner_cases():
    """name -> (reads, Params): no read of any of them is mapped"""
    d = dataset()
    rng = np.random.default_rng(SEED + 1)
    s = d["special"]
    return {
        "short": ([mi.dna(rng, k) for k in (1, 7, 12, 15, 15)], PARAMS),
        "unrelated": ([d["reads"][i] for i in d["unrelated"]], NO_SCORE),
        "below_min_score": (d["reads"][:12] + [d["reads"][s["X"]]], NO_SCORE),   # candidates and scores, none high enough
        "err": ([d["reads"][s["err"]]], PARAMS),
    }


@functools.lru_cache(maxsize=None)
def sandwich():
    """(reads, slices): 256 reads of the set, 256 unrelated reads, the rest of the set -- with chunks of 256 reads the middle
    chunk has no winner"""
    d = dataset()
    rng = np.random.default_rng(SEED + 2)
    middle = [mi.dna(rng, int(rng.integers(100, 151))) for _ in range(256)]
    return d["reads"][:256] + middle + d["reads"][256:], middle


@functools.lru_cache(maxsize=None)
def sandwich_expected(go: int, ge: int):
    d = dataset()
    _, middle = sandwich()
    hits, infos = expected_each(go, ge)
    mh, mi_ = affine_each(d["T"], middle, go, ge, PARAMS)
    return hits[:256] + mh + hits[256:], total(infos + mi_), mh


# ---- a text that is not DNA, a table that does not go to LDS ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def general_case():
    """-> dict: T over the first 12 symbols of sw_affine_oracle.big_matrix() (bytes 1..12), reads with substitutions and
    indels, forward only, the oracle's answers at (-5, -2)"""
    big = ao.big_matrix()
    rng = np.random.default_rng(SEED + 3)
    sym = np.arange(1, 13, dtype=np.uint8)
    T = sym[rng.integers(0, 12, 3000)].tobytes()
    reads = []
    for _ in range(40):
        m = int(rng.integers(40, 90))
        at = int(rng.integers(0, len(T) - m + 1))
        r = bytearray()
        for c in T[at:at + m]:
            u = rng.random()
            if u < 0.02:
                continue
            if u < 0.04:
                r.append(int(sym[rng.integers(0, 12)]))
            r.append(int(sym[rng.integers(0, 12)]) if rng.random() < 0.04 else c)
        reads.append(bytes(r))
    P = mo.Params(seed_len=8, seed_stride=4, max_occ=8, band=8, max_cand=4, both_strands=False, min_score=1)
    hits, infos = affine_each(T, reads, -5, -2, P, big)
    return dict(T=T, reads=reads, P=P, mat=big, go=-5, ge=-2, hits=hits, info=total(infos))
