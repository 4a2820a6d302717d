"""The paired-end mapper's test inputs (tests/test_map_pairs_cpu.py and tests/test_map_pairs_gpu.py share them), after the
recipe of tests/map_affine_inputs.py: one fixed-seed text of 24 kb with planted repeats, 200 sampled pairs of 100-150 bp with
mates of unequal length and inserts of 200-450, hand-made named pairs (one or more per case of the definition), and the
oracle's answers, computed once per setting and cached.  Callers leave what they get unchanged."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import map_inputs as mi
import map_pairs_oracle as mpo
import oracle
import sw_affine_oracle as ao

SEED = 77
MAT = ao.NUC_4
PARAMS = mi.PARAMS_A                          # seed_len 16, stride 8, max_occ 8, band 16, max_cand 4, both strands, min_score 40
# the named pairs run at max_cand 1, 4 and 9; ten plants of U need max_occ >= 10 to be seeded at all
PARAMS_BY_CAND = {1: dataclasses.replace(PARAMS, max_cand=1), 4: PARAMS, 9: dataclasses.replace(PARAMS, max_cand=9, max_occ=16)}
PAIR = mpo.PairParams(200, 450, True)         # rescue windows: 450 - 200 + 150 + 2 * 16 = 432 columns at most
GAPS = ((-5, -2), (-12, -2))
MAX_LEN = 150                                 # what every call passes: one named mate is longer
N = 24_000
R3_AT = (1000, 4000, 7000)                    # a 300-mer planted three times
U_AT = tuple(10_000 + 1300 * k for k in range(10))   # a 400-mer planted ten times
D_AT = (5000, 5130)                           # a 120-mer planted twice, 10 bases apart
rc = oracle.reverse_complement


def spoil(s: bytes, every: int = 12, first: int = 5) -> bytes:
    """a substitution every `every` bases: no 16-mer of s survives, on either strand"""
    out = bytearray(s)
    for i in range(first, len(out), every):
        out[i] = {65: 67, 67: 71, 71: 84, 84: 65}[out[i]]
    return bytes(out)


def fragment(T: bytes, start: int, insert: int, m1: int, m2: int, flip: bool = False):
    """the mates of the fragment T[start, start + insert): the forward one of m1 bytes, the reverse one of m2 (flip: the
    reverse one is mate 1)"""
    f, r = T[start:start + m1], rc(T[start + insert - m2:start + insert])
    return (r, f) if flip else (f, r)


def _first_fallback(T, make, tries=20):
    """make(t) for the first t whose pair has no proper combination and two rescue attempts that both fail at GAPS[0]"""
    for t in range(tries):
        pair = make(t)
        r = mpo.map_pair(T, pair[0], pair[1], MAT, *GAPS[0], PARAMS, PAIR, MAX_LEN)
        if r.case == "fallback" and not r.proper_combos and sum(1 for a in r.attempts if a.res is not None) == 2:
            return pair
    raise AssertionError("no position gives a pair whose rescue attempts both fail")


@functools.lru_cache(maxsize=None)
def dataset():
    """-> dict: T, reads1, reads2, named: name -> index of the pair, sampled: range of the sampled pairs, origin of those"""
    rng = np.random.default_rng(SEED)
    T = bytearray(mi.dna(rng, N))
    R3 = mi.dna(rng, 300)
    for at in R3_AT:
        T[at:at + 300] = R3
    U = mi.dna(rng, 400)
    for at in U_AT:
        T[at:at + 400] = U
    # the ninth copy differs from U where no seed of the combos81 mates reaches: read offset 122 of 125
    for pos in (20 + 122, 250 + 122):
        T[U_AT[8] + pos] = next(c for c in b"ACGT" if c != U[pos])
    D = mi.dna(rng, 120)
    for at in D_AT:
        T[at:at + 120] = D
    # rescue_both_*: mate 2 lies spoiled near mate 1 and clean far away, where a spoiled mate 1 lies near it
    both = {}
    for name, a_at, z_at, k2, k1 in (("rescue_both_a1", 2000, 8000, 12, 9), ("rescue_both_a2", 2600, 8600, 9, 12),
                                     ("rescue_both_tie", 3200, 9200, 12, 12)):
        m1 = bytes(T[a_at:a_at + 120])                 # forward at a_at
        frag2 = mi.dna(rng, 120)                       # mate 2 = rc(frag2): clean at z_at + 230, spoiled at a_at + 230
        T[a_at + 230:a_at + 350] = spoil(frag2, k2)
        T[z_at + 230:z_at + 350] = frag2
        T[z_at:z_at + 120] = spoil(m1, k1)
        both[name] = (m1, rc(frag2))
    T = bytes(T)
    n = len(T)
    reads1, reads2, origin = [], [], []
    for i in range(200):
        m1, m2 = int(rng.integers(100, 151)), int(rng.integers(100, 151))
        insert = int(rng.integers(200, 451))
        at = int(rng.integers(0, n - insert + 1))
        f, r = T[at:at + m1], T[at + insert - m2:at + insert]
        heavy = dict(ins=0.02, dele=0.02) if i % 4 >= 2 else {}
        f, r = mi.mutate(rng, f, **heavy), rc(mi.mutate(rng, r, **heavy))
        if i % 10 == 7:
            r = mi.dna(rng, m2)                        # an unrelated mate
        if i % 10 == 3:
            f = spoil(f)                               # a mate without a seed
        if i % 2:
            f, r = r, f
        reads1.append(f)
        reads2.append(r)
        origin.append((at, insert, bool(i % 2)))
    named = {}

    def add(name, pair):
        named[name] = len(reads1)
        reads1.append(bytes(pair[0]))
        reads2.append(bytes(pair[1]))

    # step 3
    add("repeat_pairing", (T[6740:6860], rc(T[7030:7150])))            # mate 2 inside R3: its first copy ties on its own
    add("repeat_pairing_flip", (rc(T[4040:4170]), T[3720:3830]))       # mate 1 inside R3's second copy
    add("tie_k1k2", (T[4810:4920], rc(D)))                             # inserts 310 and 440: both proper, equal sums
    add("ins_min", fragment(T, 5600, 200, 110, 120))
    add("ins_max", fragment(T, 5600, 450, 110, 120, flip=True))
    add("ins_min_minus1", fragment(T, 6100, 199, 110, 120))
    add("ins_max_plus1", fragment(T, 6100, 451, 110, 120, flip=True))
    # never proper by step 2; a rescue window of 400 columns holds a chance alignment above min_score more often than not,
    # so the first position is taken at which both attempts run and fail
    add("dovetail", _first_fallback(T, lambda t: (T[22250 + 40 * t:22370 + 40 * t], rc(T[22150 + 40 * t:22270 + 40 * t]))))
    add("same_strand", _first_fallback(T, lambda t: (T[22150 + 40 * t:22270 + 40 * t], T[22350 + 40 * t:22480 + 40 * t])))
    add("discordant", fragment(T, 300, 460, 120, 130))                 # each mate lies in the other's window, 10 bases too far
    # step 4
    f, r = fragment(T, 23300, 380, 120, 130)
    add("rescue_anchor_fwd", (f, spoil(r)))                            # "rescue_noseed": no 16-mer of mate 2 survives
    f, r = fragment(T, 9600, 300, 140, 105)
    add("rescue_anchor_rev", (spoil(f), r))
    f, r = fragment(T, 9600, 300, 140, 105, flip=True)
    add("rescue_anchor_rev_flip", (f, spoil(r)))                       # mate 1 reverse anchors mate 2 forward
    add("rescue_short", (T[7500:7640], rc(T[7500:7800])[:12]))         # 12 < seed_len
    for name, pair in both.items():
        add(name, pair)
    f, r = fragment(T, 10, 290, 120, 120)
    add("clip0", (spoil(f), r))                                        # the reverse anchor's window starts below 0
    f, r = fragment(T, n - 300, 300, 120, 120)
    add("clipn", (f, spoil(r)))                                        # the forward anchor's window ends beyond n
    add("clip_empty", (T[n - 100:], mi.dna(rng, 20)))                  # ... and starts there when the mate is short
    add("rescue_err", (T[7650:7770], b"ACGTNACGTACG"))                 # the attempt's alphabet error is not reported
    # steps 5 and 1
    withN = bytearray(rc(T[6400:6520]))
    withN[60] = ord("N")
    add("err_N", (T[6200:6310], withN))
    add("too_long", (T[600:770], rc(T[800:920])))                      # 170 > MAX_LEN
    add("unrelated", (mi.dna(rng, 120), mi.dna(rng, 131)))
    add("empty_mate", (T[5300:5420], b""))
    at = U_AT[8]
    add("combos81", (T[at + 20:at + 145], rc(T[at + 250:at + 375])))   # at max_cand 9: 9 x 9 combinations, the best at (8, 8)
    return dict(T=T, reads1=reads1, reads2=reads2, named=named, sampled=range(200), origin=origin)


def named_pairs():
    d = dataset()
    idx = list(d["named"].values())
    return [d["reads1"][i] for i in idx], [d["reads2"][i] for i in idx], list(d["named"])


@functools.lru_cache(maxsize=None)
def expected(go: int, ge: int, rescue: bool = True):
    """the oracle on the whole set with PARAMS and PAIR -> ([PairResult], counters)"""
    d = dataset()
    return mpo.map_pairs(d["T"], d["reads1"], d["reads2"], MAT, go, ge, PARAMS, dataclasses.replace(PAIR, rescue=rescue), MAX_LEN)


@functools.lru_cache(maxsize=None)
def expected_named(max_cand: int, go: int = -5, ge: int = -2):
    """the oracle on the named pairs at PARAMS_BY_CAND[max_cand] -> ({name: PairResult}, [PairResult], counters)"""
    r1, r2, names = named_pairs()
    res, info = mpo.map_pairs(dataset()["T"], r1, r2, MAT, go, ge, PARAMS_BY_CAND[max_cand], PAIR, MAX_LEN)
    return dict(zip(names, res)), res, info


def run(reads1, reads2, go, ge, P, PP, max_len=MAX_LEN):
    return mpo.map_pairs(dataset()["T"], reads1, reads2, MAT, go, ge, P, PP, max_len)


def flat(results):
    """[PairResult] -> the 2n Hits in output order, the tlen per pair"""
    return [h for r in results for h in (r.h1, r.h2)], [r.tlen for r in results]


@functools.lru_cache(maxsize=None)
def many_pairs():
    """(reads1, reads2): 264 pairs, the whole set and its first pairs again -- more than two chunks of 128"""
    d = dataset()
    k = 264 - len(d["reads1"])
    assert 0 < k < 200
    return d["reads1"] + d["reads1"][:k], d["reads2"] + d["reads2"][:k]


@functools.lru_cache(maxsize=None)
def many_expected(go: int, ge: int):
    res, _ = expected(go, ge)
    r1, _ = many_pairs()
    res = res + res[:len(r1) - len(res)]
    return res, {k: sum(r.info[k] for r in res) for k in mpo.COUNTERS}
