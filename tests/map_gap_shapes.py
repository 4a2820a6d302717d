"""The affine and the paired read mapper's inputs at the shapes only tests/map_shapes.py reaches (tests/test_map_gap_shapes_cpu.py
asserts on the oracles that each reaches the condition it is named for; tests/test_map_affine_shapes_gpu.py and
tests/test_map_pairs_shapes_gpu.py compare the GPU with the oracles on them): the affine oracle's answer to every shape of
map_shapes, and pair shapes for many combinations per pair, chunks without requests or winners, offsets that do not start at
zero, the rescue's complement table, a text shorter than the rescue window, an alphabet error at rank 3.  Builders only: fixed
seeds and places, every shape and every oracle answer cached; callers leave what they get unchanged."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

import map_affine_inputs as mai
import map_affine_oracle as mao
import map_inputs as mi
import map_oracle as mo
import map_pairs_inputs as mpi
import map_pairs_oracle as mpo
import map_shapes as ms
import sw_affine_oracle as ao

GAPS = mai.GAPS
PAIR = mpi.PAIR
rc = ms.rc


# ---------------------------------------------------------------- the affine oracle on map_shapes' shapes
@functools.lru_cache(maxsize=None)
def case_mat():
    return ao.Mat(ms.CASE_ALPHABET, ms.CASE_ALPHABET, ms.case_scores())


@functools.lru_cache(maxsize=None)
def affine_expected(name: str, *args, go: int, ge: int):
    """map_affine_oracle.map_reads on map_shapes.shape(name, *args) -> (hits, info), with the rule of a caller's max_len as
    map_shapes.oracle_map applies it: a longer read has no seeds and err 0xFFFFFFFF"""
    s = ms.shape(name, *args)
    return affine_on(s, tuple(s.reads), go, ge)


def affine_on(s: ms.Shape, reads, go: int, ge: int):
    """the same on some of the shape's reads"""
    mat = case_mat() if s.matrix == "case" else ao.NUC_4
    hits, info = mao.map_reads(s.T, [r if s.max_len is None or len(r) <= s.max_len else b"" for r in reads], mat, go, ge, s.P)
    for h, r in zip(hits, reads):
        h.err = ms.TOO_LONG if s.max_len is not None and len(r) > s.max_len else h.err
    return hits, info


@functools.lru_cache(maxsize=None)
def le2048_first3():
    """traceback_class("le2048") cut to its first three reads (the longest, 2000 bases, is the first)"""
    s = ms.shape("traceback_class", "le2048")
    return dataclasses.replace(s, reads=s.reads[:3])


# The oracle on limits' forward read is 4096 rows by 6158 columns of plain Python at band 1024: 14 s where the other shapes of
# this module take 38 s together (tests/test_map_gap_shapes_cpu.py prints both) -- less than they do, so the band is not halved
LIMITS_BAND, LIMITS_GAPS = 1024, (-12, -2)


@functools.lru_cache(maxsize=None)
def limits_forward(band: int = LIMITS_BAND):
    """limits(band) with its forward read only: max_len 4096"""
    s = ms.shape("limits", band)
    return dataclasses.replace(s, reads=s.reads[:1])


@functools.lru_cache(maxsize=None)
def cut_expected(which: str, *args, go: int, ge: int):
    s = dict(le2048_first3=le2048_first3, limits_forward=limits_forward)[which](*args)
    return affine_on(s, tuple(s.reads), go, ge)


# ---------------------------------------------------------------- pair shapes
@dataclasses.dataclass
class PairShape:
    T: bytes
    reads1: list
    reads2: list
    P: mo.Params
    PP: mpo.PairParams
    max_len: int
    results: list                # the oracle's [PairResult]
    info: dict                   # ... and its counters
    names: list = dataclasses.field(default_factory=list)
    mat: object = ao.NUC_4
    note: dict = dataclasses.field(default_factory=dict)

    def __iter__(self):          # T, reads1, reads2, Params, PairParams, max_len, the oracle's answer
        return iter((self.T, self.reads1, self.reads2, self.P, self.PP, self.max_len, (self.results, self.info)))


def _sum(results):
    return {k: sum(r.info[k] for r in results) for k in mpo.COUNTERS}


def _shape(T, pairs, P, PP, max_len, go, ge, mat=ao.NUC_4, **note):
    """pairs: [(name, mate 1, mate 2)]"""
    r1, r2 = [bytes(p[1]) for p in pairs], [bytes(p[2]) for p in pairs]
    res, info = mpo.map_pairs(T, r1, r2, mat, go, ge, P, PP, max_len)
    return PairShape(bytes(T), r1, r2, P, PP, max_len, res, info, [p[0] for p in pairs], mat, note)


def sub(s: bytes, places) -> bytes:
    """s with a substitution at every place (A -> C -> G -> T -> A)"""
    out = bytearray(s)
    for i in places:
        out[i] = {65: 67, 67: 71, 71: 84, 84: 65}[out[i]]
    return bytes(out)


def few_seeds(s: bytes, keep: int = 2, seed_len: int = 6) -> bytes:
    """s with a substitution every seed_len bases after its first seed_len + keep - 1: `keep` seeds of s survive, the
    first ones"""
    return sub(s, range(seed_len + keep - 1, len(s), seed_len))


# ---- 1. many combinations
# where a mate that keeps two seeds has a rank in the second half of 64: forward (a), (d), reverse (the flipped d)
COMBOS_A_AT, COMBOS_D_AT, COMBOS_F_AT = 9400, 15000, 4500
COMBOS_TIE = dict(a=(3000, 3240), b=(5000, 5240))   # the two fragments of the tie: (mate 1's unit, mate 2's unit), insert 300


@functools.lru_cache(maxsize=None)
def combos_text():
    """text20k() with two 60-mers planted twice each: A' .. B at 3000 and A .. B' at 5000, the primed copy with one
    substitution, so that (A', B) and (A, B') have equal sums and the ranks (1, 0) and (0, 1)"""
    rng = np.random.default_rng(131)
    T = bytearray(ms.text20k())
    A, B = mi.dna(rng, 60), mi.dna(rng, 60)
    (a1, b1), (a2, b2) = COMBOS_TIE["a"], COMBOS_TIE["b"]
    T[a1:a1 + 60], T[b1:b1 + 60] = sub(A, [30]), B
    T[a2:a2 + 60], T[b2:b2 + 60] = A, sub(B, [30])
    return bytes(T), A, B


@functools.lru_cache(maxsize=None)
def pairs_many_combos(max_cand: int = 64, rescue: bool = True, go: int = GAPS[0][0], ge: int = GAPS[0][1]):
    """many_clusters' parameters: hundreds of clusters per 60-base mate, max_cand of them kept, up to 4096 combinations"""
    T, A, B = combos_text()
    P = dataclasses.replace(ms.shape("many_clusters", max_cand).P)
    a, d, f = COMBOS_A_AT, COMBOS_D_AT, COMBOS_F_AT
    pairs = [
        # (a) mate 1 keeps two seeds where it lies: a late rank, and still the best score
        ("late_trip", few_seeds(T[a:a + 60]), rc(T[a + 260:a + 320])),
        # (b) a mate of 8 or 9 bases has fewer clusters; the long mate's rank is late again
        ("short_mate2", few_seeds(T[12000:12060]), rc(T[12292:12300])),
        ("short_mate1", T[12500:12509], rc(few_seeds(T[12740:12800], 3))),
        # (c) equal sums in different trips and lanes
        ("tie_trips", A, rc(B)),
        # (d) the other mate has no seed (5 < seed_len): nothing to combine, a winner of a late rank anchors the rescue
        ("late_anchor", few_seeds(T[d:d + 60]), rc(T[d + 295:d + 300])),
        ("late_anchor_flip", T[f - 240:f - 235], rc(few_seeds(T[f:f + 60]))),
    ]
    return _shape(T, pairs, P, dataclasses.replace(PAIR, rescue=rescue), 60, go, ge)


# ---- 2. chunks of 128 pairs without requests or without winners
CHUNK = 128                                   # map_reads.hip cuts a paired batch into chunks of a multiple of 128 pairs
SANDWICHES = ("empty_middle", "winners_middle", "late_requests")


def _cycle(idx, k):
    return [idx[i % len(idx)] for i in range(k)]


@functools.lru_cache(maxsize=None)
def pairs_sandwich(variant: str = "empty_middle", go: int = GAPS[0][0], ge: int = GAPS[0][1]):
    """3 x 128 pairs at map_pairs_inputs' PARAMS and PAIR, chunk by chunk (note["chunks"] names what each holds):
    empty_middle: sampled pairs | unrelated mates: no request, no winner | proper pairs, then eight that need a rescue
    winners_middle: sampled pairs | proper pairs: winners, no request | sampled pairs
    late_requests: proper pairs: no request | unrelated mates | sampled pairs: requests
    The pairs of the dataset keep the answers map_pairs_inputs.expected has for them."""
    d = mpi.dataset()
    res, _ = mpi.expected(go, ge)
    rng = np.random.default_rng(132)
    proper = [i for i, r in enumerate(res) if r.case == "pair"]
    rescued = [i for i, r in enumerate(res) if r.case == "rescue"]
    sampled = list(d["sampled"])[:CHUNK]
    un1 = [mi.dna(rng, int(rng.integers(100, 151))) for _ in range(CHUNK)]
    un2 = [mi.dna(rng, int(rng.integers(100, 151))) for _ in range(CHUNK)]
    un_res, _ = mpo.map_pairs(d["T"], un1, un2, mpi.MAT, go, ge, mpi.PARAMS, PAIR, mpi.MAX_LEN)

    def of(idx):
        return [d["reads1"][i] for i in idx], [d["reads2"][i] for i in idx], [res[i] for i in idx]

    unrelated = (un1, un2, un_res)
    chunks = dict(empty_middle=(of(sampled), unrelated, of(_cycle(proper, CHUNK - 8) + _cycle(rescued, 8))),
                  winners_middle=(of(sampled), of(_cycle(proper, CHUNK)), of(sampled[::-1])),
                  late_requests=(of(_cycle(proper, CHUNK)), unrelated, of(sampled)))[variant]
    r1, r2, out = [sum((c[k] for c in chunks), []) for k in range(3)]
    return PairShape(d["T"], r1, r2, mpi.PARAMS, PAIR, mpi.MAX_LEN, out, _sum(out), note=dict(chunks=[c[2] for c in chunks]))


# ---- 3. off1[0] != off2[0] != 0
OFFSET_BASES = (37, 5)


@functools.lru_cache(maxsize=None)
def pairs_offsets(go: int = GAPS[0][0], ge: int = GAPS[0][1]):
    """the named pairs; note["packed"] = ((buf1, offs1), (buf2, offs2)) behind 37 and 5 foreign bytes and before some more,
    the offsets not rebased"""
    r1, r2, names = mpi.named_pairs()
    _, res, info = mpi.expected_named(4, go, ge)
    packed = []
    for reads, base, fill in ((r1, OFFSET_BASES[0], b"G"), (r2, OFFSET_BASES[1], b"C")):
        offs = np.zeros(len(reads) + 1, np.uint64)
        offs[0] = base
        offs[1:] = base + np.cumsum([len(r) for r in reads])
        packed.append((np.frombuffer(fill * base + b"".join(reads) + b"T" * 64, np.uint8).copy(), offs))
    return PairShape(mpi.dataset()["T"], r1, r2, mpi.PARAMS, PAIR, mpi.MAX_LEN, res, info, names, note=dict(packed=tuple(packed)))


# ---- 4. the rescue's complement table
ALPHA_SYMBOLS = b"ACGTacgtRYKMBVDHrykmbvdh"
ALPHA_OUTSIDE = 0xC8                          # no symbol of big_matrix() (bytes 1 .. 126)
ALPHA_PAIR = mpo.PairParams(150, 300, True)


def respell(s: bytes, every: int = 6, first: int = 3) -> bytes:
    """the next symbol of ALPHA_SYMBOLS every `every` bytes: no 8-mer of s survives, on either strand"""
    out = bytearray(s)
    for i in range(first, len(out), every):
        out[i] = ALPHA_SYMBOLS[(ALPHA_SYMBOLS.index(out[i]) + 1) % len(ALPHA_SYMBOLS)]
    return bytes(out)


@functools.lru_cache(maxsize=None)
def pairs_alphabet(go: int = GAPS[0][0], ge: int = GAPS[0][1]):
    """a text over upper case, lower case and IUPAC letters, sw_affine_oracle.big_matrix() (126 x 126: it stays in global
    memory).  Mate 1 lies forward and clean; mate 2 is the reverse complement of a stretch 230 further on, respelled so that
    it has no seed there: it is rescued on strand 1, through the kernel's own complement table"""
    rng = np.random.default_rng(133)
    sym = np.frombuffer(ALPHA_SYMBOLS, np.uint8)
    T = bytearray(sym[rng.integers(0, len(sym), 4000)].tobytes())
    T[540:600] = sym[rng.integers(4, 8, 60)].tobytes()              # lower case only
    T[1040:1100] = sym[rng.integers(8, 16, 60)].tobytes()           # R Y K M B V D H only
    T[3350] = ALPHA_OUTSIDE                                         # inside the last pair's rescue window, outside mate 1's
    T = bytes(T)

    def pair(at, edit=lambda s: s):
        return T[at:at + 70], edit(rc(respell(T[at + 230:at + 290])))

    def with_z(s):
        return s[:20] + b"Z" + s[21:]                               # the complement of Z is 0x00

    pairs = [("mixed", *pair(2000)), ("lower", *pair(310)), ("iupac", *pair(810)), ("zero", *pair(2500, with_z)),
             ("window_outside", *pair(3100))]
    P = mo.Params(seed_len=8, seed_stride=4, max_occ=8, band=8, max_cand=4, both_strands=True, min_score=40)
    return _shape(T, pairs, P, ALPHA_PAIR, 70, go, ge, mat=ao.big_matrix())


# ---- 5. a text shorter than the rescue window
@functools.lru_cache(maxsize=None)
def pairs_short_text(go: int = GAPS[0][0], ge: int = GAPS[0][1]):
    """a text of 350 bases, PAIR (200, 450), band 0"""
    rng = np.random.default_rng(134)
    T = mi.dna(rng, 350)
    n = len(T)
    long1 = mi.dna(rng, 20) + T + mi.dna(rng, 40)
    pairs = [
        ("ends", T[0:100], rc(T[n - 100:n])),                       # proper from the candidates: [0, n)
        ("both_clipped", mpi.spoil(T[0:230]), rc(T[250:n])),        # the reverse anchor's window is [-100, 380): cut to [0, n)
        ("both_clipped_flip", rc(mpi.spoil(T[120:n])), T[0:100]),   # the forward anchor's: [-30, 450)
        ("mate1_longer", long1, rc(T[n - 100:n])),                  # 410 bases on a text of 350
    ]
    P = mo.Params(seed_len=16, seed_stride=8, max_occ=8, band=0, max_cand=4, both_strands=True, min_score=40)
    return _shape(T, pairs, P, PAIR, len(long1), go, ge)


# ---- 6. an alphabet error at rank 3
@functools.lru_cache(maxsize=None)
def pairs_rank3_error(go: int = GAPS[0][0], ge: int = GAPS[0][1]):
    """text_error_rank3's text and reads as mates 1; mates 2 are clean, 400 bases from where the read lies in the repeat's
    first copy (at 2000)"""
    s = ms.shape("text_error_rank3")
    T = s.T
    pairs = [("fwd_errs", s.reads[0], rc(T[2080 + 280:2080 + 400])),
             ("rev_errs", s.reads[1], T[2100 + 140 - 400:2100 + 140 - 280]),
             ("clean", s.reads[2], rc(T[2170 + 280:2170 + 400]))]
    return _shape(T, pairs, dataclasses.replace(s.P), PAIR, 140, go, ge)


PAIR_SHAPES = dict(pairs_many_combos=pairs_many_combos, pairs_sandwich=pairs_sandwich, pairs_offsets=pairs_offsets,
                   pairs_alphabet=pairs_alphabet, pairs_short_text=pairs_short_text, pairs_rank3_error=pairs_rank3_error)
