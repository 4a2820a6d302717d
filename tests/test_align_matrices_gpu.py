"""SmithWaterman / NeedlemanWunsch on poly's own substitution tables (tests/golden/matrices.json, the tables of
search/align/matrix/matrices.go) and on synthetic, deliberately asymmetric tables at the alphabet sizes where the plans
switch kernels.  Every pair of every case is compared with the CPU oracle in full -- SW: score, endA, endB, err and both
aligned strings; NW: score, err and both strings -- and every case asserts which kernel ran (align.last_path(),
sw_traceback_last_path(), sw_traceback_last_half(), nw_last_path()), running each kernel that qualifies by switching the
others off (POLYHIP_SW_WAVE / _SW_PAIR, POLYHIP_TB_PROF / _TB_F16 / _TB_WAVE / _TB_WAVE8, POLYHIP_NW_GENERIC).

Which kernel runs (n = codes of the first alphabet, m = of the second; "fits" = (n+1)(m+1)*4 + 512 <= 60 KB, i.e. n, m <= 122
for a square table; cp = (n + 4) & ~3; batches here are below 49,152 pairs except test_full_size_protein_batch):

  score pass (sw_batch.hip choose())                            case here
  1  lane per pair, shared B, <= 256 rows, int8, gap <= -1, cp <= 32   _SW_WAVE=0 on BLOSUM*/PAM*/...; 65,536 x 150 aa
  2  generic                                                    _SW_WAVE=0 (+ _SW_PAIR=0) off the fast path; n >= 123
  4  one wave per pair, shared B, small batch (the fast path's default)   protein tables, <= 256 rows
  5  per-pair B, register-tiled, <= 64 rows (65..256 with _SW_WAVE=0)     protein tables, 5 x 26 / 26 x 5 / 20 x 26
  6  one wave per pair: > 256 rows, gap >= 0, IDENTITY (not int8), cp > 32, per-pair B > 64 rows
  3  packed pass, shared B, <= 7 codes (cp 8), _SW_WAVE=0 at these batch sizes   6- and 7-symbol ladder steps, 5 x 26
  (7, the packed banded pass for > 256 rows, needs <= 7 codes and large batches: tests/test_align_gpu.py)

  traceback (sw_traceback.hip plan() / choose())
  1  byte profile, shared B, <= 152 rows (<= 256 with _TB_WAVE=0), int8, gap <= -1, cp <= 32,
     lenB_pad * 32 + 256 <= 160 KB (BLOSUM62: 5112 residues yes, 5113 no); half-float form when
     (lenB_pad / 4 + 1)(n + 1) * 8 + 256 <= 79 KB (27 codes: lenB <= 1488) and smax * min(lenA, lenB) <= 2047
     (PAM500: 60 rows yes, 61 no)
  2  score table, lane per pair: <= 256 rows where 1 / 5 / 6 do not apply (per-pair B, IDENTITY, 32..122 codes, long B)
  3  generic: > 256 rows with _TB_WAVE=0; n >= 123
  4  one wave per pair: 153..256 rows; 513..1024 rows; 257..512 rows with _TB_WAVE8=0 or IDENTITY / gap >= 0
  5  packed halves, two lanes per pair, shared B, 153..256 rows, smax * 256 <= 2047: MATCH, NUC_4_4
  6  packed halves, per-pair B, <= 152 rows, <= 6 codes: the 6-symbol ladder step and 5 x 26
  7  one wave per pair on a byte profile: 257..512 rows (27 codes: 64 KB of LDS), gap <= -1, smax - gap <= 127

  NW (polyhip_nw_align_batch_dev)
  1  register-tiled, <= 64 rows, fits      2  generic (_NW_GENERIC=1, n >= 123)      3  one wave per pair, 65..4096 rows

The oracle runs on up to 16 host cores; the whole file asks it for fewer than 3e9 cells."""
import concurrent.futures as cf
import json
import os

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrices.json")
with open(GOLDEN) as _f:
    TABLES = json.load(_f)

ENV = ("POLYHIP_SW_WAVE", "POLYHIP_SW_PACKED", "POLYHIP_SW_PAIR", "POLYHIP_TB_PROF", "POLYHIP_TB_F16", "POLYHIP_TB_WAVE",
       "POLYHIP_TB_WAVE8", "POLYHIP_TB_HALF2", "POLYHIP_TB_PAIR16", "POLYHIP_NW_GENERIC")
SW_VARIANTS = [{}, {"POLYHIP_SW_WAVE": "0"}, {"POLYHIP_SW_PAIR": "0"}, {"POLYHIP_SW_WAVE": "0", "POLYHIP_SW_PAIR": "0"},
               {"POLYHIP_SW_WAVE": "0", "POLYHIP_SW_PACKED": "0"}]
TB_VARIANTS = [{}, {"POLYHIP_TB_F16": "0"}, {"POLYHIP_TB_WAVE8": "0"}, {"POLYHIP_TB_WAVE": "0"},
               {"POLYHIP_TB_WAVE": "0", "POLYHIP_TB_PROF": "0"}]
NW_VARIANTS = [{}, {"POLYHIP_NW_GENERIC": "1"}]
CLASSES = [(1, 64), (65, 152), (153, 256), (257, 512), (513, 1024)]


@pytest.fixture(scope="module")
def al():
    from poly_amd import align, alphabet, matrix
    return align, alphabet, matrix


class Table:
    """one substitution table, both as poly_amd scoring and as the oracle's matrix, with what the plans look at"""

    def __init__(self, al, first: str, second: str, scores, gap: int):
        align, alphabet, matrix = al
        s = np.array(scores, dtype=np.int64)
        self.first, self.second, self.gap = first, second, gap
        self.sc = align.NewScoring(matrix.NewSubstitutionMatrix(alphabet.NewAlphabet(list(first)),
                                                                alphabet.NewAlphabet(list(second)), s.tolist()), gap)
        self.om = orc.SubstitutionMatrix(first, second, s)
        self.n, self.m = len(set(first)), len(set(second))
        self.smin, self.smax = int(s.min()), int(s.max())
        self.int8 = self.smin >= -127 and self.smax <= 127
        self.cp = (self.n + 1 + 3) & ~3
        self.fits = (self.n + 1) * (self.m + 1) * 4 + 512 <= 60 * 1024


def _poly(al, name, gap):
    t = TABLES[name]
    return Table(al, t["alphabet"], t["alphabet"], t["scores"], gap)


# ---- the plans' choices for the inputs of this file (the table at the top) -------------------------------------------------

def _off(env, k, v="0"):
    return env.get(k) == v


def sw_path(t: Table, maxA, lenB, shared, env):
    minlen = min(maxA, lenB)
    fast = (shared and t.int8 and t.gap <= -1 and maxA <= 256 and t.cp <= 32 and max(t.smax, 0) * minlen < (1 << 14))
    if fast:
        if t.fits and not _off(env, "POLYHIP_SW_WAVE"):
            return 4
        packed = (t.cp <= 8 and t.smax > 0 and t.smax * minlen < 30000 and lenB < (1 << 18) and t.fits
                  and not _off(env, "POLYHIP_SW_PACKED"))
        return 3 if packed else 1
    wave_possible = 0 < maxA <= 4096 and lenB > 0 and t.fits and not _off(env, "POLYHIP_SW_WAVE")
    if (not shared and (maxA <= 64 or (maxA <= 256 and not wave_possible)) and maxA > 0 and lenB > 0 and t.fits
            and max(t.smax, 0) * minlen < (1 << 14) and not _off(env, "POLYHIP_SW_PAIR")):
        return 5
    return 6 if wave_possible else 2


def tb_path(t: Table, maxA, lenB, shared, env):
    """(path, half)"""
    minlen = min(maxA, lenB)
    reg = maxA <= 256 and t.fits
    ra = (64 if maxA <= 64 else 152 if maxA <= 152 else 256) if reg else 0
    lenB_pad = (lenB + 3) // 4 * 4
    prof_ok = (reg and t.int8 and t.gap <= -1 and t.smax > 0 and t.cp <= 32 and lenB > 0 and
               lenB_pad * (8 if t.cp <= 8 else 32) + 256 <= 160 * 1024)
    halves = t.smax * minlen <= 2047 and t.smax - t.gap <= 2048
    half_lds = (lenB_pad // 4 + 1) * (t.n + 1) * 8 + 256 <= 79 * 1024
    half_ok = prof_ok and ra in (64, 152) and half_lds and halves
    half2_ok = prof_ok and ra == 256 and half_lds and halves
    wave_r = 0
    if 152 < maxA <= 4096 and t.fits:
        wave_r = 4 if maxA <= 256 else 8 if maxA <= 512 else 16 if maxA <= 1024 else 32 if maxA <= 2048 else 64
    smem8 = ((t.n + 1) * (t.m + 1) * 4 + 512 + 15) // 16 * 16 + 4 * (t.m + 1) * wave_r * 64
    wave8_ok = (wave_r in (8, 16) and t.gap <= -1 and -t.gap <= 127 and t.smax - t.gap <= 127 and t.smin - t.gap >= -128
                and smem8 <= 64 * 1024)
    pair16_ok = (reg and ra in (64, 152) and t.n <= 6 and t.int8 and t.gap <= -1 and t.smax > 0 and lenB > 0 and
                 t.smax * minlen <= 2047 and t.smax - t.gap <= 2048)
    f16, prof = not _off(env, "POLYHIP_TB_F16"), not _off(env, "POLYHIP_TB_PROF")
    wave_ok = wave_r != 0 and not _off(env, "POLYHIP_TB_WAVE")
    if shared and half2_ok and prof and f16:
        return 5, True
    if shared and prof_ok and not (ra == 256 and wave_ok) and prof:
        return 1, half_ok and f16
    if ra in (0, 256) and wave_ok:
        return (7 if wave8_ok and not _off(env, "POLYHIP_TB_WAVE8") else 4), False
    if not shared and pair16_ok and f16:
        return 6, True
    return (2 if ra else 3), False


def nw_path(t: Table, maxA, lenB, env):
    if _off(env, "POLYHIP_NW_GENERIC", "1") or not t.fits or maxA == 0 or lenB == 0:
        return 2
    return 1 if maxA <= 64 else 3 if maxA <= 4096 else 2


# ---- the oracle ------------------------------------------------------------------------------------------------------------

def _pool():
    return cf.ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1)))


def oracle_sw(t: Table, reads, refs):
    """(score, endA, endB, err, alignA, alignB) per pair; err = side << 8 | symbol as the kernels report it"""
    def one(ab):
        try:
            s, sa, sb, ea, eb = orc.smith_waterman(ab[0], ab[1], t.om, t.gap)
            return s, ea, eb, 0, sa.encode("latin-1"), sb.encode("latin-1")
        except orc.AlphabetError as e:
            return 0, 0, 0, (e.side << 8) | e.symbol, b"", b""
    with _pool() as ex:
        return list(ex.map(one, zip(reads, refs)))


def oracle_nw(t: Table, reads, refs):
    def one(ab):
        try:
            s, sa, sb = orc.needleman_wunsch(ab[0], ab[1], t.om, t.gap)
            return s, 0, sa.encode("latin-1"), sb.encode("latin-1")
        except orc.AlphabetError as e:
            return 0, (e.side << 8) | e.symbol, b"", b""
    with _pool() as ex:
        return list(ex.map(one, zip(reads, refs)))


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def _pack(seqs):
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), np.uint8).copy(), offs


def _rand(rng, letters: bytes, n: int) -> bytes:
    return bytes(np.frombuffer(letters, np.uint8)[rng.integers(0, len(letters), n)].tolist())


def _mutate(rng, seq: bytes, letters: bytes, sub=0.08, indel=0.02) -> bytes:
    out = bytearray()
    for c in seq:
        r = rng.random()
        if r < indel / 2:
            continue
        if r < indel:
            out.append(letters[int(rng.integers(0, len(letters)))])
        out.append(letters[int(rng.integers(0, len(letters)))] if rng.random() < sub else c)
    return bytes(out)


def make_reference(rng, letters: bytes, length: int) -> bytes:
    """random residues with a tandem repeat planted in the middle (many co-optimal cells)"""
    ref = bytearray(_rand(rng, letters, length))
    unit = _rand(rng, letters, int(rng.integers(5, 12)))
    span = min(length // 4, 300)
    at = length // 2 - span // 2
    ref[at:at + span] = (unit * (span // len(unit) + 1))[:span]
    return bytes(ref)


def make_reads(rng, ref: bytes, letters: bytes, lo: int, hi: int, n: int, pad: int = 60):
    """n reads of lo..hi residues (the first exactly hi): mutated substrings of ref, unrelated reads, repeats (pieces of the
    planted repeat), one empty read; with each, the per-pair B it is aligned to in the per-pair runs (a stretch of ref
    around where it came from, or unrelated)"""
    reads, refs = [], []
    mid = len(ref) // 2
    for i in range(n):
        L = hi if i == 0 else int(rng.integers(lo, hi + 1))
        kind = i % 5
        if kind in (0, 1, 2) or i == 0:
            s = int(rng.integers(0, max(1, len(ref) - L)))
            r = ref[s:s + L]
            if kind != 2 and i != 0:
                r = _mutate(rng, r, letters, sub=[0.02, 0.1, 0.3][i % 3])
            r = (r + _rand(rng, letters, L))[:L] if len(r) < lo else r[:hi]
            b0 = max(0, s - int(rng.integers(0, pad + 1)))
            rb = ref[b0:s + L + int(rng.integers(0, pad + 1))]
        elif kind == 3:
            r = (ref[mid - 40:mid + 40] * (hi // 80 + 2))[:L]
            rb = ref[mid - 150:mid + 150 + L // 2]
        else:
            r = _rand(rng, letters, L)
            rb = _rand(rng, letters, int(rng.integers(max(1, L // 2), L + pad + 1)))
        reads.append(r)
        refs.append(rb)
    reads[-1] = b""
    return reads, refs


# ---- running the entry points ----------------------------------------------------------------------------------------------

def _setenv(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _lens(reads, refs, shared):
    maxA = max(len(r) for r in reads)
    return maxA, (len(refs[0]) if shared else max(len(b) for b in refs))


def _inputs(reads, refs, shared):
    A, offA = _pack(reads)
    if shared:
        return A, offA, np.frombuffer(refs[0], np.uint8).copy(), None
    B, offB = _pack(refs)
    return A, offA, B, offB


def _cmp(what, got, want):
    bad = [p for p, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{what}: {len(bad)} of {len(want)} pairs differ; pair {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


def check_sw(al, monkeypatch, t: Table, reads, refs, shared: bool, score_variants=SW_VARIANTS, tb_variants=TB_VARIANTS,
             strings=True):
    """sw_batch_packed under every score variant, sw_align_packed under every traceback variant, sw_align_strings_packed
    once: every pair equals the oracle, and the kernels that ran are the ones the plans name"""
    align = al[0]
    if shared:
        refs = [refs[0]] * len(reads)
    want = oracle_sw(t, reads, refs)
    maxA, lenB = _lens(reads, refs, shared)
    A, offA, B, offB = _inputs(reads, refs, shared)
    seen = set()
    for env in score_variants:
        _setenv(monkeypatch, env)
        got = align.sw_batch_packed(t.sc, A, offA, B, offB)
        path = align.last_path()
        assert path == sw_path(t, maxA, lenB, shared, env), (env, path)
        seen.add(("sw", path))
        _cmp(f"score path {path} {env}", [tuple(int(x[p]) for x in got) for p in range(len(reads))], [w[:4] for w in want])
    for env in tb_variants:
        _setenv(monkeypatch, env)
        got = align.sw_align_packed(t.sc, A, offA, B, offB)
        path, half = align.sw_traceback_last_path(), align.sw_traceback_last_half()
        assert (align.last_path(), (path, half)) == (sw_path(t, maxA, lenB, shared, env), tb_path(t, maxA, lenB, shared, env)), env
        seen.add(("tb", path, half))
        _cmp(f"traceback path {path} half {half} {env}",
             [tuple(int(x[p]) for x in got[:4]) + (got[4][p], got[5][p]) for p in range(len(reads))], want)
    if strings:
        _setenv(monkeypatch, {})
        got = align.sw_align_strings_packed(t.sc, A, offA, B, offB)
        assert align.sw_traceback_last_path() == tb_path(t, maxA, lenB, shared, {})[0]
        _cmp("packed strings", [tuple(int(x[p]) for x in got[:4]) + (got[4][p], got[5][p]) for p in range(len(reads))], want)
    _setenv(monkeypatch, {})
    return seen


def check_nw(al, monkeypatch, t: Table, reads, refs, shared: bool, variants=NW_VARIANTS):
    align = al[0]
    if shared:
        refs = [refs[0]] * len(reads)
    want = oracle_nw(t, reads, refs)
    maxA, lenB = _lens(reads, refs, shared)
    A, offA, B, offB = _inputs(reads, refs, shared)
    seen = set()
    for env in variants:
        _setenv(monkeypatch, env)
        score, err, sa, sb = align.nw_align_packed(t.sc, A, offA, B, offB)
        path = align.nw_last_path()
        assert path == nw_path(t, maxA, lenB, env), (env, path)
        seen.add(("nw", path))
        _cmp(f"NW path {path} {env}", [(int(score[p]), int(err[p]), sa[p], sb[p]) for p in range(len(reads))], want)
    _setenv(monkeypatch, {})
    return seen


# ---- a. poly's tables through every entry point ----------------------------------------------------------------------------

REAL = ["NUC_4_4", "BLOSUM62", "PAM30", "PAM250", "PAM500", "GONNET", "IDENTITY", "MATCH"]
NREADS = {64: 60, 152: 40, 256: 28, 512: 14, 1024: 8}


@pytest.mark.parametrize("cls", CLASSES, ids=[f"{lo}-{hi}" for lo, hi in CLASSES])
@pytest.mark.parametrize("name", REAL)
def test_poly_tables(al, monkeypatch, name, cls):
    """reads of one length class against a shared reference of 1-5 kb and against per-pair B, gap -1 / -4 / -9 (by table
    and class), through sw_batch_packed, sw_align_packed, sw_align_strings_packed and nw_align_packed"""
    lo, hi = cls
    ti, ci = REAL.index(name), CLASSES.index(cls)
    gap = (-1, -4, -9)[(ti + ci) % 3]
    t = _poly(al, name, gap)
    letters = t.first.replace("-", "").encode()
    rng = np.random.default_rng(1000 * ti + ci)
    reflen = [1000, 1400, 2200, 3100, 5000][(ti + 2 * ci) % 5] if hi <= 256 else [1000, 1600, 2100][ti % 3]
    ref = make_reference(rng, letters, reflen)
    reads, refs = make_reads(rng, ref, letters, lo, hi, NREADS[hi])
    check_sw(al, monkeypatch, t, reads, [ref], shared=True)
    check_sw(al, monkeypatch, t, reads, refs, shared=False, tb_variants=TB_VARIANTS[:1] + TB_VARIANTS[3:4])
    check_nw(al, monkeypatch, t, reads, [ref[:1200]], shared=True)
    check_nw(al, monkeypatch, t, reads, refs, shared=False)


@pytest.mark.parametrize("gap", [0, 1])
@pytest.mark.parametrize("cls", [(1, 64), (65, 152), (153, 256), (257, 512)], ids=["1-64", "65-152", "153-256", "257-512"])
def test_poly_tables_nonnegative_gap(al, monkeypatch, gap, cls):
    """gap 0 (BLOSUM62) and +1 (PAM250): off every lane-per-pair fast path, onto the wave and generic kernels"""
    lo, hi = cls
    t = _poly(al, "BLOSUM62" if gap == 0 else "PAM250", gap)
    letters = t.first.replace("-", "").encode()
    rng = np.random.default_rng(77 + 10 * gap + hi)
    ref = make_reference(rng, letters, 700)
    reads, refs = make_reads(rng, ref, letters, lo, hi, 12)
    check_sw(al, monkeypatch, t, reads, [ref], shared=True)
    check_sw(al, monkeypatch, t, reads, refs, shared=False, tb_variants=TB_VARIANTS[:1] + TB_VARIANTS[3:4])
    check_nw(al, monkeypatch, t, reads, [ref], shared=True)
    check_nw(al, monkeypatch, t, reads, refs, shared=False)


@pytest.mark.parametrize("cls", [(1, 64), (65, 152), (153, 256), (257, 512)], ids=["1-64", "65-152", "153-256", "257-512"])
def test_protein_alphabet_errors(al, monkeypatch, cls):
    """U and O (not in the protein alphabet) and lower case, first / inside / last in the read and in the reference: the
    error symbol and its side (A is checked first at every cell, matrix.go:29-32) equal the oracle's on every path"""
    lo, hi = cls
    t = _poly(al, "BLOSUM62", -4)
    letters = t.first.replace("-", "").encode()
    rng = np.random.default_rng(5 + hi)
    ref = make_reference(rng, letters, 900)
    reads, refs = make_reads(rng, ref, letters, lo, hi, 30)
    for i in range(1, len(reads) - 1, 2):
        r = bytearray(reads[i])
        r[[0, len(r) - 1, len(r) // 2][i % 3]] = b"UOa"[(i // 2) % 3]
        reads[i] = bytes(r)
    bad_refs = [ref, ref[:400] + b"U" + ref[401:], b"o" + ref[1:], ref[:-1] + b"w"]
    for k, b in enumerate(bad_refs):
        check_sw(al, monkeypatch, t, reads, [b], shared=True, score_variants=SW_VARIANTS[:2], tb_variants=TB_VARIANTS[:1])
        check_nw(al, monkeypatch, t, reads, [b], shared=True, variants=NW_VARIANTS[:1])
        per = [bytes(r) for r in refs]
        for i in range(k, len(per), 4):
            if per[i]:
                per[i] = per[i][:len(per[i]) // 2] + b"UOy"[k % 3:k % 3 + 1] + per[i][len(per[i]) // 2 + 1:]
        check_sw(al, monkeypatch, t, reads, per, shared=False, score_variants=SW_VARIANTS[:1], tb_variants=TB_VARIANTS[:1])
        check_nw(al, monkeypatch, t, reads, per, shared=False, variants=NW_VARIANTS[:1])


# ---- b. alphabet-size ladder, asymmetric tables ----------------------------------------------------------------------------

def _symbols(n: int, seed: int) -> str:
    """n distinct one-byte symbols (never NUL: the oracle passes symbols as C strings); 127 = every byte 0x01..0x7F"""
    pool = np.arange(1, 128)
    if n < 127:
        pool = np.random.default_rng(seed).permutation(pool)[:n]
    return "".join(chr(int(c)) for c in pool)


def _random_table(al, first: str, second: str, seed: int, gap: int) -> Table:
    rng = np.random.default_rng(seed)
    s = rng.integers(-9, 10, (len(first), len(second)))
    if len(first) == len(second):
        s[0, 1], s[1, 0] = 7, -5   # never symmetric: a transposed lookup scores differently
        assert (s != s.T).any()
    return Table(al, first, second, s, gap)


LADDER = [6, 7, 8, 26, 31, 32, 122, 123, 127]


@pytest.mark.parametrize("cls", [(1, 64), (65, 152), (153, 256), (257, 400)], ids=["1-64", "65-152", "153-256", "257-400"])
@pytest.mark.parametrize("n", LADDER)
def test_alphabet_size_ladder(al, monkeypatch, n, cls):
    """n-symbol tables with seeded entries in [-9, 9], not symmetric: 6 | 7 (the packed-halves per-pair traceback holds up
    to 6 codes), 8 (cp 12), 26, 31 | 32 (cp 32 | 36: out of the lane-per-pair and byte-profile kernels), 122 | 123 (the
    compact table no longer fits 60 KB of LDS: generic kernels), 127 (every byte 0x01..0x7F)"""
    lo, hi = cls
    sym = _symbols(n, n)
    t = _random_table(al, sym, sym, 100 + n, -3)
    letters = sym.encode("latin-1")
    rng = np.random.default_rng(n * 1000 + hi)
    ref = make_reference(rng, letters, 600)
    reads, refs = make_reads(rng, ref, letters, lo, hi, 24 if hi <= 152 else 8)
    check_sw(al, monkeypatch, t, reads, [ref], shared=True)
    check_sw(al, monkeypatch, t, reads, refs, shared=False, tb_variants=TB_VARIANTS[:2] + TB_VARIANTS[3:4])
    check_nw(al, monkeypatch, t, reads, [ref], shared=True)
    check_nw(al, monkeypatch, t, reads, refs, shared=False)


@pytest.mark.parametrize("cls", [(1, 64), (65, 152), (153, 256), (257, 400)], ids=["1-64", "65-152", "153-256", "257-400"])
@pytest.mark.parametrize("na,nb", [(5, 26), (26, 5), (20, 26)])
def test_two_alphabets_of_different_sizes(al, monkeypatch, na, nb, cls):
    """first and second alphabets of different sizes (na x nb table; the symbols overlap, so reads and references share
    residues): a kernel that swaps the two codes or uses na where it needs nb reads the wrong entry or leaves the table"""
    lo, hi = cls
    protein = "ABCDEFGHIKLMNPQRSTVWYXZ*J-"
    first = protein[:na] if na < nb else protein
    second = protein[:nb] if nb < na else protein
    if na == 20:
        first = "ACDEFGHIKLMNPQRSTVWY"
    t = _random_table(al, first, second, 7 * na + nb, -2)
    rng = np.random.default_rng(na * 100 + nb + hi)
    ref = make_reference(rng, second.encode(), 700)
    reads, refs = make_reads(rng, ref, second.encode(), lo, hi, 24 if hi <= 152 else 8)
    fa = first.encode()
    reads = [bytes(c if c in fa else fa[c % len(fa)] for c in r) for r in reads]   # reads in the first alphabet
    check_sw(al, monkeypatch, t, reads, [ref], shared=True)
    check_sw(al, monkeypatch, t, reads, refs, shared=False, tb_variants=TB_VARIANTS[:2] + TB_VARIANTS[3:4])
    check_nw(al, monkeypatch, t, reads, [ref], shared=True)
    check_nw(al, monkeypatch, t, reads, refs, shared=False)


# ---- c. LDS and score limits at poly's tables ------------------------------------------------------------------------------

@pytest.mark.parametrize("reflen,path", [(5112, 1), (5113, 2)])
def test_byte_profile_lds_limit(al, monkeypatch, reflen, path):
    """the byte-profile traceback at CP = 32 needs lenB_pad * 32 + 256 <= 160 KB: BLOSUM62, 5112 residues fit, 5113 not"""
    t = _poly(al, "BLOSUM62", -4)
    letters = t.first.replace("-", "").encode()
    rng = np.random.default_rng(reflen)
    ref = make_reference(rng, letters, reflen)
    reads, _ = make_reads(rng, ref, letters, 20, 150, 30)
    reads[1] = ref[-150:]   # a hit at the very end of the reference
    assert tb_path(t, 150, reflen, True, {})[0] == path
    seen = check_sw(al, monkeypatch, t, reads, [ref], shared=True, score_variants=SW_VARIANTS[:2], tb_variants=TB_VARIANTS[:2])
    assert ("tb", path, False) in seen


@pytest.mark.parametrize("reflen,half", [(1488, True), (1489, False)])
def test_half_float_traceback_lds_limit(al, monkeypatch, reflen, half):
    """the half-float byte-profile traceback with 27 codes needs (lenB_pad / 4 + 1) * 27 * 8 + 256 <= 79 KB"""
    t = _poly(al, "BLOSUM62", -1)
    letters = t.first.replace("-", "").encode()
    rng = np.random.default_rng(reflen)
    ref = make_reference(rng, letters, reflen)
    reads, _ = make_reads(rng, ref, letters, 20, 152, 30)
    reads[1] = ref[-152:]
    assert tb_path(t, 152, reflen, True, {}) == (1, half)
    seen = check_sw(al, monkeypatch, t, reads, [ref], shared=True, score_variants=SW_VARIANTS[:1], tb_variants=TB_VARIANTS[:2])
    assert ("tb", 1, half) in seen and ("tb", 1, False) in seen


@pytest.mark.parametrize("rows,half", [(60, True), (61, False)])
def test_half_float_traceback_score_limit(al, monkeypatch, rows, half):
    """smax * min(lenA, lenB) <= 2047 for the half-float traceback: PAM500 (W/W = 34) with 60 rows yes, 61 no.  Read 0
    is a run of W that meets one in the reference: the largest score the batch can reach"""
    t = _poly(al, "PAM500", -4)
    letters = t.first.replace("-", "").encode()
    rng = np.random.default_rng(rows)
    ref = bytearray(make_reference(rng, letters, 1000))
    ref[100:100 + rows] = b"W" * rows
    ref = bytes(ref)
    reads, _ = make_reads(rng, ref, letters, 10, rows, 40)
    reads[0] = b"W" * rows
    assert tb_path(t, rows, 1000, True, {}) == (1, half)
    seen = check_sw(al, monkeypatch, t, reads, [ref], shared=True, score_variants=SW_VARIANTS[:1], tb_variants=TB_VARIANTS[:2])
    assert ("tb", 1, half) in seen
    assert int(al[0].sw_batch_packed(t.sc, *_pack(reads[:1]), np.frombuffer(ref, np.uint8).copy(), None)[0][0]) == 34 * rows


@pytest.mark.parametrize("name", ["MATCH", "NUC_4_4"])
def test_two_lane_half_traceback(al, monkeypatch, name):
    """153..256 rows against one reference with smax * 256 <= 2047 (MATCH: 1, NUC_4_4: 5): the packed-halves traceback
    with two lanes per pair (path 5); POLYHIP_TB_F16=0 steps down to the wave kernel, _TB_WAVE=0 + _TB_PROF=0 to the
    table kernel"""
    t = _poly(al, name, -2)
    letters = t.first.replace("-", "").encode()
    rng = np.random.default_rng(len(name))
    ref = make_reference(rng, letters, 1200)
    reads, _ = make_reads(rng, ref, letters, 153, 256, 24)
    assert tb_path(t, 256, 1200, True, {}) == (5, True)
    seen = check_sw(al, monkeypatch, t, reads, [ref], shared=True, score_variants=SW_VARIANTS[:2])
    assert {("tb", 5, True), ("tb", 4, False), ("tb", 2, False)} <= seen


@pytest.mark.parametrize("rows,path", [(512, 7), (513, 4)])
def test_byte_profile_wave_traceback_lds_limit(al, monkeypatch, rows, path):
    """the one-wave-per-pair traceback on a byte profile (path 7) with 27 codes: 257..512 rows fit its 64 KB, 513 do not"""
    t = _poly(al, "BLOSUM62", -4)
    letters = t.first.replace("-", "").encode()
    rng = np.random.default_rng(rows)
    ref = make_reference(rng, letters, 1500)
    reads, refs = make_reads(rng, ref, letters, 257, rows, 6)
    assert tb_path(t, rows, 1500, True, {})[0] == path
    seen = check_sw(al, monkeypatch, t, reads, [ref], shared=True, score_variants=SW_VARIANTS[:1], tb_variants=TB_VARIANTS[:1])
    seen |= check_sw(al, monkeypatch, t, reads, refs, shared=False, score_variants=SW_VARIANTS[:1], tb_variants=TB_VARIANTS[:1])
    assert seen == {("sw", 6), ("tb", path, False)}


# ---- d. one full-size protein batch ----------------------------------------------------------------------------------------

def test_full_size_protein_batch(al, monkeypatch):
    """65,536 reads of up to 150 aa against a 1 kb BLOSUM62 reference: above WAVE_BATCH (49,152 pairs) the score pass is
    the 32-bit lane-per-pair kernel at CP = 32 (path 1) and the traceback the half-float byte-profile kernel.  Every pair
    equals the same batch given as per-pair B (each pair handed the reference: the one-wave-per-pair score kernel and the
    table traceback); a seeded sample of 2,048 pairs equals the oracle, strings included."""
    align = al[0]
    t = _poly(al, "BLOSUM62", -4)
    letters = np.frombuffer(t.first.replace("-", "").encode(), np.uint8)
    rng = np.random.default_rng(65536)
    n, L, LB = 65536, 150, 1000
    ref = letters[rng.integers(0, len(letters), LB)]
    starts = rng.integers(0, LB - L, n)
    reads = ref[starts[:, None] + np.arange(L)[None, :]]
    rate = np.linspace(0.0, 0.8, n)[:, None]
    hit = rng.random((n, L)) < rate
    reads[hit] = letters[rng.integers(0, len(letters), int(hit.sum()))]
    lens = np.where(rng.random(n) < 0.5, L, rng.integers(0, L + 1, n))
    lens[0] = L
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    flat = np.concatenate([reads[i, :lens[i]] for i in range(n)])
    _setenv(monkeypatch, {})
    got = align.sw_align_packed(t.sc, flat, offs, ref.copy(), None)
    assert (align.last_path(), align.sw_traceback_last_path(), align.sw_traceback_last_half()) == (1, 1, True)
    B = np.tile(ref, n)
    offB = np.arange(0, (n + 1) * LB, LB, dtype=np.uint64)
    per = align.sw_align_packed(t.sc, flat, offs, B, offB)
    assert (align.last_path(), align.sw_traceback_last_path()) == (6, 2)
    for k in range(4):
        assert (got[k] == per[k]).all(), k
    assert got[4] == per[4] and got[5] == per[5]
    assert int((got[3] != 0).sum()) == 0
    sample = np.sort(np.random.default_rng(2048).choice(n, 2048, replace=False))
    reads_s = [flat[offs[p]:offs[p + 1]].tobytes() for p in sample]
    want = oracle_sw(t, reads_s, [ref.tobytes()] * len(sample))
    _cmp("full batch sample", [tuple(int(x[p]) for x in got[:4]) + (got[4][p], got[5][p]) for p in sample], want)
