"""The primer-dimer screen without a GPU: the oracle (tests/dimers_oracle.py) against answers written out by hand, the stack table
against its formula worked by hand, what the inputs (tests/dimers_inputs.py) hold, `render`, the declarations, and the argument
errors in their documented order (they are all decided before any device call)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import dimers_inputs as di  # noqa: E402
import dimers_oracle as do  # noqa: E402

NONE = do.NONE
# the table at 310150 mK (37 degrees Celsius), AA AC AG AT CA CC CG CT GA GC GG GT TA TC TG TT
T37 = [-994, -1453, -1287, -873, -1460, -1828, -2164, -1287, -1315, -2232, -1828, -1453, -594, -1315, -1460, -994]


# ---------------------------------------------------------------- 1. the stack table
def test_table_at_37_degrees_by_hand():
    assert do.stack_table(310150) == T37
    # AA: dH -7.6, dS -21.3.  num = -76 * 1e6 + 310150 * 213 = -76,000,000 + 66,061,950 = -9,938,050 -> -993.805 -> -994
    assert -76 * 1_000_000 + 310150 * 213 == -9_938_050 and T37[0] == -994
    # CG: dH -10.6, dS -27.2.  num = -106,000,000 + 310150 * 272 = -106,000,000 + 84,360,800 = -21,639,200 -> -2163.92 -> -2164
    assert -106 * 1_000_000 + 310150 * 272 == -21_639_200 and T37[6] == -2164
    # TA: dH -7.2, dS -21.3.  num = -72,000,000 + 66,061,950 = -5,938,050 -> -593.805 -> -594
    assert T37[12] == -594
    # GC: dH -9.8, dS -24.4.  num = -98,000,000 + 310150 * 244 = -98,000,000 + 75,676,600 = -22,323,400 -> -2232.34 -> -2232
    assert 310150 * 244 == 75_676_600 and T37[9] == -2232


def test_table_at_the_range_ends_and_its_rounding():
    lo, hi = do.stack_table(273150), do.stack_table(338000)
    # 273150 mK: AA num = -76,000,000 + 273150 * 213 = -17,819,050 -> -1781.905 -> -1782; TA -72,000,000 + 58,180,950 -> -1382
    # CG num = -106,000,000 + 273150 * 272 = -31,703,200 -> -3170, the lowest entry of all
    assert lo[0] == -1782 and lo[12] == -1382 and 273150 * 272 == 74_296_800 and min(lo) == lo[6] == -3170
    # 338000 mK: TA num = -72,000,000 + 338000 * 213 = -72,000,000 + 71,994,000 = -6,000 -> -0.6 -> -1: still negative
    assert hi[12] == -1 and max(hi) == -1 and all(-30000 <= v <= 0 for v in lo + hi)
    # ... and above 338028 mK its num is positive: the range ends below that
    assert -72_000_000 + 338029 * 213 == 177 and -72_000_000 + 338028 * 213 == -36
    # half away from zero: a remainder of exactly 5000 goes to the larger magnitude.  AT (-72, -204) at 300000 mK:
    # -72,000,000 + 61,200,000 = -10,800,000 -> -1080 exactly; CC (-80, -199) at 325000: -80,000,000 + 64,675,000 = -15,325,000
    # -> -1532.5 -> -1533
    assert do.stack_table(300000)[3] == -1080 and do.stack_table(325000)[5] == -1533
    with pytest.raises(AssertionError):
        do.stack_table(338001)


def test_table_is_symmetric_under_reverse_complement():
    for temp in (273150, 310150, 338000):
        t = do.stack_table(temp)
        for a in range(4):
            for b in range(4):
                assert t[4 * a + b] == t[4 * (3 - b) + (3 - a)]           # ab read 5'->3' on one strand is comp(b) comp(a) on the other


def test_library_table_equals_the_formula():
    """polyhip_primer_stack_dg needs no device"""
    from poly_amd import _lib, dimers
    assert dimers.stack_dg().tolist() == T37 and dimers.stack_dg(37.0).dtype == np.int32
    out = np.zeros(16, np.int32)
    L = _lib.lib()
    for temp in (273150, 300000, 310150, 325000, 338000):
        assert L.polyhip_primer_stack_dg(temp, out.ctypes.data) == _lib.OK and out.tolist() == do.stack_table(temp)
    for temp in (0, 273149, 338001, 4_000_000_000):
        assert L.polyhip_primer_stack_dg(temp, out.ctypes.data) == _lib.ERR_INVALID and b"temp_mK" in L.polyhip_last_error()
    assert L.polyhip_primer_stack_dg(310150, None) == _lib.ERR_INVALID


# ---------------------------------------------------------------- 2. the oracle against answers worked out by hand
def test_oracle_pairs_by_hand():
    AA, AC, CA, CC, CG, GC, GG, GT, TG, TT = (T37[i] for i in (0, 1, 4, 5, 6, 9, 10, 11, 14, 15))
    # ACGTTGCA: AC CG GT TT TG GC CA
    assert AC + CG + GT + TT + TG + GC + CA == -11216 and 9 * AA == -8946 and 2 * GG + GC + 2 * CC == -9544
    assert AC + CG + GT == -5070 and 3 * GG == -5484
    assert do.revcomp(b"ACGTTGCA") == b"TGCAACGT" and do.revcomp(b"GGGCCC") == b"GGGCCC" and do.revcomp(b"acgtN") == b"NACGT"
    for x, y, want_any, want_end in di.hand():
        p = do.pair(x, y)
        assert (p.dg_any, p.any_shift, p.any_pos, p.any_pairs) == want_any, (x, y, p)
        assert (p.dg_end, p.end_shift, p.end_pairs) == want_end, (x, y, p)
    # the fold: the lower-case pair is the upper-case pair
    assert do.pair(b"acgtNACGT", b"ACGTNACGT") == do.pair(b"ACGTNACGT", b"acgtnacgt")
    # the 64-mer against its reverse complement: all 63 stacks, and the reverse complement sees the same
    x64 = di.hand()[5][0]
    assert len(x64) == 64 and do.pair(do.revcomp(x64), x64).dg_any == do.pair(x64, do.revcomp(x64)).dg_any
    # runs, one by one: GGAGG against CCTCC pairs everything at s = 0; against CCACC the middle breaks the run in two
    assert (GG + T37[8] + T37[2] + GG, 0, 0, 4) in list(do.runs(b"GGAGG", b"CCTCC", T37))
    assert [r for r in do.runs(b"GGAGG", b"CCACC", T37) if r[1] == 0] == [(GG, 0, 0, 1), (GG, 0, 3, 4)]
    # among equal energies the smallest shift: GG twice on x, CC once on y, met at s = -1 (x[0, 1]) and at s = 2 (x[3, 4])
    p = do.pair(b"GGAGG", b"ACCA")
    assert (p.dg_any, p.any_shift, p.any_pos, p.any_pairs) == (GG, -1 + 3, 0, 2) and (p.dg_end, p.end_shift, p.end_pairs) == (GG, 2 + 3, 2)
    # ... then the smallest position: GGACC meets itself at s = 0 only, in the runs GG and CC, which have the same energy
    assert GG == CC and [r for r in do.runs(b"GGACC", b"GGACC", T37)] == [(GG, 0, 0, 1), (CC, 0, 3, 4)]
    p = do.pair(b"GGACC", b"GGACC")
    assert (p.dg_any, p.any_shift, p.any_pos, p.any_pairs) == (GG, 4, 0, 2) and (p.dg_end, p.end_shift, p.end_pairs) == (CC, 4, 2)
    # a table of one's own, zeros among its entries: a run of two pairs with dg 0 is still the run
    zero = [0] * 16
    p = do.pair(b"GG", b"CC", zero)
    assert (p.dg_any, p.any_shift, p.any_pos, p.any_pairs) == (0, 1, 0, 2) and do.screen_row(b"GG", [b"CC"], 0, 0, zero)["any_partner"] == NONE


def test_oracle_dg_any_is_symmetric():
    """the table's symmetry makes dg_any(x, y) == dg_any(y, x): the duplex read from y's side is the same duplex, its stacks the
    reverse complements of x's.  The best run has as many pairs either way on these 3,000 pairs (runs of different length with
    the same energy to the cal/mol, between which the tie rule could choose differently from the two sides, do not occur)"""
    rng = np.random.default_rng(3000)
    for _ in range(3000):
        x, y = di._dna(rng, int(rng.integers(8, 25))), di._dna(rng, int(rng.integers(8, 25)))
        a, b = do.pair(x, y), do.pair(y, x)
        assert a.dg_any == b.dg_any and a.any_pairs == b.any_pairs, (x, y, a, b)


def test_oracle_screen_flags_the_one_end_dimer():
    pool = di.end_dimer_pool()
    a, b = di.END_A, di.END_B
    assert len(pool) == 8 and pool[a][-6:] == do.revcomp(pool[b][-6:]) == b"CGGACC"
    # CG GG GA AC CC
    assert T37[6] + T37[10] + T37[8] + T37[1] + T37[5] == -8588 <= di.END_THRESHOLD < 2 * -2232
    s = do.screen(pool, None, any_threshold=-30000 * 63, end_threshold=di.END_THRESHOLD)
    assert s["end_count"].tolist() == [1 if i in (a, b) else 0 for i in range(8)]
    assert s["end_partner"][a] == b and s["end_partner"][b] == a and s["end_dg"][a] <= -8588 and s["end_pairs"][a] >= 6
    assert s["any_count"].tolist() == [0] * 8
    _, end, _, _ = do.matrix(pool)
    assert sorted(zip(*np.nonzero(end <= di.END_THRESHOLD))) == [(a, b), (b, a)]


# ---------------------------------------------------------------- 3. what the inputs hold
def test_inputs_hold_what_they_promise():
    # the grid: every pair of lengths, three pairs each where a piece of two fits
    for m in di.GRID:
        for n in di.GRID:
            ps = di.grid_pairs(m, n)
            assert len(ps) == (3 if min(m, n) >= 2 else 1) and all(len(x) == m and len(y) == n for x, y in ps)
    p = do.pair(*di.grid_pairs(64, 64)[0])
    assert (p.any_shift, p.any_pos, p.any_pairs, p.end_shift, p.end_pairs) == (63, 0, 64, 63, 64)          # bit 63 of every mask
    (x, y), = di.grid_pairs(64, 1)
    assert do.pair(x, y).any_pairs == 0
    x, y = di.grid_pairs(64, 64)[1]
    assert any(s == 62 and i1 == 63 for _, s, _, i1 in do.runs(x, y, T37))                                   # the largest shift with a stack
    x, y = di.grid_pairs(64, 64)[2]
    assert any(s == -62 and i0 == 0 for _, s, i0, _ in do.runs(x, y, T37))                                   # the smallest
    x, y = di.grid_pairs(33, 63)[0]
    assert do.pair(x, y).any_pairs >= 33
    # sizes
    X, Y = di.sized_pool()
    assert len(X) == 65 and len(Y) == 1000 and {len(p) for p in X + Y} == set(range(6, 15))
    # bad primers
    X, Y = di.bad_lengths()
    s = do.screen(X, Y, -6000, -4000)
    assert s["errX"].tolist() == [0, 1, 0, 2, 2, 0] and s["errY"].tolist() == [2, 0, 1, 0, 2]
    assert s["any_partner"].tolist()[:5] == [1, NONE, 3, NONE, NONE] and s["any_pairs"].tolist()[:5] == [24, 0, 64, 0, 0]
    assert s["any_partner"][5] in (1, 3) and s["any_pairs"][5] < 20          # row 5's reverse complement stands in a bad y only
    assert s["any_count"].tolist()[1] == 0 and s["any_count"].tolist()[3:5] == [0, 0] and s["end_count"].tolist()[:3] == [1, 0, 1]
    a, e, _, _ = do.matrix(X, Y)
    assert not a[[1, 3, 4]].any() and not a[:, [0, 2, 4]].any() and not e[[1, 3, 4]].any() and a[0, 1] < 0 and a[2, 3] < 0
    assert do.info(X, Y) == dict(primers=11, bad=6, pairs=6, shifts=(24 + 64 + 20) * 2 + 3 * (24 + 64) - 6)
    # bytes
    X, Y = di.odd_bytes()
    s = do.screen(X, Y, -6000, -4000)
    assert do.pair(X[0], Y[0]) == do.pair(X[0].upper(), Y[1]) == do.pair(X[4], Y[0])
    assert s["any_pairs"][0] == 12 and s["any_pairs"][1] == 4 and s["any_pairs"][2] == 3 and s["any_pairs"][3] == 4
    assert do.pair(X[2], Y[4]).any_pairs == 0                                                               # U pairs with nothing, A with no U
    assert do.pair(X[0], Y[5]).any_pairs == 4 and do.pair(X[5], Y[0]).any_pairs == 4
    # duplicates: the best partner stands in Y more than once, the first wins
    X, Y = di.duplicates()
    s = do.screen(X, Y, -6000, -4000)
    assert Y[1] == Y[3] == Y[4] and Y[2] == Y[5] and s["any_partner"].tolist() == [1, 2] and s["end_partner"].tolist() == [1, 2]
    assert s["any_count"].tolist()[0] >= 3 and s["any_pairs"].tolist() == [22, 19]
    # no partner
    X, Y = di.no_partner()
    s = do.screen(X, Y, 0, 0)
    assert s["any_partner"].tolist()[:2] == [NONE, NONE] and s["any_dg"].tolist()[:2] == [0, 0] and s["any_partner"][2] != NONE
    assert s["any_count"].tolist()[:2] == [3, 3]                                                            # 0 <= 0: a threshold of 0 counts every valid y
    # the wide set: more y than any chunk, mostly repeats
    X, Y = di.wide()
    assert len(X) == 3 and len(Y) == di.WIDE_NY == 70_000 and len(set(Y)) <= 5376 and {len(y) for y in Y} == {4, 5, 6}
    s = do.screen(X, Y, -2500, -1500)
    assert len({int(j) // 1024 for j in s["any_partner"]}) == 3 and int(s["any_count"].min()) > 1024       # partners in three different chunks
    assert len(di.random_pool()) == 100 and {len(p) for p in di.random_pool()} <= set(range(18, 31))


def test_render_by_hand():
    from poly_amd import dimers
    assert dimers.render("ACGTTGCA", "TGCAACGT", 7) == "ACGTTGCA\n||||||||\nTGCAACGT"
    # x's 3' end on y's 3' end: GGGGAAAA over CCCC at shift 3 and AAAAGGGG over CCCC at shift 7
    assert dimers.render(b"GGGGAAAA", b"CCCC", 3) == "GGGGAAAA\n||||\nCCCC"
    assert dimers.render(b"AAAAGGGG", b"CCCC", 7) == "AAAAGGGG\n    ||||\n    CCCC"
    # y hangs over on the left at a negative s: shift 3 of acgtNACGT / ACGTNACGT is s = -5
    assert dimers.render("acgtNACGT", "ACGTNACGT", 3) == "     acgtNACGT\n     ||||\nTGCANTGCA"
    assert dimers.render("acgtNACGT", "ACGTNACGT", 8) == "acgtNACGT\n|||| ||||\nTGCANTGCA"
    # single pairs show too; unpaired columns are blank
    assert dimers.render("ACAC", "GAGA", 3) == "ACAC\n | |\nAGAG"
    for x, y, want_any, _ in di.hand()[:5]:
        lines = dimers.render(x, y, want_any[1]).split("\n")
        assert max(len(run) for run in lines[1].split(" ")) == want_any[3]
    for bad in (("", "ACGT", 0), ("ACGT", "ACGT", 7), ("ACGT", "ACGT", -1), ("A" * 65, "ACGT", 0)):
        with pytest.raises(ValueError):
            dimers.render(*bad)


# ---------------------------------------------------------------- 4. the declarations and the errors that need no device
def test_declarations():
    from poly_amd import _lib, dimers
    assert len(_lib.SIGNATURES["polyhip_primer_dimer_matrix"][1]) == 11 and len(_lib.SIGNATURES["polyhip_primer_dimer_screen"][1]) == 20
    assert C.sizeof(dimers._CParams) == 72 and C.sizeof(dimers._CInfo) == 40
    assert tuple(n for n, _ in dimers._CInfo._fields_) == do.INFO_FIELDS
    header = open(os.path.join(ROOT, "include", "polyhip.h")).read()
    assert "uint64_t primers, bad, pairs, shifts, launches;" in header and "#define POLYHIP_ABI_VERSION 1\n" in header
    for n in ("polyhip_primer_stack_dg", "polyhip_primer_dimer_matrix", "polyhip_primer_dimer_screen", "polyhip_primer_dimer_last_info"):
        assert f"int {n}(" in header and "polyhip_stream_t" not in header.split(f"int {n}(")[1].split(";")[0]
        assert hasattr(_lib.lib(), n)
    assert "_dev" not in "".join(n for n in _lib.SIGNATURES if "primer_dimer" in n)
    for words in ("NO initiation term", "no terminal-AT term", "no dangling end", "no loop", "no mismatch term", "not a Tm"):
        assert words in header
    assert (dimers.NONE, dimers.MAX_PRIMER) == (do.NONE, do.MAX_PRIMER)
    for f in (dimers.stack_dg, dimers.matrix_packed, dimers.screen_packed, dimers.matrix, dimers.screen, dimers.last_info, dimers.render):
        assert callable(f)
    assert tuple(f for f in dimers.DimerScreen.__dataclass_fields__) == do.SCREEN_FIELDS + ("errX", "errY")


def test_argument_errors_without_gpu():
    """everything the header lists is decided before any device call, in the documented order: each case holds every later fault as
    well"""
    from poly_amd import _lib, dimers
    L = _lib.lib()
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
    seq = np.frombuffer(b"ACGTACGTACGT", np.uint8).copy()
    up, down = np.array([0, 4, 12], np.uint64), np.array([0, 8, 4], np.uint64)
    o32, e32 = np.zeros(4, np.int32), np.zeros(4, np.uint32)
    good = np.array(T37, np.int32)
    low, high = good.copy(), good.copy()
    low[5], high[15] = -30001, 1

    def matrix(table=good, X=seq, offX=up, nx=2, Y=seq, offY=up, ny=2, any_=o32, end=o32, errX=e32, errY=e32):
        rc = L.polyhip_primer_dimer_matrix(p(table), p(X), p(offX), nx, p(Y), p(offY), ny, p(any_), p(end), p(errX), p(errY))
        return rc, L.polyhip_last_error()

    worst = dict(Y=None, ny=2, any_=None, end=None, errX=None, offX=down)                       # every later fault at once
    for kw, status, word in (
            (dict(worst, table=None), INV, b"null stack_dg"),
            (dict(worst, table=low), INV, b"stack_dg[5] = -30001"),
            (dict(worst, table=high), INV, b"stack_dg[15] = 1"),
            (worst, INV, b"Y, offY and ny"),
            (dict(worst, Y=seq, offY=None), INV, b"Y, offY and ny"),
            (dict(worst, Y=seq, ny=0), INV, b"Y, offY and ny"),
            (dict(worst, Y=None, offY=None, ny=3), INV, b"Y, offY and ny"),
            (dict(worst, Y=seq), INV, b"dg_any and dg_end are both NULL"),
            (dict(worst, Y=seq, any_=o32), INV, b"null output: errX"),
            (dict(worst, Y=seq, any_=o32, errX=e32, errY=None), INV, b"null output: errY"),
            (dict(offX=down, X=None), INV, b"null X or offX"),
            (dict(offX=None, offY=down), INV, b"null X or offX"),
            (dict(offX=down, offY=down), INV, b"offX is not ascending at 1"),
            (dict(offY=down), INV, b"offY is not ascending at 1"),
            # 32769 x 32769 > 2^30 in pool mode; the offsets are real, they are read before the limit is
            (dict(Y=None, offY=None, ny=0, errY=None, nx=(1 << 15) + 1, offX=np.arange((1 << 15) + 2, dtype=np.uint64),
                  X=np.zeros(1 << 16, np.uint8)), UNS, b"32769 x 32769 cells"),
    ):
        rc, msg = matrix(**kw)
        assert rc == status and word in msg and b"polyhip_primer_dimer_matrix" in msg, (kw, rc, msg)
    # the empty call needs no device and writes nothing; pool mode needs no errY
    e32[:] = 7
    assert matrix(nx=0, X=None, offX=None)[0] == _lib.OK and matrix(nx=0, X=None, offX=None, Y=None, offY=None, ny=0, errY=None)[0] == _lib.OK
    assert e32.tolist() == [7] * 4 and dimers.last_info() == dict.fromkeys(do.INFO_FIELDS, 0)
    assert L.polyhip_primer_dimer_last_info(None) == INV

    P = dimers._CParams

    def params(table=T37, a=-6000, e=-4000):
        return P((C.c_int32 * 16)(*table), a, e)

    def screen(prm, X=seq, offX=up, nx=2, Y=seq, offY=up, ny=2, outs=None, errX=e32, errY=e32):
        outs = [o32, e32, e32, e32, e32, o32, e32, e32, e32, e32, e32] if outs is None else outs
        rc = L.polyhip_primer_dimer_screen(None if prm is None else C.byref(prm), p(X), p(offX), nx, p(Y), p(offY), ny, *[p(o) for o in outs],
                                           p(errX), p(errY))
        return rc, L.polyhip_last_error()

    none_out = [None] * 11
    worst = dict(Y=None, ny=2, outs=none_out, errX=None, offX=down)
    cases = [
        (None, worst, INV, b"null params"),
        (params(low.tolist(), 1, 1), worst, INV, b"stack_dg[5] = -30001"),
        (params(a=1, e=1), worst, INV, b"any_threshold = 1"),
        (params(a=0, e=1), worst, INV, b"end_threshold = 1"),
        (params(a=0, e=0), worst, INV, b"Y, offY and ny"),
        (params(), dict(worst, Y=seq), INV, b"null output"),
        (params(), dict(worst, Y=seq, outs=None), INV, b"null output: errX"),
        (params(), dict(offX=down, errY=None), INV, b"null output: errY"),
        (params(), dict(offX=down, X=None), INV, b"null X or offX"),
        (params(), dict(offX=down), INV, b"offX is not ascending at 1"),
        (params(), dict(offY=down), INV, b"offY is not ascending at 1"),
    ]
    for k in range(11):                                      # each of the eleven arrays by itself
        outs = [o32, e32, e32, e32, e32, o32, e32, e32, e32, e32, e32]
        outs[k] = None
        cases.append((params(), dict(outs=outs, offX=down), INV, b"null output"))
    for prm, kw, status, word in cases:
        rc, msg = screen(prm, **kw)
        assert rc == status and word in msg and b"polyhip_primer_dimer_screen" in msg, (kw, rc, msg)
    assert screen(params(), nx=0, X=None, offX=None)[0] == _lib.OK
    assert screen(params(a=0, e=0), nx=0, X=None, offX=None, Y=None, offY=None, ny=0, errY=None)[0] == _lib.OK
    # the wrappers
    with pytest.raises(ValueError):
        dimers.matrix_packed(seq, up, seq, None)
    with pytest.raises(ValueError):
        dimers.matrix_packed(seq, [0, 4, 13])
    with pytest.raises(_lib.PolyhipError) as ei:
        dimers.screen(["ACGT"], any_threshold=5)
    assert ei.value.status == INV and "any_threshold = 5" in ei.value.message
    with pytest.raises(_lib.PolyhipError) as ei:
        dimers.matrix(["ACGT"], table=[-40000] * 16)
    assert ei.value.status == INV and "stack_dg[0]" in ei.value.message
    assert dimers.matrix([]).dg_any.shape == (0, 0) and len(dimers.screen([]).any_partner) == 0


def test_kernels_use_no_scratch(tmp_path):
    """what the compiler made of primer_dimers.hip: its kernels, none of which spills to scratch; and it compiles without a
    warning"""
    import re
    import subprocess
    from poly_amd import build
    asm = str(tmp_path / "primer_dimers.s")
    flags = [f for f in build.CXXFLAGS if f != "-fPIC"]
    res = subprocess.run([build._hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(build.CSRC, "primer_dimers.hip"), "-o", asm],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "primer_dimers.hip" not in res.stderr, res.stderr[-2000:]
    seen = {}
    for block in re.split(r"\n\s+- \.", open(asm).read().split("amdhsa.kernels:", 1)[1]):
        name = re.search(r"\.name:\s+\S*?\d+(prepare|pair|detail)_kernel(ILb[01]E)?E", block)
        if name:
            seen[name.group(1) + (name.group(2) or "")] = {key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
                                                           for key in ("vgpr_count", "private_segment_fixed_size")}
    assert sorted(seen) == ["detail", "pairILb0E", "pairILb1E", "prepare"], seen
    for kernel, m in seen.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_count"] <= 64, (kernel, m)
