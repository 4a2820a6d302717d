"""The inputs of tests/nw_shapes.py have the properties they are named for -- asserted on the CPU oracle and on the numpy
restatement of the recurrence (nw_shapes.dp / walk), so that tests/test_nw_shapes_gpu.py is known to take the nine
NeedlemanWunsch kernels through their edges: the rows-per-lane form each longest A selects, last rows in lane 0 / at a
lane's last and first row / in lane 63, B lengths of every residue modulo the steps of a packed word and on both sides
of the 64-column reload, walks that stand on every kind of tied cell, the reference's error order, the int32 range.

Tie kinds visited by the reference's walk, per class over its nine scorings (asserted below, TIE_COUNTS):

    class     diag  diag_tie     up  up_tie   left
    path1     3301      3023    236    2548    882
    R2        4701      4483    794    4066    709
    R8        3935      7169   3559    8851    612
    R32       3697      7418   3730   25640    600
    generic   4607      4522    837    3950    701"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import nw_shapes as ns  # noqa: E402
import oracle as orc  # noqa: E402


def _om(sc: ns.Scoring):
    return orc.SubstitutionMatrix(sc.first, sc.second, np.array(sc.scores, dtype=np.int64))


def _oracle(a, b, sc):
    s, sa, sb = orc.needleman_wunsch(a, b, _om(sc), sc.gap)
    return s, sa.encode("latin-1"), sb.encode("latin-1")


# ---------------------------------------------------------------- the restatement itself
def test_the_numpy_walk_is_the_oracle():
    """dp() / walk() against the oracle: the reference's example, a ladder class, poly's BLOSUM62"""
    assert ns.walk(b"GATTACA", b"GCATGCT", ns.simple(1, -1, -1))[:3] == (0, b"G-ATTACA", b"GCA-TGCT")
    for batch, sc in ((ns.ladder(129), ns.asym(-2)), (ns.ladder(129), ns.asym(0)), (ns.ladder(65), ns.asym(1)),
                      (ns.ladder(64, True), ns.blosum62(-4))):
        for a, b in zip(batch.A, batch.B):
            assert ns.walk(a, b, sc)[:3] == _oracle(a, b, sc), (a, b, sc.gap)


# ---------------------------------------------------------------- 1. ladder
def test_restated_rows_per_lane():
    assert [ns.wave_r(n) for n in ns.LADDER] == [ns.LADDER_R[n] for n in ns.LADDER]
    assert [ns.wave_r(n) for n in (0, 1, 64, 4097, 1 << 20)] == [0] * 5
    # every length has the R of the class it lies in
    bounds = [(65, 128, 2), (129, 192, 3), (193, 256, 4), (257, 512, 8), (513, 1024, 16), (1025, 2048, 32), (2049, 4096, 64)]
    for lo, hi, r in bounds:
        assert {ns.wave_r(n) for n in range(lo, hi + 1)} == {r}
    assert [ns.path(n) for n in ns.LADDER] == [1] + [3] * 14 + [2]
    assert ns.path(65, True) == ns.path(2049, True) == 2


@pytest.mark.parametrize("max_a", ns.LADDER)
def test_ladder_class(max_a):
    r, u = ns.LADDER_R[max_a], ns.unit(max_a)
    assert u == (r or (32 if max_a == 64 else 16))
    for sc, protein in ns.ladder_scorings(max_a):
        b = ns.ladder(max_a, protein)
        letters = set(ns.protein_letters() if protein else ns.DNA)
        assert b.max_a == len(b.A[0]) == max_a and ns.wave_r(b.max_a) == r
        assert all(set(s) <= letters for s in b.A + b.B)
        assert set(letters) <= {ord(c) for c in sc.first}
        assert b.max_b == 190 and (max_a <= 1024 or b.max_b <= 200)
    gaps = [sc.gap for sc, protein in ns.ladder_scorings(max_a) if not protein]
    assert gaps == ([-2, 0, 1] if max_a <= 256 else [-2, 0])
    assert [protein for _, protein in ns.ladder_scorings(max_a)].count(True) == (max_a > 1024)
    assert sum(ns.ladder(max_a, protein).cells for _, protein in ns.ladder_scorings(max_a)) <= ns.MAX_CELLS
    b = ns.ladder(max_a)
    la = sorted({n for n in (1, 2, u - 1, u, u + 1, 2 * u, 63 * u, 63 * u + 1, max_a) if 1 <= n <= max_a})
    assert la == ns.ladder_a_lengths(max_a) and set(la) | {0} <= {len(a) for a in b.A} and b"" in b.B
    # every A length meets every B length
    for n in la:
        assert {len(y) for x, y in zip(b.A, b.B) if len(x) == n} >= set(ns.B_LENGTHS), n
    lb = {len(y) for y in b.B}
    assert {n % 4 for n in lb if 0 < n < 64} == {n % 4 for n in lb if n > 64} == {0, 1, 2, 3}
    assert {63, 64, 65, 127, 128, 129} <= lb and 1 in lb
    # the asymmetric table: no two off-diagonal entries agree
    off = [ns.ASYM[i][j] for i in range(4) for j in range(4) if i != j]
    assert len(set(off)) == 12
    if r:   # the lane and the row of the lane that hold the last row of A
        where = {((n - 1) // r, (n - 1) % r) for n in la if n}
        assert {(0, 0), (0, r - 1), (1, 0)} <= where                      # lane 0, a lane's last row, a lane's first row
        assert any(k == r - 1 for lane, k in where if lane > 0) or max_a < 2 * r
        assert ((max_a - 1) // r, (max_a - 1) % r) in where
        if max_a == 64 * r:                                               # the high side of a switch point: every lane full
            assert {(62, r - 1), (63, 0), (63, r - 1)} <= where
        else:                                                             # the low side: the lanes above the last row are empty
            assert max_a - 1 in ns.LADDER and (max_a - 1) // r < 63
        # B of every residue modulo the steps that share a packed word (4, 2, 1 for R <= 4, 8, 16); lane 63 ends on the
        # word flushed at the last step unless lenB = 1 modulo that
        sp = 4 if r <= 4 else 2 if r == 8 else 1
        assert {n % sp for n in lb if n} == set(range(sp))


# ---------------------------------------------------------------- 2. ties
TIE_COUNTS = {
    "path1": (3301, 3023, 236, 2548, 882),
    "R2": (4701, 4483, 794, 4066, 709),
    "R8": (3935, 7169, 3559, 8851, 612),
    "R32": (3697, 7418, 3730, 25640, 600),
    "generic": (4607, 4522, 837, 3950, 701),
}


@pytest.mark.parametrize("cls", list(ns.TIE_CLASSES))
def test_tie_walks_stand_on_every_kind_of_cell(cls):
    max_a, generic = ns.TIE_CLASSES[cls]
    b = ns.ties(cls)
    assert b.max_a == max_a and b.max_b <= 190
    want_r = {"path1": 0, "R2": 2, "R8": 8, "R32": 32, "generic": 2}[cls]
    assert ns.wave_r(max_a) == want_r and ns.path(max_a, generic) == {"path1": 1, "generic": 2}.get(cls, 3)
    assert any(set(x) == set(y) == {65} and len(x) != len(y) for x, y in zip(b.A, b.B))          # homopolymers
    assert any(x.startswith(b"ACAC") and y.startswith(b"CACA") for x, y in zip(b.A, b.B))        # AC against CA
    assert any(set(x) | set(y) == set(b"AC") and b"AA" in x for x, y in zip(b.A, b.B))            # two letters
    assert any(set(x) == set(ns.DNA) for x in b.A)
    total = dict.fromkeys(ns.KINDS, 0)
    per_gap = {}
    for match, mismatch in ns.TIE_TABLES:
        for gap in ns.TIE_GAPS:
            sc = ns.simple(match, mismatch, gap)
            for x, y in zip(b.A, b.B):
                s, sa, sb, kinds = ns.walk(x, y, sc)
                if len(x) <= 64 or cls == "R2":   # the restatement against the oracle (the long walks: on the GPU module's side)
                    assert (s, sa, sb) == _oracle(x, y, sc)
                for k, v in kinds.items():
                    total[k] += v
                    per_gap[gap, k] = per_gap.get((gap, k), 0) + v
    print(cls, total, per_gap)
    assert all(total[k] >= ns.TIE_MIN for k in ns.KINDS), total
    assert tuple(total[k] for k in ns.KINDS) == TIE_COUNTS[cls]
    # a negative gap alone brings diagonal ties, a positive gap alone up / left ties
    assert per_gap[-1, "diag_tie"] >= ns.TIE_MIN and per_gap[1, "up_tie"] >= ns.TIE_MIN and per_gap[-1, "left"] >= ns.TIE_MIN


# ---------------------------------------------------------------- 3. error order
@pytest.mark.parametrize("cls", list(ns.ERR_CLASSES))
def test_error_order(cls):
    max_a, generic = ns.ERR_CLASSES[cls]
    b, want, what = ns.errors(cls)
    assert b.max_a == max_a and b.max_b == 150
    assert ns.wave_r(max_a) == {"path1": 0, "R2": 2, "R16": 16, "generic": 2}[cls]
    om = _om(ns.asym(-2))
    for a, y, w, name in zip(b.A, b.B, want, what):
        try:
            s, sa, sb = orc.needleman_wunsch(a, y, om, -2)
            got = 0
        except orc.AlphabetError as e:
            got = (e.side << 8) | e.symbol
        assert got == w, name
        if name.endswith("no error"):
            assert (s, sa, sb) == (-2 * max(len(a), len(y)), "", "")
    bad = lambda s: [i for i, c in enumerate(s) if c not in ns.DNA]   # noqa: E731
    ia = {tuple(bad(a)) for a, y in zip(b.A, b.B) if not bad(y) and y}
    ib = {tuple(bad(y)) for a, y in zip(b.A, b.B) if not bad(a) and a}
    assert {(0,), (1,), (63,), (max_a - 1,)} <= ia and {(0,), (63,), (64,), (149,)} <= ib
    if max_a > 64:
        assert {(64,), (65,)} <= ia
    assert any(len(i) == 2 for i in ia) and any(len(i) == 2 for i in ib)
    both = [(bad(a), bad(y)) for a, y in zip(b.A, b.B) if bad(a) and bad(y) and a and y]
    assert any(i[0] == 0 for i, j in both) and any(i[0] > 0 for i, j in both)
    assert len(set(want)) >= 14   # the symbols differ, so a wrong index shows


# ---------------------------------------------------------------- 4. chunks / 5. shared B
@pytest.mark.parametrize("cls", list(ns.DEV_CLASSES))
def test_dev_batch(cls):
    max_a, max_b, generic = ns.DEV_CLASSES[cls]
    b = ns.dev_batch(cls)
    assert len(b.A) == ns.DEV_PAIRS == 2 * ns.DEV_CHUNK + 88
    assert (b.max_a, b.max_b) == (max_a, max_b) and [len(a) for a in b.A[:3]] == [0, 1, max_a]
    assert ns.wave_r(max_a) == {"path1": 0, "R2": 2, "R8": 8, "generic": 2}[cls]
    for lo in (0, 256, 512):   # every launch holds invalid symbols, empty strings and pairs that align
        part = list(zip(b.A, b.B))[lo:lo + 256]
        assert any(ord("N") in a for a, y in part) and any(a and not y for a, y in part)
        assert sum(1 for a, y in part if len(a) > 20 and len(y) > 20) > 40


@pytest.mark.parametrize("cls", list(ns.SHARED_CLASSES))
def test_shared_b(cls):
    max_a, generic = ns.SHARED_CLASSES[cls]
    A, Bs = ns.shared(cls)
    assert max(map(len, A)) == len(A[0]) == max_a and b"" in A and A[3][0] == ord("X")
    assert ns.wave_r(max_a) == {"path1": 0, "R2": 2, "R16": 16, "generic": 2}[cls]
    assert [len(y) for y in Bs] == [1, 63, 64, 65, 200, 200]
    assert [i for i, c in enumerate(Bs[5]) if c not in ns.DNA] == [64] and all(set(y) <= set(ns.DNA) for y in Bs[:5])


# ---------------------------------------------------------------- 6. the int32 range
@pytest.mark.parametrize("cls", list(ns.GUARD_CASES))
@pytest.mark.parametrize("gap", [-ns.BIG, ns.BIG])
def test_guard_batch_runs_next_to_the_int32_limits(cls, gap):
    max_a, max_b, generic = ns.GUARD_CASES[cls]
    b = ns.guard_batch(max_a, max_b)
    sc = ns.big(gap)
    assert (b.max_a, b.max_b) == (max_a, max_b) and ns.BIG * (max_a + max_b) == 2**31 - 2**24
    assert ns.path(max_a, generic) == {"path1": 1, "R2": 3, "generic": 2}[cls]
    lo = hi = 0
    for a, y in zip(b.A, b.B):
        H, _ = ns.dp(a, y, sc)
        lo, hi = min(lo, int(H.min())), max(hi, int(H.max()))
        assert ns.walk(a, y, sc)[:3] == _oracle(a, y, sc)   # the oracle's 64 bits hold what Python's integers give
    assert -2**31 < lo and hi < 2**31
    if gap > 0:
        assert hi == 2**31 - 2**24          # every step a gap: BIG * (lenA + lenB)
    else:
        assert hi == ns.BIG * max_b and lo == -ns.BIG * max_a
    for ra, rb in ns.GUARD_REFUSED:
        assert ns.BIG * (ra + rb) == 2**31
