"""Smith-Waterman with affine gaps on the GPU against tests/sw_affine_oracle.py: every comparison is exact, on all six
outputs (score, endA, endB, err, alignA, alignB).  tests/test_sw_affine_cpu.py asserts that the shared inputs hold what
each test here is meant to exercise."""
import os
import sys
import threading

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import sw_affine_oracle as ao  # noqa: E402

from poly_amd import _lib, align  # noqa: E402
from poly_amd.mash import _pack  # noqa: E402

pytestmark = pytest.mark.gpu

_SCORINGS = {}


def scoring(mat, gap=-1):
    key = (id(mat), gap)
    if key not in _SCORINGS:
        _SCORINGS[key] = (mat, mat.scoring(gap))
    return _SCORINGS[key][1]


def packed(case):
    A, offA = _pack(list(case.A))
    if case.shared:
        return A, offA, _pack([case.B])[0], None
    B, offB = _pack(list(case.B))
    return A, offA, B, offB


def run(case, capacity=None):
    """both calls on a case -> the six outputs of the strings call, after checking the score call gives the same four"""
    A, offA, B, offB = packed(case)
    sc = scoring(case.mat)
    s1 = align.sw_affine_packed(sc, case.go, case.ge, A, offA, B, offB)
    score, endA, endB, err, sa, sb = align.sw_affine_align_packed(sc, case.go, case.ge, A, offA, B, offB, capacity=capacity)
    for x, y in zip(s1, (score, endA, endB, err)):
        assert (x == y).all(), case.name
    return [ao.Result(int(score[p]), int(endA[p]), int(endB[p]), int(err[p]), sa[p], sb[p]) for p in range(len(case.A))]


def check(case, **kw):
    got, want = run(case, **kw), ao.expect(case)
    bad = [p for p in range(len(want)) if got[p] != want[p]]
    assert not bad, (case.name, len(bad), bad[:5], [(got[p], want[p]) for p in bad[:2]])


@pytest.fixture(scope="module")
def rb():
    """RB of the kernel that ran, from the library"""
    align.SmithWatermanAffine("ACGT", "ACGT", scoring(ao.ACGT), -3, -1)
    info = align.sw_affine_last_info()
    assert info["pairs"] == 1 and info["cells"] == 16 and info["tb_cells"] == 16 and info["chunks"] == 1
    assert info["rows_per_band"] == ao.rows_per_band()
    return info["rows_per_band"]


# a. the three known answers
def test_known_answers():
    for A, B, match, mismatch, go, ge, score, alignA, alignB, endA, endB in ao.KNOWN:
        assert align.SmithWatermanAffine(A, B, scoring(ao.simple("ACGT", match, mismatch)), go, ge) == (score, alignA, alignB)
    res = align.SmithWatermanAffineBatch([k[0] for k in ao.KNOWN[:1]] * 3 + ["AAxA"], ao.KNOWN[0][1], scoring(ao.simple("ACGT", 2, -3)), -5, -1)
    assert res[:3] == [(20, ao.KNOWN[0][7], ao.KNOWN[0][8])] * 3 and str(res[3]) == "Symbol x not in alphabet"
    with pytest.raises(align.alphabet.Error, match="Symbol x not in alphabet"):
        align.SmithWatermanAffine("AAxA", "AAAA", scoring(ao.ACGT), -3, -1)
    assert align.SmithWatermanAffine("", "AAAA", scoring(ao.ACGT), -3, -1) == (0, "", "")


# b. band edges
def test_band_edges(rb):
    for case in ao.band_cases(rb):
        check(case)


# c. mixed batch in one wave, pair counts around the wave and the workgroup
@pytest.mark.parametrize("npairs", [1, 63, 64, 65, 257])
def test_mixed_batch(rb, npairs):
    check(ao.prefix(ao.mixed_case(rb), npairs))


def test_mixed_batch_shared_reference(rb):
    mixed = ao.mixed_case(rb)
    check(ao.Case("mixed-shared", mixed.mat, mixed.go, mixed.ge, mixed.A[:130], mixed.B[0] + mixed.B[1], True))
    # an invalid symbol in the shared B: every pair with a valid a[0] names it
    check(ao.Case("mixed-shared-bad", mixed.mat, mixed.go, mixed.ge, mixed.A[:70], mixed.B[0] + b"y" + mixed.B[1], True))
    check(ao.Case("mixed-shared-empty", mixed.mat, mixed.go, mixed.ge, mixed.A[:70], b"", True))


# d. tie rules
def test_tie_rules():
    check(ao.tie_case())


# e. long gaps and the window
def test_long_gaps_and_windows():
    for case in ao.gap_cases():
        check(case)


# f. linear parity
@pytest.mark.parametrize("shared", [True, False])
def test_equal_gaps_are_the_linear_kernels(shared):
    case = ao.parity_batch(shared)
    A, offA, B, offB = packed(case)
    want = align.sw_align_strings_packed(scoring(case.mat, -2), A, offA, B, offB)
    got = align.sw_affine_align_packed(scoring(case.mat, -2), -2, -2, A, offA, B, offB)
    assert int(want[0].min()) > 300 and any(b"-" in s for s in want[4]) and any(b"-" in s for s in want[5])
    for x, y in zip(want[:4], got[:4]):
        assert (x == y).all()
    assert want[4] == got[4] and want[5] == got[5]
    info = align.sw_affine_last_info()
    assert info["pairs"] == 300 and info["table_in_lds"]
    assert info["cells"] == sum(len(a) * (len(case.B) if shared else len(case.B[p])) for p, a in enumerate(case.A))
    assert 0 < info["tb_cells"] < info["cells"]


# g. table in global memory
def test_table_in_global_memory_and_two_alphabets():
    big, shared, asym = ao.table_cases()
    check(big)
    assert align.sw_affine_last_info()["table_in_lds"] is False
    check(shared)
    assert align.sw_affine_last_info()["table_in_lds"] is False
    check(asym)
    assert align.sw_affine_last_info()["table_in_lds"] is True


# h. chunks and the capacity
def test_chunks_of_pairs(rb, monkeypatch):
    case = ao.mixed_case(rb)
    check(case)
    assert align.sw_affine_last_info()["chunks"] == 1
    monkeypatch.setenv("POLYHIP_SWA_CHUNK_PAIRS", "64")
    check(case)
    info = align.sw_affine_last_info()
    assert info["chunks"] >= 5 and info["pairs"] == 300


@pytest.mark.parametrize("chunk", [None, "64"])
def test_capacity_too_small(rb, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("POLYHIP_SWA_CHUNK_PAIRS", chunk)
    case = ao.mixed_case(rb)
    want = ao.expect(case)
    need = sum(len(r.alignA) for r in want)
    A, offA, B, offB = packed(case)
    n = len(case.A)
    score = np.zeros(n, np.int64)
    endA, endB, err = (np.zeros(n, np.uint32) for _ in range(3))
    off = np.zeros(n + 1, np.uint64)
    cap = need - 1
    alnA, alnB = np.full(cap, 7, np.uint8), np.full(cap, 7, np.uint8)
    rc = _lib.lib().polyhip_sw_affine_align_batch_packed(
        scoring(case.mat).handle(), case.go, case.ge, A.ctypes.data, offA.ctypes.data, n, B.ctypes.data, offB.ctypes.data, 0,
        score.ctypes.data, endA.ctypes.data, endB.ctypes.data, err.ctypes.data, alnA.ctypes.data, alnB.ctypes.data,
        off.ctypes.data, cap)
    assert rc == _lib.ERR_INVALID and b"aln_capacity" in _lib.lib().polyhip_last_error()
    assert int(off[-1]) == need and off.tolist() == np.cumsum([0] + [len(r.alignA) for r in want]).tolist()
    assert score.tolist() == [r.score for r in want] and endA.tolist() == [r.endA for r in want]
    assert endB.tolist() == [r.endB for r in want] and err.tolist() == [r.err for r in want]
    check(case, capacity=1)                                      # the retry path returns the strings


# i. two threads on one scoring handle, each on its own host streams
def test_two_threads_on_one_handle(rb):
    ties = ao.tie_case()
    work = [ao.mixed_case(rb),                                   # both on ao.ACGT, so on one handle
            ao.Case("ties-on-ACGT", ao.ACGT, -4, -2, tuple(a.replace(b"B", b"C") for a in ties.A),
                    tuple(b.replace(b"B", b"C") for b in ties.B), False)]
    assert work[0].mat is work[1].mat
    scoring(ao.ACGT).handle()
    ao.expect(work[0]), ao.expect(work[1])
    errors = []
    start = threading.Barrier(2)

    def body(case):
        try:
            start.wait()
            for _ in range(3):
                check(case)
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=body, args=(c,)) for c in work]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# j. a score beyond 16 bits
def test_score_beyond_int16():
    case = ao.range_case()
    check(case)
    assert run(case)[0].score == 300 * 127


def test_refused_and_empty_calls():
    sc = scoring(ao.S127)
    A, offA = _pack(["ACGT"])
    with pytest.raises(_lib.PolyhipError) as ei:                 # 127 * (4 + 2^24) >= 2^30
        align.sw_affine_packed(sc, -3, -1, A, offA, np.zeros(1 << 24, np.uint8), None)
    assert ei.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.PolyhipError) as ei:
        align.sw_affine_packed(sc, -3, -1, A, np.array([4, 0], np.uint64), A, None)
    assert ei.value.status == _lib.ERR_INVALID
    out = align.sw_affine_align_packed(sc, -3, -1, np.zeros(0, np.uint8), np.zeros(1, np.uint64), A, None)
    assert [len(x) for x in out] == [0] * 6 and align.sw_affine_last_info()["pairs"] == 0
