"""search/bwt with up to k mismatches on the GPU against the brute-force oracle (tests/bwt_mismatch_oracle.py).  Every
test runs in both occurrence layouts ("auto": nucleotide for <= 4 distinct bytes; "general": POLYHIP_BWT_GENERAL=1 forces
the byte layout on DNA too), compares counts, first, pos and mm exactly, and the count call with the locate call."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bwt_mismatch_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["auto", "general"])
def layout(request, monkeypatch):
    if request.param == "general":
        monkeypatch.setenv("POLYHIP_BWT_GENERAL", "1")
    else:
        monkeypatch.delenv("POLYHIP_BWT_GENERAL", raising=False)
    return request.param


def _new(seq, layout):
    from poly_amd import bwt
    idx = bwt.New(seq)
    distinct = len(set(seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)))
    assert idx.Layout() == ("nucleotide" if layout == "auto" and distinct <= 4 else "general")
    return idx


def _check(idx, case, k):
    """count and locate of the whole case at k == the oracle, and each other; returns (first, info)"""
    want_counts, want_first, want_pos, want_mm = case.expect(k)
    counts = idx.CountMismatchBatch(case.pats, k)
    assert counts.dtype == np.int64 and counts.shape == (len(case.pats), k + 1)
    assert (counts == want_counts).all(), ("counts", k, np.argwhere(counts != want_counts)[:5])
    first, pos, mm = idx.LocateMismatchBatch(case.pats, k)
    assert first.dtype == np.uint64 and pos.dtype == np.uint32 and mm.dtype == np.uint8
    assert (first == want_first).all(), ("first", k)
    assert (pos == want_pos).all(), ("pos", k, np.flatnonzero(pos != want_pos)[:5])
    assert (mm == want_mm).all(), ("mm", k, np.flatnonzero(mm != want_mm)[:5])
    # the count call against the locate call
    owner = np.repeat(np.arange(len(case.pats)), np.diff(first.astype(np.int64)))
    again = np.zeros_like(counts)
    np.add.at(again, (owner, mm.astype(np.int64)), 1)
    assert (again == counts).all()
    info = idx.MismatchInfo()
    assert info["patterns"] == len(case.pats) and info["hits"] == int(first[-1])
    assert info["leaves"] <= info["nodes"]
    if idx.Layout() == "nucleotide":
        assert info["occ_lines"] <= 2 * info["nodes"]      # one line per interval end serves all four children
        expanded = info["nodes"] - info["leaves"]           # nodes counts the leaves too; only expansions read lines
        assert expanded <= info["occ_lines"] <= 2 * expanded
    return first, info


# ---------------------------------------------------------------- 1. exhaustive, tiny
@pytest.mark.parametrize("name", ["banana", "A", "AC", "ACGTx3", "dna7", "dna31"])
def test_every_short_pattern_on_tiny_texts(layout, name):
    case = mo.tiny_case(name)
    idx = _new(case.seq, layout)
    for k in range(5):
        _check(idx, case, k)


# ---------------------------------------------------------------- 2. line and checkpoint boundaries
@pytest.mark.parametrize("leading_a", [0, 1])
@pytest.mark.parametrize("n", mo.BOUNDARY_N)
def test_line_and_checkpoint_boundaries(layout, n, leading_a):
    case = mo.boundary_case(n, leading_a)
    idx = _new(case.seq, layout)
    for k in range(4):
        _check(idx, case, k)


# ---------------------------------------------------------------- 3. at size
@pytest.fixture(scope="module")
def at_size_indexes():
    made = {}

    def get(layout):
        if layout not in made:
            made[layout] = _new(mo.at_size_text(), layout)
        return made[layout]
    return get


def test_at_size_20mers_k4(layout, at_size_indexes):
    _check(at_size_indexes(layout), mo.at_size_case(), 4)


def test_at_size_12mers_k3_sorts_tens_of_hits_per_pattern(layout, at_size_indexes):
    first, _ = _check(at_size_indexes(layout), mo.at_size_sort_case(), 3)
    assert int(first[-1]) >= 5_000


# ---------------------------------------------------------------- 4. general alphabets
def test_protein_text(layout):
    case = mo.protein_case()
    _check(_new(case.seq, layout), case, 2)


def test_text_over_every_byte_but_the_null_char(layout):
    case = mo.bytes_case()
    idx = _new(case.seq, layout)
    _check(idx, case, 1)
    _check(idx, case, 0)


def test_seven_symbol_text(layout):
    case = mo.seven_case()
    idx = _new(case.seq, layout)
    for k in range(5):
        _check(idx, case, k)


# ---------------------------------------------------------------- 5. degenerate
def test_one_symbol_text(layout):
    idx = _new("A" * 1000, layout)
    for k in range(5):
        assert idx.CountMismatch("AAAA", k).tolist() == [997] + [0] * k
    assert idx.CountMismatch("AACA", 0).tolist() == [0]
    assert idx.CountMismatch("AACA", 1).tolist() == [0, 997]
    assert idx.CountMismatch("CCCC", 3).tolist() == [0, 0, 0, 0]
    assert idx.CountMismatch("CCCC", 4).tolist() == [0, 0, 0, 0, 997]
    assert idx.LocateMismatch("CCCC", 3) is None
    assert idx.LocateMismatch("CCCC", 4) == [(p, 4) for p in range(997)]
    assert idx.LocateMismatch("AACA", 1) == [(p, 1) for p in range(997)]
    case = mo.Case("A" * 1000, ["AAAA", "AACA", "CCCC", "A", "C", "A" * 1000, "A" * 999 + "C", "A" * 1001])
    for k in range(5):
        _check(idx, case, k)


def test_periodic_text(layout):
    text = "ACGT" * 250
    case = mo.Case(text, ["ACGT", "CGTA", "AAAA", "ACGTACGTAC", "TGCA", "ACGTTCGTACGA", "G", "GT", text[:999], "ACGA" * 10])
    idx = _new(text, layout)
    for k in range(5):
        _check(idx, case, k)


def test_wide_leaf_intervals(layout):
    case = mo.wide_case()
    first, info = _check(_new(case.seq, layout), case, 2)
    assert int(first[-1]) == 9_999 and info["leaves"] == 16      # every 2-mer is a leaf, thousands of rows between them


def test_empty_pattern_inside_a_batch(layout):
    from poly_amd.mash import _pack
    text = mo.tiny_texts()["dna31"]
    idx = _new(text, layout)
    pats = [text[3:9], "", text[10:14]]
    want = mo.Case(text, pats).expect(2)
    counts, err = idx.count_mismatch_packed(*_pack(pats), 2)
    assert err.tolist() == [0, 1, 0] and (counts == want[0]).all() and counts[1].tolist() == [0, 0, 0]
    first, pos, mm, err = idx.locate_mismatch_packed(*_pack(pats), 2)
    assert err.tolist() == [0, 1, 0] and (first == want[1]).all() and (pos == want[2]).all() and (mm == want[3]).all()
    assert first[1] == first[2]
    for call in (idx.CountMismatchBatch, idx.LocateMismatchBatch):
        with pytest.raises(ValueError, match="Pattern can not be empty"):
            call(pats, 2)
    for call in (idx.CountMismatch, idx.LocateMismatch):
        with pytest.raises(ValueError, match="Pattern can not be empty"):
            call("", 2)


# ---------------------------------------------------------------- 6. capacity
def test_capacity(layout):
    from poly_amd import _lib
    from poly_amd.mash import _pack
    case = mo.boundary_case(449, 0)
    idx = _new(case.seq, layout)
    _, want_first, want_pos, want_mm = case.expect(2)
    total = int(want_first[-1])
    buf, offs = _pack(case.pats)
    n = len(case.pats)
    L = _lib.lib()

    def call(capacity, npat=n):
        first = np.full(n + 1, 2 ** 64 - 1, np.uint64)
        pos, mm, err = np.full(total + 1, 0xDEADBEEF, np.uint32), np.full(total + 1, 0xEE, np.uint8), np.zeros(n, np.uint32)
        status = L.polyhip_bwt_locate_mismatch(idx.handle(), buf.ctypes.data, offs.ctypes.data, npat, 2, first.ctypes.data,
                                               pos.ctypes.data, mm.ctypes.data, capacity, err.ctypes.data)
        return status, first, pos, mm

    status, first, pos, mm = call(total - 1)
    assert status == _lib.ERR_INVALID and str(total) in L.polyhip_last_error().decode()
    assert (first == want_first).all() and (pos == 0xDEADBEEF).all() and (mm == 0xEE).all()
    status, first, pos, mm = call(total)
    assert status == _lib.OK and (first == want_first).all()
    assert (pos[:total] == want_pos).all() and (mm[:total] == want_mm).all() and pos[total] == 0xDEADBEEF and mm[total] == 0xEE
    status, first, pos, mm = call(0, npat=0)
    assert status == _lib.OK and first[0] == 0 and (pos == 0xDEADBEEF).all()
    with pytest.raises(_lib.PolyhipError) as ei:
        idx.LocateMismatchBatch(case.pats, 2, capacity=total - 1)
    assert ei.value.status == _lib.ERR_INVALID and str(total) in ei.value.message
    assert idx.CountMismatchBatch([], 2).shape == (0, 3)
    with pytest.raises(_lib.PolyhipError) as ei:
        idx.CountMismatchBatch(case.pats, 5)
    assert ei.value.status == _lib.ERR_UNSUPPORTED


# ---------------------------------------------------------------- 7. agreement with the exact path
def test_k0_agrees_with_count_and_locate(layout):
    case = mo.exact_case()
    idx = _new(case.seq, layout)
    assert (idx.CountMismatchBatch(case.pats, 0)[:, 0] == idx.CountBatch(case.pats)).all()
    first, pos, mm = idx.LocateMismatchBatch(case.pats, 0)
    efirst, eout = idx.LocateBatch(case.pats)
    assert (first == efirst).all() and not mm.any()
    for p in range(len(case.pats)):
        a, b = int(first[p]), int(first[p + 1])
        assert (pos[a:b] == np.sort(eout[a:b])).all(), p
    _check(idx, case, 0)
    ban = _new("banana", layout)
    assert ban.Count("a$") == 1                               # the exact Count is cyclic through the '$' ...
    assert ban.CountMismatch("a$", 0).tolist() == [0]         # ... the search with mismatches never is
    assert ban.LocateMismatch("a$", 0) is None and ban.LocateMismatch("a$", 1) == [(1, 1), (3, 1)]
