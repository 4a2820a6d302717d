"""search/bwt with mismatches without a GPU: the exported symbols and the binding table, the argument errors that are
decided before any device call, what the compiler made of the kernels (no scratch: the DFS stack lives in LDS), and the
conditions that make the inputs of tests/test_bwt_mismatch_gpu.py non-vacuous, asserted on the oracle."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bwt_mismatch_oracle as mo  # noqa: E402

from poly_amd import _lib, build  # noqa: E402

SYMBOLS = ("polyhip_bwt_count_mismatch", "polyhip_bwt_locate_mismatch", "polyhip_bwt_mismatch_last_info")


def test_symbols_are_exported_and_bound():
    L = C.CDLL(build.build_lib())
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.lib().polyhip_abi_version() == 1
    header = open(os.path.join(build.ROOT, "include", "polyhip.h")).read()
    assert re.search(r"#define\s+POLYHIP_BWT_MAX_MISMATCHES\s+4u", header)
    assert re.search(r"#define\s+POLYHIP_ABI_VERSION\s+1\b", header)


def test_argument_errors_need_no_device():
    L = _lib.lib()
    pat, off = np.frombuffer(b"ACGT", np.uint8), np.array([0, 4], np.uint64)
    counts, err, first = np.zeros(6, np.uint32), np.zeros(1, np.uint32), np.zeros(2, np.uint64)
    pos, mm = np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    # k > 4 is decided first, before the handle is looked at
    assert L.polyhip_bwt_count_mismatch(None, pat.ctypes.data, off.ctypes.data, 1, 5, counts.ctypes.data, err.ctypes.data) \
        == _lib.ERR_UNSUPPORTED
    assert b"at most 4" in L.polyhip_last_error()
    assert L.polyhip_bwt_locate_mismatch(None, pat.ctypes.data, off.ctypes.data, 1, 5, first.ctypes.data, pos.ctypes.data,
                                         mm.ctypes.data, 4, err.ctypes.data) == _lib.ERR_UNSUPPORTED
    for k in range(5):
        assert L.polyhip_bwt_count_mismatch(None, pat.ctypes.data, off.ctypes.data, 1, k, counts.ctypes.data, err.ctypes.data) \
            == _lib.ERR_INVALID
        assert L.polyhip_bwt_locate_mismatch(None, pat.ctypes.data, off.ctypes.data, 1, k, first.ctypes.data, pos.ctypes.data,
                                             mm.ctypes.data, 4, err.ctypes.data) == _lib.ERR_INVALID
    assert L.polyhip_bwt_mismatch_last_info(None) == _lib.ERR_INVALID
    info = (C.c_uint64 * 5)()
    assert L.polyhip_bwt_mismatch_last_info(C.addressof(info)) == _lib.OK


# ---------------------------------------------------------------- kernel resources
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{(layout, emit): metadata} of every instantiation of the search kernel, and the locate helpers"""
    asm = str(tmp_path_factory.mktemp("bwtmm") / "bwt_mismatch.s")
    flags = [f for f in build.CXXFLAGS if f != "-fPIC"]
    res = subprocess.run([build._hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(build.CSRC, "bwt_mismatch.hip"),
                                                     "-o", asm], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = {}
    for block in re.split(r"\n\s+- \.", open(asm).read().split("amdhsa.kernels:", 1)[1]):
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
                                  for key in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return out


def test_search_and_locate_kernels_have_no_scratch(kernels):
    search = {n: m for n, m in kernels.items() if "mismatch_kernel" in n}
    assert len(search) == 4, sorted(kernels)            # two layouts x (count, locate)
    helpers = {n: m for n, m in kernels.items() if "mismatch_totals_kernel" in n or "mismatch_unpack_kernel" in n}
    assert len(helpers) == 2, sorted(kernels)
    for name, m in kernels.items():                     # the scans and the radix sort the locate step runs, too
        assert m["private_segment_fixed_size"] == 0, (name, m)


# ---------------------------------------------------------------- the oracle, and what the GPU inputs must exercise
def test_oracle_on_hand_checked_cases():
    assert mo.distances("banana", "ana").tolist() == [3, 0, 3, 0]
    pos, mm = mo.hits("banana", "ana", 0)
    assert pos.tolist() == [1, 3] and mm.tolist() == [0, 0]
    pos, mm = mo.hits("banana", "bnn", 1)
    assert pos.tolist() == [0] and mm.tolist() == [1]
    assert mo.hits("banana", "a$", 0)[0].size == 0                  # never cyclic through the '$'
    assert mo.hits("banana", "a$", 1)[0].tolist() == [1, 3]         # '$' always costs one mismatch (an, an; not at 5: a + end)
    assert mo.hits("banana", "bananas", 4)[0].size == 0             # m > n
    assert mo.hits("A" * 1000, "CCCC", 4)[1].tolist() == [4] * 997
    counts, first, pos, mm = mo.Case("banana", ["ana", "x", "nan"]).expect(1)
    assert counts.tolist() == [[2, 0], [0, 6], [1, 1]] and first.tolist() == [0, 2, 8, 10]
    assert pos.tolist() == [1, 3, 0, 1, 2, 3, 4, 5, 0, 2] and mm.tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 1, 0]


def test_tiny_inputs_cover_every_pattern_and_the_long_ones():
    for name, text in mo.tiny_texts().items():
        case = mo.tiny_case(name)
        n = len(text)
        assert len(case.pats) == 6 + 36 + 216 + 1296 + 8
        assert {n, n + 1, 2 * n} <= {len(p) for p in case.pats}
        assert any("$" in p for p in case.pats) and any("N" in p for p in case.pats)
        assert case.expect(4)[1][-1] > case.expect(0)[1][-1] > 0


def test_boundary_inputs_hold_the_ends_of_the_text():
    for n in mo.BOUNDARY_N:
        for leading_a in (0, 1):
            case = mo.boundary_case(n, leading_a)
            assert len(case.seq) == n and len(case.pats) == 250
            assert case.pats[0] == case.seq[:8] and case.dist[0][0] == 0        # cut at position 0, no substitution
            assert case.dist[1][n - 8] == 1                                     # cut at n - 8, one substitution
            assert bool(leading_a) == case.seq.startswith(b"A" * 40)
            counts = case.expect(3)[0]
            assert (counts.sum(axis=0) > 0).all()


def test_at_size_inputs_are_not_vacuous():
    case = mo.at_size_case()
    assert len(case.seq) == 100_003 and len(case.pats) == 500 and all(len(p) == 20 for p in case.pats)
    assert case.dist[0][0] == 0 and case.dist[1][100_003 - 20] == 1
    counts, first, pos, mm = case.expect(4)
    per = np.diff(first.astype(np.int64))
    assert (counts.sum(axis=0) > 0).all(), counts.sum(axis=0)       # every distance class 0..4
    assert (per >= 2).sum() >= 10 and (per == 0).sum() >= 50
    sort_case = mo.at_size_sort_case()
    counts, first, pos, mm = sort_case.expect(3)
    assert 5_000 <= int(first[-1]) <= 50_000 and np.diff(first.astype(np.int64)).max() >= 20


def test_general_and_degenerate_inputs_are_not_vacuous():
    assert len(set(mo.protein_case().seq)) == 20 and mo.protein_case().expect(2)[0].sum(axis=0).min() > 0
    by = mo.bytes_case()
    assert len(set(by.seq)) == 255 and ord("$") not in set(by.seq) and len(by.pats) == 100
    assert any(0 in p for p in by.pats) and any(max(p) >= 0x80 for p in by.pats)
    assert by.expect(1)[0].sum(axis=0).min() > 0
    assert len(set(mo.seven_case().seq)) == 7 and len(mo.seven_case().seq) == 1000
    counts, first, pos, mm = mo.wide_case().expect(2)
    assert int(first[-1]) == 9_999 and counts.min() > 500           # three leaves classes, each hundreds of rows wide
    ex = mo.exact_case()
    assert len(ex.pats) == 1000 and all(b"$" not in p and 1 <= len(p) <= len(ex.seq) for p in ex.pats)
