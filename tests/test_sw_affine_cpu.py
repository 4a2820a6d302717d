"""Smith-Waterman with affine gaps without a GPU: the oracle (tests/sw_affine_oracle.py) on known answers and against the
linear oracle, the conditions that make the inputs of tests/test_sw_affine_gpu.py non-vacuous, the exported symbols and
the argument errors that are decided before any device call, and what the compiler made of the kernels (no scratch)."""
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
import sw_affine_oracle as ao  # noqa: E402

import oracle  # noqa: E402
from poly_amd import _lib, build  # noqa: E402

SYMBOLS = ("polyhip_sw_affine_batch", "polyhip_sw_affine_align_batch_packed", "polyhip_sw_affine_last_info")


# ---------------------------------------------------------------- the oracle
def test_known_answers():
    for A, B, match, mismatch, go, ge, score, alignA, alignB, endA, endB in ao.KNOWN:
        res = ao.align(A, B, ao.simple("ACGT", match, mismatch), go, ge)
        assert res == (score, endA, endB, 0, alignA.encode(), alignB.encode()), (A, B, res)
    # why the feature exists: the linear model cannot keep the 8-base deletion together
    A, B = ao.KNOWN[0][:2]
    assert oracle.smith_waterman(A, B, ao.simple("ACGT", 2, -3).reference(), -5)[0] == 16


def test_equal_open_and_extend_is_the_linear_smith_waterman():
    rng = np.random.default_rng(31)
    n = 0
    for letters in ("AB", "ABC", "ACGT"):
        for _ in range(400):
            match, mismatch, gap = int(rng.integers(1, 6)), -int(rng.integers(0, 6)), -int(rng.integers(1, 8))
            mat = ao.simple(letters, match, mismatch)
            a = ao._rand(rng, letters, int(rng.integers(0, 30)))
            b = ao._rand(rng, letters, int(rng.integers(0, 30)))
            res = ao.align(a, b, mat, gap, gap)
            score, sa, sb, ea, eb = oracle.smith_waterman(a, b, mat.reference(), gap)
            assert (res.score, res.endA, res.endB, res.alignA.decode(), res.alignB.decode()) == (score, ea, eb, sa, sb), (a, b, gap)
            n += 1
    assert n >= 1000


def test_error_order_is_the_linear_one():
    mat = ao.ACGT
    for a, b in ((b"xCGT", b"AyGT"), (b"ACGx", b"AyGT"), (b"ACxT", b"ACGT"), (b"", b"yy"), (b"xx", b"")):
        res = ao.align(a, b, mat, -3, -1)
        try:
            oracle.smith_waterman(a, b, mat.reference(), -3)
            want = 0
        except oracle.AlphabetError as e:
            want = (e.side << 8) | e.symbol
        assert res.err == want and (not want or res == (0, 0, 0, want, b"", b"")), (a, b, res, want)


def test_every_gpu_case_rescores_and_fits_its_window():
    rb = ao.rows_per_band()
    n = exact = clipped = 0
    for case in ao.gpu_cases(rb):
        for p, res in enumerate(ao.expect(case)):
            if res.score == 0:
                assert res[1:] == (0, 0, res.err, b"", b"")
                continue
            assert ao.rescore(res.alignA, res.alignB, case.mat, case.go, case.ge) == res.score, (case.name, p)
            W, cols, bound = ao.window(res, case.mat, case.ge)
            span = len(res.alignB) - res.alignB.count(b"-")          # columns of B the path covers
            assert span <= cols and len(res.alignA) <= bound, (case.name, p, span, W, bound)
            exact += span == W
            clipped += W > res.endB and span == res.endB
            n += 1
    assert n > 700 and exact >= 10 and clipped >= 10, (n, exact, clipped)


def test_band_and_mixed_inputs_hold_their_shapes():
    rb = ao.rows_per_band()
    assert rb >= 8 and rb % 8 == 0
    pairs = [c for c in ao.band_cases(rb) if not c.shared]
    assert len(pairs) == 2
    for c in pairs:
        assert {len(a) for a in c.A} == {rb - 1, rb, rb + 1, 2 * rb, 2 * rb + 1, 1}
        assert {len(b) for b in c.B} == {1, 2, 63, 64, 65}
    assert sorted(len(c.B) for c in ao.band_cases(rb) if c.shared) == sorted([1, 2, 63, 64, 65] * 2)
    mixed = ao.mixed_case(rb)
    lens = [len(a) for a in mixed.A]
    assert len(mixed.A) == 300 and max(lens) == 3 * rb and lens.count(0) >= 3 and sum(len(b) == 0 for b in mixed.B) >= 3
    assert sum(abs(lens[i] - lens[i + 1]) > rb for i in range(63)) >= 10          # neighbouring lanes differ
    errs = [r.err for r in ao.expect(mixed)]
    first_a = [p for p, e in enumerate(errs) if e == (1 << 8) | ord("x") and mixed.A[p][0] == ord("x")]
    then_b = [p for p, e in enumerate(errs) if e == (2 << 8) | ord("y") and mixed.A[p][-1] == ord("x")]
    later_a = [p for p, e in enumerate(errs) if e == (1 << 8) | ord("z")]
    assert first_a and then_b and later_a and min(map(min, (first_a, then_b, later_a))) < 63


def test_tie_inputs_meet_every_tie_rule():
    case = ao.tie_case()
    assert case.go == 2 * case.ge
    seen = {}
    for a, b in zip(case.A, case.B):
        for cond in ao.tie_conditions(a, b, case.mat, case.go, case.ge):
            seen[cond] = seen.get(cond, 0) + 1
    assert set(seen) == {"max-twice", "diag-and-F", "F-and-E", "open-and-extend"} and min(seen.values()) >= 3, seen


def test_gap_inputs_keep_their_inserts_together():
    wide, narrow = ao.gap_cases()
    assert (wide.ge, wide.mat.smax, narrow.ge) == (-1, 5, -4)
    for case in (wide, narrow):
        runs = set()
        for res in ao.expect(case)[:40]:
            for s in (res.alignA, res.alignB):
                runs |= {len(r) for r in re.findall(rb"-+", s)}
        assert len(runs & set(range(1, 41))) >= (30 if case is wide else 8), (case.name, sorted(runs))
    assert max(ao.window(r, wide.mat, wide.ge)[1] - r.endA for r in ao.expect(wide)) >= 40


def test_table_and_range_inputs():
    big, shared, asym = ao.table_cases()
    assert (len(big.mat.first) + 1) * (len(big.mat.second) + 1) * 4 + 512 > 60 * 1024            # table_fits is false
    assert (len(asym.mat.first) + 1) * (len(asym.mat.second) + 1) * 4 + 512 <= 60 * 1024
    assert asym.mat.first != asym.mat.second and any(r.err for r in ao.expect(big))
    res = ao.expect(ao.range_case())
    assert res[0].score == 300 * 127 > 32767 and res[1].score > 32767 and b"-" in res[1].alignA


# ---------------------------------------------------------------- the ABI
def test_symbols_are_exported_and_bound():
    L = C.CDLL(build.build_lib())
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    assert _lib.lib().polyhip_abi_version() == 1
    header = open(os.path.join(build.ROOT, "include", "polyhip.h")).read()
    assert re.search(r"#define\s+POLYHIP_ABI_VERSION\s+1\b", header)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert "polyhip_stream_t" not in "".join(re.findall(r"polyhip_sw_affine\w*\s*\([^;]*;", header))


def test_gap_errors_need_no_device():
    L = _lib.lib()
    seq, off = np.frombuffer(b"ACGT", np.uint8), np.array([0, 4], np.uint64)
    score, ends, err = np.zeros(1, np.int64), np.zeros(2, np.uint32), np.zeros(1, np.uint32)
    aln, aoff = np.zeros(16, np.uint8), np.zeros(2, np.uint64)

    def both(go, ge):
        return (L.polyhip_sw_affine_batch(None, go, ge, seq.ctypes.data, off.ctypes.data, 1, seq.ctypes.data, None, 4,
                                          score.ctypes.data, ends.ctypes.data, ends[1:].ctypes.data, err.ctypes.data),
                L.polyhip_sw_affine_align_batch_packed(None, go, ge, seq.ctypes.data, off.ctypes.data, 1, seq.ctypes.data, None, 4,
                                                       score.ctypes.data, ends.ctypes.data, ends[1:].ctypes.data, err.ctypes.data,
                                                       aln.ctypes.data, aln[8:].ctypes.data, aoff.ctypes.data, 8))
    # the gap check comes first, before the handle is looked at
    assert both(-1, -2) == (_lib.ERR_UNSUPPORTED,) * 2            # go > ge
    assert b"gap_open <= gap_extend <= -1" in L.polyhip_last_error()
    assert both(-3, 0) == (_lib.ERR_UNSUPPORTED,) * 2             # ge = 0
    assert both(2, 3) == (_lib.ERR_UNSUPPORTED,) * 2
    assert both(-3, -1) == (_lib.ERR_INVALID,) * 2                # gaps in range: the NULL handle is what is wrong
    assert both(-2, -2) == (_lib.ERR_INVALID,) * 2
    assert L.polyhip_sw_affine_last_info(None) == _lib.ERR_INVALID
    info = (C.c_uint64 * 6)()
    assert L.polyhip_sw_affine_last_info(C.addressof(info)) == _lib.OK


# ---------------------------------------------------------------- kernel resources
@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel: metadata} of every kernel in sw_affine.hip"""
    asm = str(tmp_path_factory.mktemp("swa") / "sw_affine.s")
    flags = [f for f in build.CXXFLAGS if f != "-fPIC"]
    res = subprocess.run([build._hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(build.CSRC, "sw_affine.hip"),
                                                     "-o", asm], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = {}
    for block in re.split(r"\n\s+- \.", open(asm).read().split("amdhsa.kernels:", 1)[1]):
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
                                  for key in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return out


def test_kernels_have_no_scratch(kernels):
    swa = {n: m for n, m in kernels.items() if "swa_kernel" in n}
    assert len(swa) == 6, sorted(kernels)       # score pass: (LDS, global) x (shared, per-pair B); traceback: (LDS, global)
    assert len(kernels) == len(swa), sorted(kernels)
    for name, m in kernels.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
