"""polyhip_trim_reads and polyhip_trim_pairs without a GPU: the oracle (tests/trim_oracle.py) against answers written out by hand
for each rule of the definition, what the hand-built inputs (tests/trim_inputs.py) hold, the declarations, the argument errors
in their documented order (they are all decided before any device call), and the share of planted inserts the definition
recovers."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import trim_inputs as ti  # noqa: E402
import trim_oracle as to  # noqa: E402

A = ti.ADAPTER
TC = b"TCCTTCTCCTCTTTCCTCTCCTTCCCTTTCTCTCCTTTCTTCCTCTTCCTTCTCCCTTCT"      # 60 bytes without A or G: nothing in it starts the adapter


def _ends(Q, c5=0, c3=0):
    return to.quality_ends(ti.phred(Q), 33, c5, c3, len(Q))


# ---------------------------------------------------------------- 1. the oracle against answers worked out by hand
def test_oracle_quality_walk_by_hand():
    # the sum goes 10, -10: the walk ends there although 0, 10, 20 would follow
    assert to.walk([10, 40, 10, 10, 10], 20) == 1
    assert _ends([10, 10, 10, 40, 10], c3=20) == (0, 4, 1) and _ends([10, 40, 10, 10, 10], c5=20) == (1, 5, 2)
    # ties of the greatest sum: 10, 10, 10, 0 and 10, 0, 10 -- the first holder stays
    assert to.walk([10, 20, 20, 30], 20) == 1 and to.walk([10, 30, 10], 20) == 1
    assert _ends([10, 30, 10], c3=20) == (0, 2, 1) and _ends([10, 30, 10], c5=20) == (1, 3, 2)
    # a sum that stays >= 0 walks on over a good base: 15, 30, 20, 35
    assert to.walk([5, 5, 30, 5], 20) == 4
    # all below: everything goes, and an emptied read is 0, 0 with bit 0; all above, and all equal to the cut-off: nothing goes
    assert _ends([5] * 4, c3=20) == (0, 0, 1) and _ends([5] * 4, c5=20) == (0, 0, 1) and _ends([5] * 4, 20, 20) == (0, 0, 1)
    assert _ends([30] * 4, 20, 20) == (0, 4, 0) and _ends([20] * 4, 20, 20) == (0, 4, 0) and _ends([], 20, 20) == (0, 0, 0)
    # both ends: 3' 15, -5 -> b = 5; 5' 15, 30, 10, -10 -> a = 2
    assert _ends([5, 5, 40, 40, 40, 5], 20, 20) == (2, 5, 3)
    # a >= b: each walk on the read as it came takes all of it (a = 7, b = 0)
    assert _ends([5, 5, 5, 25, 5, 5, 5], 20, 20) == (0, 0, 1)
    # a = b exactly: 5' takes 2 (15, 30, -10), 3' takes 2 (15, 30, -10 ...) of four
    assert _ends([5, 5, 5, 5], 20, 0) == (0, 0, 1) and _ends([5, 5, 60, 60, 5, 5], 20, 20) == (2, 4, 3)
    # cut-off 0 is off whatever the qualities
    assert _ends([0] * 5) == (0, 5, 0)
    # judging: length first, then the range; nothing else is looked at
    assert to.judge(3, None, 33) == 0 and to.judge(3, b"II", 33) == 1 and to.judge(3, b"I I", 33) == 2 and to.judge(3, b"I\x7fI", 33) == 2
    assert to.judge(3, b"!~I", 33) == 0 and to.judge(2, b" ", 33) == 1
    r = to.trim_reads([A + b"ACGT"], [ti.phred([2] * 36) + b" "], [A], min_qual_3p=20, min_len=10)
    assert (r.start[0], r.end[0], r.flags[0], r.err[0]) == (0, 0, 0, 2) and r.offsets.tolist() == [0, 0] and r.info["bad"] == 1 and r.info["too_short"] == 0


def _hit(read, adapters, **kw):
    r = to.trim_reads([read], None, adapters, **kw)
    return (int(r.end[0]), int(r.flags[0]) >> 8) if r.flags[0] & to.F_ADAPTER else None


def test_oracle_adapters_by_hand():
    # budgets with 10 %: 100 * mism <= 10 * L
    for L, x, want in ((9, 0, True), (9, 1, False), (10, 1, True), (10, 2, False), (19, 1, True), (19, 2, False), (20, 2, True), (20, 3, False)):
        read = TC + ti.spoil(A[:L], range(1, 1 + 3 * x, 3))
        assert (_hit(read, [A], min_overlap=9, adapter_err_pct=10) == (60, 0)) == want, (L, x)
    # s = b - min_overlap hits; s = b - min_overlap + 1 has one byte too few
    assert _hit(TC + A[:5], [A], min_overlap=5) == (60, 0) and _hit(TC + A[:4], [A], min_overlap=5) is None
    assert _hit(TC + A[:5], [A], min_overlap=6) is None
    # a whole adapter anywhere, and the smallest s wins over a later, better one
    assert _hit(TC + A + TC, [A]) == (60, 0) and _hit(TC + ti.spoil(A, (3, 30)) + A, [A]) == (60, 0)
    # two adapters tying at one s: the lowest index, whichever it is
    x, y = b"ACGTACGTTT", b"ACGTACGTGG"
    assert _hit(TC + b"ACGTACGT", [x, y]) == (60, 0) and _hit(TC + b"ACGTACGT", [y, x]) == (60, 0)
    assert _hit(TC + b"ACGTACGTGG", [x, y], adapter_err_pct=0) == (60, 1)
    # ... but a smaller s of a later adapter beats a larger s of an earlier one
    assert _hit(TC + b"GGACGTACGTTT", [x, b"GGACG"], adapter_err_pct=0) == (60, 1)
    # lower case matches, N (and n) is a mismatch: one of ten
    assert _hit(TC + b"agatNggaag", [A], min_overlap=10, adapter_err_pct=10) == (60, 0)
    assert _hit(TC + b"agatNggaag", [A], min_overlap=10, adapter_err_pct=9) is None and _hit(TC + b"agatcggaag", [A], adapter_err_pct=0) == (60, 0)
    # a hit at s = 0: an empty read, which min_len > 0 then flags
    r = to.trim_reads([A + TC], None, [A], min_len=1)
    assert (r.start[0], r.end[0], r.flags[0]) == (0, 0, to.F_ADAPTER | to.F_SHORT) and r.info["too_short"] == 1 and len(r.seqs) == 0
    # the search runs on r[a, b): an adapter inside a quality-cut tail is not found, one before it is, with L up to the new b
    q = ti.phred([35] * 60 + [2] * 33)
    r = to.trim_reads([TC + A], [q], [A], min_qual_3p=20)
    assert (r.end[0], r.flags[0]) == (60, to.F_QUAL_3P)
    q = ti.phred([35] * 70 + [2] * 23)
    r = to.trim_reads([TC + A], [q], [A], min_qual_3p=20)
    assert (r.end[0], r.flags[0]) == (60, to.F_QUAL_3P | to.F_ADAPTER)
    # min_len at b - a and b - a + 1; the output keeps the bytes as they were
    r = to.trim_reads([b"acgtn" * 4 + A], None, [A], min_len=20)
    assert r.seqs.tobytes() == b"acgtn" * 4 and r.flags[0] == to.F_ADAPTER
    r = to.trim_reads([b"acgtn" * 4 + A], None, [A], min_len=21)
    assert len(r.seqs) == 0 and r.flags[0] == to.F_ADAPTER | to.F_SHORT and (r.start[0], r.end[0]) == (0, 20)


def test_oracle_pairs_by_hand():
    s = ti.pairs()
    rep1, rep2 = s.reads1[7], s.reads2[7]
    # the tandem repeat: inserts 40 and 64 both qualify without a mismatch, the greatest wins
    assert to.find_insert(rep1[:40], rep2[:40], 40, 0) == 40 and to.find_insert(rep1[:64], rep2[:64], 64, 0) == 64
    assert to.find_insert(rep1, rep2, 20, 0) == 64
    assert to.find_insert(b"ACGTT", b"AACGT", 5, 0) == 5 and to.find_insert(b"ACGTT", b"AACGT", 6, 0) is None
    assert to.find_insert(b"ACGTTGG", b"AACGTCC", 3, 0) == 5                # 7 and 6 do not qualify
    # N never pairs, not even with N: position 2 of both is one mismatch of five
    assert to.find_insert(b"ACNTT", b"AANGT", 5, 19) is None and to.find_insert(b"ACNTT", b"AANGT", 5, 20) == 5
    assert to.find_insert(b"acgtt", b"aacgt", 5, 0) == 5
    r = to.trim_pairs(s.reads1, s.reads2, s.quals1, s.quals2, [], **s.modes[0])
    ends = [(int(r.end[2 * i]), int(r.end[2 * i + 1])) for i in range(len(s.reads1))]
    assert ends[:5] == [(20, 20), (100, 100), (100, 100), (60, 60), (45, 45)] and ends[7] == (64, 64) and ends[8] == (70, 70)
    ov = [(int(r.flags[2 * i]) >> 4 & 1, int(r.flags[2 * i + 1]) >> 4 & 1) for i in range(len(s.reads1))]
    assert ov[:5] == [(1, 1), (0, 0), (0, 0), (1, 0), (1, 1)]
    assert r.err[10:14].tolist() == [0, 2, 1, 0] and ends[5] == (100, 0) and ends[6] == (0, 100) and ov[5] == ov[6] == (0, 0)
    # pair 9: a = 35 from the 5' quality cut, the insert is 30: the mate is emptied to 0, 0 and keeps bit 1
    assert (r.start[18], r.end[18], r.flags[18]) == (0, 0, to.F_QUAL_5P | to.F_OVERLAP) and (r.start[19], r.end[19]) == (0, 30)
    assert ends[10] == (0, 0) and r.info["overlap_cut"] == 11 and r.info["bad"] == 2
    # without a mismatch allowed pair 8 is left alone; with pair_min_overlap 0 nothing is looked for
    strict = to.trim_pairs(s.reads1, s.reads2, s.quals1, s.quals2, [], **s.modes[1])
    assert (strict.end[16], strict.end[17]) == (100, 100) and (strict.end[0], strict.end[1]) == (20, 20)
    assert to.trim_pairs(s.reads1, s.reads2, s.quals1, s.quals2, [], **s.modes[2]).info["overlap_cut"] == 0
    # an adapter hit on either mate switches step P off for the pair: every short insert is found by its adapter instead
    w = ti.pairs_with_adapters()
    r = to.trim_pairs(w.reads1, w.reads2, w.quals1, w.quals2, w.adapters, **w.modes[0])
    assert (r.end[0], r.end[1], r.flags[0], r.flags[1]) == (20, 20, to.F_ADAPTER, to.F_ADAPTER | 1 << 8)
    assert r.flags[14] & to.F_OVERLAP and not r.flags[14] & to.F_ADAPTER                         # the repeat has no adapter
    assert r.flags[6] == to.F_ADAPTER and r.flags[7] == 0 and (r.end[6], r.end[7]) == (60, 60)   # mate 2 is all insert: P is off


# ---------------------------------------------------------------- 2. what the hand-built inputs hold
def _run(s, mode):
    if hasattr(s, "reads1"):
        return to.trim_pairs(s.reads1, s.reads2, s.quals1, s.quals2, s.adapters, **mode)
    return to.trim_reads(s.reads, s.quals, s.adapters, **mode)


def test_inputs_hold_what_they_promise():
    names = [s.name for s in ti.single_sets() + ti.pair_sets()] + ["many_small"]
    assert len(names) == len(set(names))
    s = ti.lengths()
    assert sorted({len(r) for r in s.reads}) == list(ti.LENGTHS) and len(s.reads) == 30
    r = _run(s, s.modes[0])
    assert r.info["cut_3p"] > 10 and r.info["cut_5p"] > 10 and r.info["adapter_hits"] >= 12 and r.info["bad"] == 0
    assert r.flags[28] & to.F_ADAPTER and r.end[28] <= 5000 - 33 and _run(s, s.modes[3]).info["too_short"] > 8
    s = ti.adapter_lengths()
    assert tuple(len(a) for a in s.adapters) == ti.ADAPTER_LENGTHS
    r = _run(s, s.modes[2])                                               # 32 bytes at least, 10 %: only the three long adapters can hit
    assert [int(f) >> 8 for f in r.flags[6:15:3]] == [2, 3, 4] and r.end[6:15:3].tolist() == [40, 40, 40]           # whole, at 40
    assert r.end[7:15:3].tolist() == [166, 150, 150]                      # the first half at the end: 16, 32 and 32 bytes
    assert r.end[8:15:3].tolist() == [70, 70, 154]                        # 3 of 32 and 6 of 63 changed pass, 7 of 64 do not
    assert _run(s, s.modes[0]).info["adapter_hits"] == len(s.reads)       # one byte, no mismatch: every read holds it somewhere
    r = _run(s, s.modes[3])
    assert r.flags[12] == to.F_ADAPTER | 4 << 8 and r.end[12] == 0        # 64 bytes, any mismatches: the first start with 64 bytes of room
    s = ti.adapter_places()
    r = _run(s, s.modes[0])
    assert r.end.tolist() == [0, 50, 120, 70, 70, 30, 45, 90] and [int(f) >> 8 for f in r.flags] == [0, 0, 0, 0, 1, 0, 0, 0]
    assert r.start.tolist() == [0] * 7 + [20] and r.flags[7] == to.F_QUAL_5P | to.F_ADAPTER
    r = _run(s, s.modes[1])
    assert r.end[6] == len(s.reads[6]) and not r.flags[6] & to.F_ADAPTER   # the N and n count when no mismatch is allowed
    s = ti.budgets()
    r = _run(s, s.modes[0])
    assert [bool(f & to.F_ADAPTER) for f in r.flags] == s.hit == [True, False, True, False, True, False, True, False]
    assert all(e == 60 for e, h in zip(r.end, s.hit) if h)
    s = ti.many_adapters()
    r = _run(s, s.modes[0])
    assert len(s.adapters) == 255 and [int(f) >> 8 for f in r.flags[:40]] == s.which and s.which[3] == 254 and r.flags[40] == 0
    assert set(r.end[:40]) == {60}
    s = ti.quality_edges()
    r = _run(s, s.modes[0])
    k = len(s.cuts)
    assert r.end[0:2 * k:2].tolist() == [200 - c for c in s.cuts] and r.start[1:2 * k:2].tolist() == list(s.cuts)
    assert (r.end[2 * k], r.start[2 * k + 1]) == (120, 80) and (r.start[2 * k + 2], r.end[2 * k + 2], r.flags[2 * k + 2]) == (0, 0, 1)
    assert r.flags[2 * k + 3] == 0 and r.flags[2 * k + 4] == 0
    s = ti.errs()
    r = _run(s, s.modes[0])
    assert r.err.tolist() == [0, 1, 0, 1, 2, 0, 2, 1, 0, 0] and r.info["bad"] == 5 and r.flags[8] == to.F_ADAPTER and r.flags[9] == to.F_QUAL_3P | to.F_SHORT
    assert all(r.start[i] == r.end[i] == r.flags[i] == 0 for i in (1, 3, 4, 6, 7))
    s = ti.phred64()
    assert [_run(s, m).err.tolist() for m in s.modes] == [[0, 0, 0], [0, 0, 0], [2, 2, 2]]
    assert _run(s, s.modes[0]).end.tolist() == [22, 92, 142] and _run(s, s.modes[1]).end.tolist() == [30, 100, 150]   # Q 34 and 71 at 33
    s = ti.min_len_edges()
    a, b = _run(s, s.modes[0]), _run(s, s.modes[1])
    assert (a.end - a.start).tolist() == [40, 40, 40] and a.info["too_short"] == 0 and b.info["too_short"] == 3 and len(b.seqs) == 0
    assert np.diff(a.offsets.astype(np.int64)).tolist() == [40, 40, 40] and a.start.tolist() == b.start.tolist() == [0, 6, 0]
    s = ti.no_qual()
    r = _run(s, s.modes[0])
    assert r.quals is None and r.end.tolist() == [70, 72, 70, 70, 70, 0, 50]
    s = ti.pairs_no_qual()
    r = _run(s, s.modes[0])
    assert (r.end[-2], r.end[-1]) == (260, 260) and len(s.reads1[-1]) == 300 and len(s.reads2[-1]) == 280


def test_many_small_holds_what_it_promises():
    s = ti.many_small()
    r = _run(s, s.modes[0])
    assert len(s.reads) == 70_000 and r.info["adapter_hits"] > 3000 and r.info["cut_3p"] > 10_000 and r.info["too_short"] > 4000
    assert 0 < r.info["bytes_out"] < r.info["bytes_in"] == 350_000


# ---------------------------------------------------------------- 3. the declarations and the errors that need no device
def test_declarations():
    from poly_amd import _lib, trim
    assert len(_lib.SIGNATURES["polyhip_trim_reads"][1]) == 16 and len(_lib.SIGNATURES["polyhip_trim_pairs"][1]) == 23
    assert "polyhip_trim_last_info" in _lib.SIGNATURES
    assert C.sizeof(trim._CParams) == 32 and C.sizeof(trim._CInfo) == 72
    assert tuple(n for n, _ in trim._CInfo._fields_) == to.INFO_FIELDS
    assert tuple(n for n, _ in trim._CParams._fields_) == tuple(to.DEFAULTS)
    header = open(os.path.join(ROOT, "include", "polyhip.h")).read()
    assert "uint64_t reads, bytes_in, bytes_out, cut_3p, cut_5p, adapter_hits, overlap_cut, too_short, bad;" in header
    assert "#define POLYHIP_ABI_VERSION 1\n" in header
    for n in ("polyhip_trim_reads", "polyhip_trim_pairs", "polyhip_trim_last_info"):
        assert not n.endswith("_dev") and hasattr(_lib.lib(), n)
    assert (trim.FLAG_QUAL_3P, trim.FLAG_QUAL_5P, trim.FLAG_ADAPTER, trim.FLAG_SHORT, trim.FLAG_OVERLAP) == \
        (to.F_QUAL_3P, to.F_QUAL_5P, to.F_ADAPTER, to.F_SHORT, to.F_OVERLAP)
    for f in (trim.trim_packed, trim.trim_pairs_packed, trim.trim_fastq, trim.last_info):
        assert callable(f)


def test_argument_errors_without_gpu():
    """everything the header lists is decided before any device call, in the documented order: each case holds every later
    fault as well"""
    from poly_amd import _lib, trim
    L = _lib.lib()
    P = trim._CParams
    a32, out8 = np.zeros(4, np.uint32), np.zeros(64, np.uint8)
    up, down, o64 = np.array([0, 4, 8], np.uint64), np.array([0, 8, 4], np.uint64), np.zeros(3, np.uint64)
    huge = np.array([0, 1 << 24, (1 << 24) + 1], np.uint64)
    rd = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    ad = np.frombuffer(b"ACGTACGTA" + b"C" * 70, np.uint8).copy()
    good_ad, empty_ad, long_ad, lower_ad = (np.array(x, np.uint32) for x in ([0, 4], [4, 4], [9, 74], [0, 2]))
    lower = np.frombuffer(b"Ac", np.uint8).copy()
    p = lambda x: None if x is None else x.ctypes.data      # noqa: E731
    ok = P(33, 0, 0, 10, 3, 0, 0, 10)

    def call(params, adapters=ad, adoff=good_ad, nad=1, reads=rd, off=up, qual=None, qoff=None, n=2, start=a32, out=out8, oq=None, ooff=o64):
        rc = L.polyhip_trim_reads(None if params is None else C.byref(params), p(adapters), p(adoff), nad, p(reads), p(off), p(qual),
                                  p(qoff), n, p(start), a32.ctypes.data, a32.ctypes.data, a32.ctypes.data, p(out), p(oq), p(ooff))
        return rc, L.polyhip_last_error()

    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    worst = dict(nad=256, adoff=empty_ad, qoff=down, oq=out8, start=None, off=huge)       # every later fault at once
    cases = (
        (None, worst, INV, b"null params"),
        (P(163, 94, 94, 101, 0, 0, 0, 101), worst, INV, b"qual_offset"),
        (P(162, 94, 94, 101, 0, 0, 0, 101), worst, INV, b"min_qual_5p"),
        (P(162, 93, 94, 101, 0, 0, 0, 101), worst, INV, b"min_qual_3p"),
        (P(162, 93, 93, 101, 0, 0, 0, 101), worst, INV, b"adapter_err_pct"),
        (P(162, 93, 93, 100, 0, 0, 0, 101), worst, INV, b"min_overlap"),
        (P(162, 93, 93, 100, 1, 0, 0, 101), worst, INV, b"pair_err_pct"),
        (P(33, 20, 0, 100, 1, 0, 0, 100), worst, INV, b"256 adapters"),
        (P(33, 20, 0, 10, 1, 0, 0, 10), dict(worst, nad=1, adapters=None), INV, b"null adapters"),
        (P(33, 20, 0, 10, 1, 0, 0, 10), dict(worst, nad=1), INV, b"adapter 0 is empty"),
        (P(33, 20, 0, 10, 1, 0, 0, 10), dict(worst, nad=1, adoff=long_ad), INV, b"adapter 0 has 65 bytes"),
        (P(33, 20, 0, 10, 1, 0, 0, 10), dict(worst, nad=1, adapters=lower, adoff=lower_ad), INV, b"adapter 0 has byte 0x63 at 1"),
        (P(33, 20, 0, 10, 1, 0, 0, 10), dict(worst, nad=1, adoff=good_ad), INV, b"cut-off without qualities"),
        (P(33, 0, 20, 10, 1, 0, 0, 10), dict(worst, nad=1, adoff=good_ad), INV, b"cut-off without qualities"),
        (ok, dict(worst, nad=0, adapters=None, adoff=None), INV, b"qual and qual_off come together"),
        (ok, dict(worst, nad=0, qual=rd, qoff=None), INV, b"qual and qual_off come together"),
        (ok, dict(worst, nad=0, qoff=None), INV, b"out_qual is given exactly when qual is"),
        (ok, dict(worst, nad=0, qual=rd, oq=None), INV, b"out_qual is given exactly when qual is"),
        (ok, dict(worst, nad=0, qoff=None, oq=None), INV, b"null argument"),
        (ok, dict(nad=0, out=None, off=huge), INV, b"null argument"),
        (ok, dict(nad=0, ooff=None, off=huge), INV, b"null argument"),
        (ok, dict(nad=0, reads=None, off=huge), INV, b"null argument"),
        (ok, dict(nad=0, off=None), INV, b"null argument"),
        (ok, dict(nad=0, n=0, out=None, reads=None, off=None), INV, b"null argument"),
        (ok, dict(nad=0, off=down), INV, b"not ascending"),
        (ok, dict(nad=0, qual=rd, qoff=down, oq=out8, off=huge), INV, b"not ascending"),
        (ok, dict(nad=0, off=huge), UNS, b"read 0 has 16777216 bytes"),
    )
    for params, kw, status, word in cases:
        rc, msg = call(params, **kw)
        assert rc == status and word in msg and b"polyhip_trim_reads" in msg, (kw, rc, msg)
    # the empty batch needs no device and no inputs: out_off[0] = 0, and the info is that of an empty call
    o64[:] = 7
    assert call(ok, nad=0, n=0, reads=None, off=None)[0] == _lib.OK and o64[0] == 0 and trim.last_info() == dict.fromkeys(to.INFO_FIELDS, 0)
    assert L.polyhip_trim_last_info(None) == INV
    r = trim.trim_packed(np.zeros(0, np.uint8), [0])
    assert len(r.seqs) == 0 and r.offsets.tolist() == [0] and r.quals is None and len(r.start) == 0

    # the pairs call shares the checks; what it adds: qualities of one mate only, and its own name in the message
    def pairs(params, q1=None, qo1=None, q2=None, qo2=None, oq1=None, oq2=None, off2=up, n=2):
        rc = L.polyhip_trim_pairs(C.byref(params), None, None, 0, p(rd), p(up), p(q1), p(qo1), p(rd), p(off2), p(q2), p(qo2), n, p(a32), p(a32),
                                  p(a32), p(a32), p(out8), p(oq1), p(o64), p(out8), p(oq2), p(o64))
        return rc, L.polyhip_last_error()

    for kw, status, word in ((dict(q1=rd, qo1=up, oq1=out8), INV, b"qualities of one mate only"),
                             (dict(q1=rd, qo1=up, q2=rd, qo2=up, oq1=out8), INV, b"out_qual is given exactly when qual is"),
                             (dict(off2=down), INV, b"not ascending"), (dict(off2=huge), UNS, b"2^24")):
        rc, msg = pairs(ok, **kw)
        assert rc == status and word in msg and b"polyhip_trim_pairs" in msg, (kw, rc, msg)
    rc, msg = pairs(P(33, 0, 0, 10, 3, 0, 20, 101))
    assert rc == INV and b"pair_err_pct" in msg
    assert pairs(ok, n=0)[0] == _lib.OK
    with pytest.raises(_lib.PolyhipError) as ei:
        trim.trim_packed(rd, up, adapters=["ACGN"])
    assert ei.value.status == INV and "adapter 0" in ei.value.message
    with pytest.raises(ValueError):
        trim.trim_packed(rd, up, quals=rd)
    with pytest.raises(ValueError):
        trim.trim_pairs_packed(rd, up, rd, [0, 8])


def test_kernels_use_no_scratch(tmp_path):
    """what the compiler made of trim.hip: its four kernels, none of which spills to scratch, none below 8 waves per SIMD"""
    import re
    import subprocess
    from poly_amd import build
    asm = str(tmp_path / "trim.s")
    flags = [f for f in build.CXXFLAGS if f != "-fPIC"]
    res = subprocess.run([build._hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(build.CSRC, "trim.hip"), "-o", asm],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    seen = {}
    for block in re.split(r"\n\s+- \.", open(asm).read().split("amdhsa.kernels:", 1)[1]):
        name = re.search(r"\.name:\s+\S*?\d+(decide|pair|finish|gather)_kernelE", block)
        if name:
            seen[name.group(1)] = {key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1)) for key in ("vgpr_count", "private_segment_fixed_size")}
    assert sorted(seen) == ["decide", "finish", "gather", "pair"], seen
    for kernel, m in seen.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_count"] <= 64, (kernel, m)


# ---------------------------------------------------------------- 4. what the definition recovers of planted inserts
def test_planted_inserts_are_recovered():
    """Pairs drawn from a text with inserts of 30..160 bases, 100-base reads that run into the adapters, one base in a hundred
    misread (tests/trim_inputs.py::planted).  A short insert counts as recovered when both mates end exactly at it.  The
    oracle alone recovers 222 of the 226 inserts shorter than the reads, 98.2 %, and leaves 168 of the 174 others whole (with
    min_overlap 3 a read that ends in AGA loses those three bases); the floor asserted is 95 %.  tests/test_trim_gpu.py runs
    the same pairs through the GPU and on into the mapper."""
    d = ti.planted()
    r = to.trim_pairs(d["reads1"], d["reads2"], d["quals1"], d["quals2"], [ti.ADAPTER, ti.ADAPTER2], **ti.PLANTED_PARAMS)
    short = [i for i, I in enumerate(d["insert"]) if I < ti.PLANTED_READ]
    exact = [i for i in short if r.end[2 * i] == r.end[2 * i + 1] == d["insert"][i] and r.start[2 * i] == r.start[2 * i + 1] == 0]
    whole = [i for i, I in enumerate(d["insert"]) if I >= ti.PLANTED_READ and r.end[2 * i] == r.end[2 * i + 1] == ti.PLANTED_READ]
    print(f"planted inserts: {len(exact)} of {len(short)} short ones recovered exactly, {len(whole)} of {ti.PLANTED_N - len(short)} others whole")
    assert len(short) > ti.PLANTED_N // 2 and len(exact) >= 0.95 * len(short)
    assert (len(exact), len(short), len(whole)) == (222, 226, 168)
    assert r.info["bad"] == 0 and r.info["overlap_cut"] > 0 and r.info["adapter_hits"] > 300
