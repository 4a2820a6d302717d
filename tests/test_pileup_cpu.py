"""polyhip_pileup without a GPU: the oracle (tests/pileup_oracle.py) against answers written out by hand, what the hand-built
inputs (tests/pileup_inputs.py) hold, the declarations, the argument errors that need no device, and planted variants found
again through the CPU oracle of the affine mapper."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import aln_records_inputs as ari  # noqa: E402
import pileup_inputs as pi  # noqa: E402
import pileup_oracle as po  # noqa: E402

INPUTS = ("flags", "mapq", "ref_start", "ref_end", "alnA", "alnB", "aln_off")


def _run(entries, ref, **kw):
    p = pi.pack(entries)
    return po.pileup(*[p[k] for k in INPUTS], ref, **kw)


def _want(s, k):
    return _run(s.entries, s.ref, **s.settings[k])


# ---------------------------------------------------------------- 1. the oracle against answers worked out by hand
#                 0123456789 11
WORKED_TEXT = b"ACGTACGTACGT"
# reads 0 and 2 (forward, from 0): T for G at 2, GG inserted after 5, 8..10 deleted; read 1 (reverse, from 2): the text's 2..9
WORKED_A = b"ACTTACGGGT---T"
WORKED_B = b"ACGTAC--GTACGT"
WORKED_COUNTS = [
    [2, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0],      # forward A
    [0, 2, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0],      # C
    [0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0],      # G
    [0, 0, 2, 2, 0, 0, 0, 2, 0, 0, 0, 2],      # T: the SNV at 2
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],      # other
    [0, 0, 0, 0, 0, 0, 0, 0, 2, 2, 2, 0],      # deleted bases
    [0, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0],      # insertion events: anchored at 5
    [0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 0],      # deletion events: anchored at 7
    [0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0],      # reverse A
    [0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0],      # C
    [0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0],      # G
    [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0],      # T
    [0] * 12, [0] * 12, [0] * 12, [0] * 12,
]
WORKED_SITES = [   # pos, depth, count, count_fwd, kind, ref, alt, pad
    (2, 3, 2, 2, 1, ord("G"), ord("T"), 0),
    (5, 3, 2, 2, 2, ord("C"), 0, 0),
    (7, 3, 2, 2, 3, ord("T"), 0, 0),
]


def _worked(**kw):
    fwd = pi.Entry("fwd", "", WORKED_A, WORKED_B, 0, 12)
    rev = pi.Entry("rev", "", WORKED_TEXT[2:10], WORKED_TEXT[2:10], 2, 10, flags=pi.MAPPED | pi.REVERSE)
    return _run((fwd, rev, fwd), WORKED_TEXT, **kw)


def test_oracle_worked_example():
    for kw in ({}, dict(min_alt_permille=500), dict(min_alt_permille=666, min_alt_count=2, min_depth=2)):
        r = _worked(**kw)
        assert r.counts.tolist() == WORKED_COUNTS and r.counts.shape == (16, 12) and r.counts.dtype == np.uint32
        assert r.consensus.tobytes() == b"ACTTACGT***T"
        assert r.site_list() == WORKED_SITES
        assert list(r.err) == [0, 0, 0]
        assert r.info == dict(entries=3, used=3, skipped_mapq=0, bad=0, columns=36, edge_events=0, sites=3)
    assert _worked(min_alt_permille=667).site_list() == []                   # 2 * 1000 < 667 * 3
    assert _worked(min_alt_count=3).site_list() == []
    deep = _worked(min_depth=3)                                                # positions 0, 1, 10 and 11 have depth 2
    assert deep.consensus.tobytes() == b"NNTTACGT**NN" and deep.site_list() == WORKED_SITES
    assert _worked(min_depth=4).consensus.tobytes() == b"N" * 12 and _worked(min_depth=4).site_list() == []
    part = _worked(region=(5, 8))
    assert part.counts.tolist() == [row[5:8] for row in WORKED_COUNTS] and part.consensus.tobytes() == b"CGT"
    assert part.site_list() == WORKED_SITES[1:]
    assert _worked(region=(6, 7)).site_list() == [] and _worked(region=(4, 4)).counts.shape == (16, 0)


def test_oracle_err_and_events_by_hand():
    T = b"ACGTACGT"
    e = lambda A, B, rs, re_: po.entry_err(len(A), A, B, rs, re_, T)      # noqa: E731
    assert e(b"ACGT", b"ACGT", 0, 4) == 0 and e(b"CGTA", b"CGTA", 1, 5) == 0
    assert e(b"AC-T", b"AC-T", 0, 3) == 1
    assert e(b"ACGT", b"ACGT", 0, 5) == 2 and e(b"ACGT", b"ACGT", 0, 3) == 2
    assert e(b"ACGTA", b"ACGTA", 4, 9) == 2                                  # the symbols agree, the text ends at 8
    assert e(b"", b"", 3, 3) == 3 and e(b"", b"", 3, 4) == 2
    assert e(b"ACGT", b"AGGT", 0, 4) == 5 and e(b"acgt", b"acgt", 0, 4) == 5   # raw bytes: no case is folded
    assert e(b"A--T", b"A--T", 0, 9) == 1 and e(b"ACGT", b"AGGT", 0, 5) == 2   # 1 before 2, 2 before 5
    assert e(b"GG", b"--", 8, 8) == 0                                          # an insertion alone, at the text's end
    assert po.entry_err((1 << 28), b"", b"", 0, 0, T) == 4 and po.entry_err((1 << 28) - 1, b"", b"", 0, 0, T) != 4
    # D I D: two deletion events, the second anchored at the first's base; I D I: the second insertion hangs on the deleted base
    assert po.entry_adds(b"A-G-C", b"AC-GC", 0, 0) == ([(0, 0), (7, 0), (5, 1), (6, 1), (7, 1), (5, 2), (1, 3)], 0)
    assert po.entry_adds(b"AG-GC", b"A-C-C", 4, 1) == ([(8, 4), (14, 4), (15, 4), (13, 5), (14, 5), (9, 6)], 0)
    assert po.entry_adds(b"GGAC", b"--AC", 0, 0) == ([(0, 0), (1, 1)], 1) and po.entry_adds(b"-C", b"AC", 0, 1) == ([(13, 0), (9, 1)], 1)
    assert po.entry_adds(b"GGAC", b"--CG", 1, 0) == ([(6, 0), (0, 1), (1, 2)], 0)
    assert po.entry_adds(b"aNn-", b"ACGT", 0, 0)[0] == [(0, 0), (4, 1), (4, 2), (7, 2), (5, 3)]
    # err 4 by faked offsets: the strings are not there to be read; unmapped and skipped entries are never read either
    big = po.pileup([1, 1], None, [0, 0], [4, 4], b"ACGT", b"ACGT", [0, 4, 4 + (1 << 28)], T)
    assert list(big.err) == [0, 4] and big.info["bad"] == 1 and big.info["used"] == 1 and big.info["columns"] == 4
    skip = po.pileup([1, 0, 1], [3, 60, 20], [0, 0, 0], [4, 0, 4], b"--------ACGT", b"--------ACGT", [0, 4, 8, 12], T, min_mapq=20)
    assert list(skip.err) == [0, 0, 0] and skip.info == dict(entries=3, used=1, skipped_mapq=1, bad=0, columns=4, edge_events=0, sites=0)
    # consensus: ties to the lowest k; a base against '*'
    assert po.call_position([2, 2, 0, 0, 0, 0, 0, 0] + [0] * 8, 65, 7, 0, 0, 0)[0] == ord("A")
    assert po.call_position([0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0], 84, 7, 0, 0, 0)[0] == ord("T")
    assert po.call_position([0, 0, 0, 1, 0, 2, 0, 0] + [0] * 8, 84, 7, 0, 0, 0)[0] == ord("*")
    assert po.call_position([0] * 16, 84, 7, 0, 0, 0) == (ord("N"), [])
    # a lower-case or unknown text byte: class by the same table; 'N' is class 4, so every base is an SNV
    assert [s[6] for s in po.call_position([1, 1, 1, 1] + [0] * 12, ord("c"), 0, 0, 0, 0)[1]] == list(b"AGT")
    assert [s[6] for s in po.call_position([1, 1, 1, 1] + [0] * 12, ord("N"), 0, 0, 0, 0)[1]] == list(b"ACGT")
    # order within a position: SNVs, then INS, then DEL; events count against the depth at their anchor
    got = po.call_position([0, 3, 0, 1, 0, 0, 1, 0, 4, 0, 0, 0, 0, 0, 0, 2], 65, 9, 0, 0, 0)[1]
    assert got == [(9, 8, 3, 3, 1, 65, 67, 0), (9, 8, 1, 1, 1, 65, 84, 0), (9, 8, 1, 1, 2, 65, 0, 0), (9, 8, 2, 0, 3, 65, 0, 0)]


# ---------------------------------------------------------------- 2. what the hand-built inputs hold
def _starts(classes, c):
    return [m.start() for m in re.finditer(f"(?<!{c}){c}", classes)]


def _ends(classes, c):
    return [m.end() for m in re.finditer(f"{c}(?!{c})", classes)]


def test_inputs_cover_the_walk():
    s = pi.shapes()
    assert pi.strings is ari.strings and pi.runs is ari.runs and pi.random_classes is ari.random_classes
    by = {e.name: e for e in s.entries}
    assert sorted(len(e.A) for e in s.entries if e.name.startswith("cols")) == [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4096 + 7168]
    for c in "ID":
        assert sorted(x for end in (63, 64, 65) for x in _ends(by[f"run_{c}_ends{end}"].classes, c)) == [63, 64, 65]
        t = by[f"run_{c}_three_steps"].classes
        assert _starts(t, c)[0] // 64 == 0 and (_ends(t, c)[0] - 1) // 64 == 3 and _ends(t, c)[0] - _starts(t, c)[0] >= 129
        assert _starts(by[f"run_{c}_starts_lane0"].classes, c) == [64]
    assert _starts(by["run_D_lane0_after_I"].classes, "D") == [64] and by["run_D_lane0_after_I"].classes[63] == "I"
    assert _starts(by["run_I_lane0_after_D"].classes, "I") == [64] and by["run_I_lane0_after_D"].classes[63] == "D"
    assert _starts(by["run_I_lane0_of_third_step"].classes, "I") == [128]
    assert "DID" in by["d_i_d"].classes and "IDI" in by["i_d_i"].classes
    assert {e.flags & pi.REVERSE for e in s.entries} == {0, pi.REVERSE}
    for st in pi.all_sets():
        assert len(st.settings) >= 2
        for e in st.entries:
            assert len(e.A) == len(e.B) and (not e.classes or len(e.classes) == len(e.A))
    # every used entry's b columns are the text, and every set has used entries
    for st in pi.all_sets():
        r = _want(st, 0)
        assert r.info["used"] > 0 and r.info["entries"] == len(st.entries)


def test_inputs_cover_edges_and_regions():
    s = pi.edges()
    by = {e.name: e for e in s.entries}
    assert by["i_first_at_0"].classes[0] == "I" and by["i_first_at_0"].ref_start == 0
    assert by["d_first_at_0"].classes[0] == "D" and by["d_first_at_0"].ref_start == 0
    r = _want(s, 0)
    assert r.info["edge_events"] == 5 and r.info["bad"] == 0 and _want(s, 2).info["edge_events"] == 5
    assert r.counts[6, 0] == 1 and r.counts[7, 0] == 1                 # the same events one position on are counted
    g = pi.regions()
    regs = [st["region"] for st in g.settings]
    L = len(g.ref)
    assert None in regs and any(r and r[1] - r[0] == 1 for r in regs) and sum(1 for r in regs if r and r[0] == r[1]) >= 3
    assert (0, 0) in regs and (L, L) in regs
    d, i, long_ = g.entries[0], g.entries[1], g.entries[2]
    assert d.classes == "====DDD===" and d.ref_start == 10 and i.classes == "====II====" and i.ref_start == 30
    whole = _want(g, 0)
    assert whole.counts[7, 13] == 1 and list(whole.counts[5, 14:17]) == [1, 1, 1] and whole.counts[8 + 6, 33] == 1
    assert (10, 14) in regs and (14, 20) in regs       # the deletion's anchor without its bases, its bases without the anchor
    assert (33, 34) in regs and (34, 40) in regs       # the insertion's anchor alone, and the bases after it
    assert any(r and long_.ref_start < r[0] < r[1] < long_.ref_end for r in regs)          # an entry cut at both ends
    assert any(r and d.ref_start < r[0] < d.ref_end <= r[1] for r in regs)                 # ... at its start only
    assert any(r and r[0] <= i.ref_start < r[1] < i.ref_end for r in regs)                 # ... at its end only
    for k, reg in enumerate(regs):
        if reg:
            got = _want(g, k)
            assert got.counts.tolist() == whole.counts[:, reg[0]:reg[1]].tolist()
            assert got.site_list() == [x for x in whole.site_list() if reg[0] <= x[0] < reg[1]]
            assert got.info["columns"] == whole.info["columns"]


def test_inputs_cover_contention_random_and_bytes():
    c = pi.contention()
    assert len(c.entries) == 257 and len(set(c.entries)) == 1 and c.entries[0].ref_end - c.entries[0].ref_start == 70
    r = _want(c, 0)
    assert r.counts.max() == 257 and [x[2] for x in r.site_list()] == [257, 257, 257] and sorted(x[4] for x in r.site_list()) == [1, 2, 3]
    assert _want(c, 1).info["sites"] == 3 and _want(c, 2).info["sites"] == 0 and _want(c, 2).consensus.tobytes() == b"N" * 90
    q = pi.random_set()
    assert len(q.entries) == 5000 and len(q.ref) == 300
    assert 2000 < sum(1 for e in q.entries if e.flags & pi.REVERSE) < 3000
    w = _want(q, 0)
    assert (w.counts[:8].sum(axis=1) > 0).sum() >= 7 and (w.counts[8:].sum(axis=1) > 0).sum() >= 7 and w.info["edge_events"] > 0
    assert 0 < _want(q, 1).info["skipped_mapq"] < 5000
    b = pi.byte_set()
    by = {e.name: e for e in b.entries}
    assert any(97 <= x <= 122 for x in by["lower_read"].A) and set(by["iupac_read"].A) & set(b"RYKMSWBDHVN")
    assert any(97 <= x <= 122 for x in b.ref) and b"N" in b.ref
    assert by["same_class_other_case"].A.isupper() and by["same_class_other_case"].B.islower()
    wb = _want(b, 0)
    assert wb.info["bad"] == 0 and wb.counts[4].sum() + wb.counts[12].sum() > 0
    assert any(chr(x[5]).islower() for x in wb.site_list()) and any(x[5] == ord("N") for x in wb.site_list())


def test_inputs_cover_errs():
    s = pi.errs()
    names = [e.name for e in s.entries]
    err = dict(zip(names, _want(s, 0).err.tolist()))
    assert err["good"] == 0 and err["ends_at_text_end"] == 0 and err["mapq_at_threshold"] == 0
    assert err["err1"] == 1 and err["err1_second_step"] == 1 and s.entries[names.index("err1_second_step")].classes.index("?") >= 64
    assert err["err2_end_short"] == err["err2_end_long"] == err["err2_beyond_text"] == 2
    e = s.entries[names.index("err2_beyond_text")]
    assert e.ref_start + pi.text_columns(e.B) == e.ref_end > len(s.ref)        # the second form of 2 alone
    assert err["err3"] == 3 and err["err2_before_err3"] == 2
    assert err["err5"] == 5 and err["err5_read_agrees"] == 5 and err["err5_second_step"] == 5
    assert err["err1_before_err2"] == 1 and err["err2_before_err5"] == 2
    assert err["unmapped_invalid"] == 0 and 45 in s.entries[names.index("unmapped_invalid")].B
    assert err["low_mapq_invalid"] == 1 and err["low_mapq_err5"] == 5
    for k in (1, 2):
        skipped = dict(zip(names, _want(s, k).err.tolist()))
        assert skipped["low_mapq_invalid"] == 0 and skipped["low_mapq_err5"] == 0 and skipped["err1"] == 1
        assert _want(s, k).info["skipped_mapq"] == 2 and _want(s, k).info["used"] == 3


def test_inputs_cover_thresholds_and_batches():
    s = pi.thresholds()
    d = pi.THRESHOLD_DEPTH
    kw = [dict((k, v) for k, v in st.items() if v) for st in s.settings]
    whole = _want(s, 0)
    assert set(whole.counts[:6, 10:40].sum(axis=0) + whole.counts[8:14, 10:40].sum(axis=0)) == {d}
    snv = lambda r: [(x[0], x[2]) for x in r.site_list() if x[4] == 1]      # noqa: E731
    assert snv(_want(s, kw.index(dict(min_alt_permille=250)))) == [(15, 2), (25, 4)]           # 2 * 1000 == 250 * 8: a site
    assert snv(_want(s, kw.index(dict(min_alt_permille=251)))) == [(25, 4)]
    assert snv(_want(s, kw.index(dict(min_alt_permille=125)))) == [(15, 2), (20, 1), (25, 4)]  # 1 * 1000 == 125 * 8
    assert snv(_want(s, kw.index(dict(min_alt_count=2)))) == [(15, 2), (25, 4)] and snv(_want(s, kw.index(dict(min_alt_count=3)))) == [(25, 4)]
    assert _want(s, kw.index(dict(min_depth=d - 1))).info["sites"] == _want(s, kw.index(dict(min_depth=d))).info["sites"] > 0
    deep = _want(s, kw.index(dict(min_depth=d + 1)))
    assert deep.info["sites"] == 0 and deep.consensus.tobytes() == b"N" * 50
    r = _want(s, kw.index(dict(min_depth=d)))
    two = r.counts[:8].astype(int) + r.counts[8:].astype(int)
    assert two[0, 25] == two[1, 25] == 4 and r.consensus[25] == ord("A")       # a tie between two bases: the lower k
    assert two[0, 30] == two[5, 30] == 4 and r.consensus[30] == ord("A")       # a tie between a base and '*'
    assert r.consensus.tobytes() == b"N" * 10 + b"A" * 30 + b"N" * 10
    assert [len(pi.batch(n).entries) for n in ari.BATCH_SIZES] == [1, 255, 256, 257] == list(ari.BATCH_SIZES)
    assert any(len(e.A) == ari.LONGEST for e in pi.batch(257).entries) and any(not e.flags & 1 for e in pi.batch(255).entries)


# ---------------------------------------------------------------- 3. the declarations
def test_declarations():
    from poly_amd import _lib, pileup
    for name in ("polyhip_pileup", "polyhip_pileup_last_info"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["polyhip_pileup"][1]) == 17
    assert C.sizeof(pileup._CParams) == 32 and C.sizeof(pileup._CInfo) == 56
    assert pileup.SITE_DTYPE == po.SITE_DTYPE and pileup.SITE_DTYPE.itemsize == 20 and pileup.CHANNELS == po.CHANNELS == 16
    header = open(os.path.join(ROOT, "include", "polyhip.h")).read()
    assert "#define POLYHIP_PILEUP_CHANNELS 16u" in header
    assert callable(pileup.pileup_packed) and callable(pileup.pileup) and callable(pileup.last_info)
    p = pileup.Pileup(np.arange(32, dtype=np.uint32).reshape(16, 2), np.frombuffer(b"AC", np.uint8), None, np.zeros(0, np.uint32))
    assert p.depth().tolist() == [sum(range(0, 12, 2)) + sum(range(16, 28, 2)), sum(range(1, 12, 2)) + sum(range(17, 28, 2))]
    assert p.consensus_string() == "AC"


def test_argument_errors_without_gpu():
    """what is decided before any device call returns its status without a device"""
    from poly_amd import _lib, pileup
    L = _lib.lib()
    one32, one8, off = np.zeros(1, np.uint32), np.zeros(1, np.uint8), np.zeros(2, np.uint64)
    counts, cons, ns = np.zeros(16 * 4, np.uint32), np.zeros(4, np.uint8), C.c_uint64(7)
    ref = np.frombuffer(b"ACGT", np.uint8)

    def call(params, mapq=None, n=1):
        return L.polyhip_pileup(None if params is None else C.byref(params), n, one32.ctypes.data, mapq, one32.ctypes.data, one32.ctypes.data,
                                one8.ctypes.data, one8.ctypes.data, off.ctypes.data, ref.ctypes.data, 4, counts.ctypes.data, cons.ctypes.data,
                                C.byref(ns), None, 0, one32.ctypes.data)

    P = pileup._CParams
    assert call(None) == _lib.ERR_INVALID and b"null params" in L.polyhip_last_error()
    assert call(P(3, 2, 0, 0, 0, 0)) == _lib.ERR_INVALID and b"region_lo" in L.polyhip_last_error()
    assert call(P(0, 5, 0, 0, 0, 0)) == _lib.ERR_INVALID and b"region_hi" in L.polyhip_last_error()
    assert call(P(0, 4, 0, 0, 0, 1001)) == _lib.ERR_INVALID and b"min_alt_permille" in L.polyhip_last_error()
    assert call(P(0, 4, 0, 0, 0, 1000), n=1 << 32) == _lib.ERR_UNSUPPORTED
    assert call(P(0, 4, 1, 0, 0, 0)) == _lib.ERR_INVALID and b"mapq" in L.polyhip_last_error()
    assert call(P(3, 2, 1, 0, 0, 1001)) == _lib.ERR_INVALID and b"region_lo" in L.polyhip_last_error()   # the first that applies
    assert ns.value == 7                                                                               # nothing was written
    with pytest.raises(_lib.PolyhipError) as ei:
        pileup.pileup_packed([1], [0], [4], ref, ref, [0, 4], b"ACGT", min_alt_permille=1001)
    assert ei.value.status == _lib.ERR_INVALID


# ---------------------------------------------------------------- 4. planted variants, through the mapper's CPU oracle
def test_planted_variants_are_the_sites():
    import map_affine_inputs as mai
    import map_affine_oracle as mao
    d = pi.planted()
    T = d["T"]
    assert len(T) == 2000 and len(d["reads"]) == 200 and {len(r) for r in d["reads"]} == {100} and len(d["sample"]) == 1999
    hits, _ = mao.map_reads(T, d["reads"], mai.MAT, *mai.GAPS[0], mai.PARAMS)
    assert sum(h.flags & 1 for h in hits) == 200 and 90 <= sum(h.flags >> 1 & 1 for h in hits) <= 110
    A = [bytes(h.alignA) if h.flags & 1 else b"" for h in hits]
    B = [bytes(h.alignB) if h.flags & 1 else b"" for h in hits]
    off = np.zeros(len(hits) + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in A])
    r = po.pileup([h.flags for h in hits], None, [h.ref_start for h in hits], [h.ref_end for h in hits], b"".join(A), b"".join(B), off, T,
                  min_alt_permille=500)
    assert r.info["bad"] == 0 and r.info["used"] == 200
    assert [(x[0], x[4]) for x in r.site_list()] == list(pi.PLANTED_SITES)
    snv, dele, ins = r.site_list()
    assert snv[5] == T[500] and snv[6] == d["snv"] and snv[2] == snv[1] >= 5 and 0 < snv[3] < snv[2]     # both strands say so
    assert dele[2] >= 5 and ins[2] >= 5
    assert list(r.counts[5, 1000:1003] + r.counts[13, 1000:1003]) == [dele[2]] * 3
    want = bytearray(T)
    want[500] = d["snv"]
    assert r.consensus[:1000].tobytes() == bytes(want[:1000]) and r.consensus[1000:1003].tobytes() == b"***"
