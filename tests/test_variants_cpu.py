"""polyhip_call_variants without a GPU: the oracle (tests/variants_oracle.py) against records written out by hand for each rule of
the definition and against polyhip_pileup_qual's oracle, what the hand-built inputs (tests/variants_inputs.py) hold, the
declarations, the argument errors in their documented order (all decided before any device call), poly_amd.vcf against lines
written out by hand, and the planted variants through the mapper's CPU oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import pileup_qual_oracle as qo  # noqa: E402
import variants_inputs as vi  # noqa: E402
import variants_oracle as vo  # noqa: E402

M, R = vi.MAPPED, vi.REVERSE
HAND_TEXT = b"TTGACCGATAGGCTCAATCG"


def _run(entries, text, with_qual=False, **st):
    s = vi.attach("hand", entries, text, (), 99)
    return vo.call_variants(*vi.oracle_args(s, with_qual), **dict(vi.DEFAULTS, **st))


def _sets():
    return {s.name: s for s in vi.all_sets()}


# ---------------------------------------------------------------- 1. the oracle against records worked out by hand
def _hand_entries():
    ops = (("=", 3), ("I", b"tT"), ("=", 3), ("D", 2), ("=", 4))          # GAC +tT CGA -TA GGCT on positions 2..13
    return (vi.make("fwd", HAND_TEXT, 2, ops), vi.make("rev", HAND_TEXT, 2, ops, M | R),
            vi.make("snv", HAND_TEXT, 2, (("=", 5), ("X", b"T"), ("=", 6))))


def test_oracle_by_hand_without_left_alignment():
    r = _run(_hand_entries(), HAND_TEXT, left_align=0)
    # (allele_off, pos, depth, count, count_fwd, ref_count, qsum, allele_len, kind, ref, alt, gt)
    assert r.record_list() == [(0, 4, 3, 2, 1, 1, 0, 2, 2, ord("C"), 0, 1),
                               (0, 7, 3, 1, 1, 2, 0, 1, 1, ord("A"), ord("T"), 1),
                               (0, 7, 3, 2, 1, 1, 0, 2, 3, ord("A"), 0, 1)]
    assert r.alleles.tobytes() == b"TT"                                   # folded
    assert r.info == dict(entries=3, used=3, skipped_mapq=0, bad=0, columns=40, edge_events=0, sites=3, filtered_bases=0, events=4,
                          long_events=0, open_events=0, shifted_events=0, alleles=2, allele_bytes=2)


def test_oracle_by_hand_with_left_alignment():
    # GATAG: taking TA out of 8..9 is taking AT out of 7..8; the G at 6 stops the walk.  The insertion behind C ends in T: it stays
    r = _run(_hand_entries(), HAND_TEXT)
    assert r.record_list() == [(0, 4, 3, 2, 1, 1, 0, 2, 2, ord("C"), 0, 1),
                               (0, 6, 3, 2, 1, 1, 0, 2, 3, ord("G"), 0, 1),
                               (0, 7, 3, 1, 1, 2, 0, 1, 1, ord("A"), ord("T"), 1)]
    assert r.info["shifted_events"] == 2 and r.info["events"] == 4
    # hom_permille: 2 of 3 reads are 666 permille
    assert [x[-1] for x in _run(_hand_entries(), HAND_TEXT, hom_permille=666).record_list()] == [2, 2, 1]
    assert [x[-1] for x in _run(_hand_entries(), HAND_TEXT, hom_permille=667).record_list()] == [1, 1, 1]
    # max_indel = 1 drops all four events as long ones; the SNV stays
    r = _run(_hand_entries(), HAND_TEXT, max_indel=1)
    assert [x[8] for x in r.record_list()] == [1] and r.info["long_events"] == 4 and r.info["events"] == 0 and r.info["alleles"] == 0
    # with qualities the SNV carries the quality sum of its one read
    s = vi.attach("hand", _hand_entries(), HAND_TEXT, (), 99)
    r = _run(_hand_entries(), HAND_TEXT, with_qual=True)
    assert r.record_list()[2][6] == s.quals[2][s.read_start[2] + 5] - 33


def test_oracle_shift_rules_by_hand():
    text = b"GCAAAAATCCGTAGGAT"
    k = lambda ops, rs=0, **kw: _run((vi.make("e", text, rs, ops),), text, **kw)      # noqa: E731
    # an A behind AAAAA moves to the C in front of them; written in lower case it is the same allele
    r = k((("=", 7), ("I", b"a"), ("=", 5)))
    assert r.record_list() == [(0, 1, 1, 1, 1, 0, 0, 1, 2, ord("C"), 0, 2)] and r.alleles.tobytes() == b"A"
    assert k((("=", 7), ("I", b"a"), ("=", 5)), left_align=0).record_list()[0][1] == 6
    # a read that begins inside the run does not show where it starts: open with left alignment, counted without
    r = k((("=", 3), ("D", 1), ("=", 5)), rs=3)
    assert r.info["open_events"] == 1 and r.info["events"] == 0 and len(r.records) == 0
    assert k((("=", 3), ("D", 1), ("=", 5)), rs=3, left_align=0).record_list()[0][1:4] == (5, 1, 1)
    # a mismatch column stops the walk: the deletion of one A lands behind the mismatch at 4
    r = k((("=", 4), ("X", b"G"), ("=", 1), ("D", 1), ("=", 6)))
    assert [(x[1], x[8]) for x in r.record_list()] == [(4, 1), (4, 3)]
    # an I run directly in front of a D run: the D run does not move (the column before it is no match column), the I run does
    r = k((("=", 7), ("I", b"A"), ("D", 2), ("=", 5)))
    assert sorted((x[1], x[8]) for x in r.record_list()) == [(1, 2), (6, 3)]
    # a run that opens the entry: anchor ref_start - 1 without left alignment, -1 at the start of the text
    assert k((("D", 2), ("=", 5)), rs=2, left_align=0).groups == {(1, 3, 2, b""): [1, 1]}
    r = k((("I", b"TT"), ("=", 5)), left_align=0)
    assert r.info["edge_events"] == 1 and r.info["events"] == 0
    # two insertions of one length behind one position, ordered by their bytes; the shorter one first; deletions by length last
    ents = tuple(vi.make(f"e{i}", text, 8, (("=", 3), ("I", x), ("=", 4))) for i, x in enumerate((b"GT", b"GA", b"G", b"GT")))
    ents += (vi.make("d", text, 8, (("=", 3), ("D", 2), ("=", 2))), vi.make("d1", text, 8, (("=", 3), ("D", 1), ("=", 3))))
    r = _run(ents, text, left_align=0)
    assert [(x[1], x[8], x[7], x[3], x[0]) for x in r.record_list()] == [(10, 2, 1, 1, 0), (10, 2, 2, 1, 1), (10, 2, 2, 2, 3), (10, 3, 1, 1, 0),
                                                                       (10, 3, 2, 1, 0)]
    assert r.alleles.tobytes() == b"GGAGT" and [x[5] for x in r.record_list()] == [2, 2, 2, 4, 4]     # depth 6 less the site's events


# ---------------------------------------------------------------- 2. the oracle against polyhip_pileup_qual's oracle
IDENTITY = dict(left_align=0, min_alt_count=1, min_alt_permille=0, max_indel=255, min_depth=0)


@pytest.mark.parametrize("name", vi.SET_NAMES)
def test_oracle_agrees_with_the_pileup(name):
    s = _sets()[name]
    for st in s.settings:
        st = dict(st, **IDENTITY)
        r = vo.call_variants(*vi.oracle_args(s), **st)
        p = r.planes
        assert isinstance(p, qo.Result)
        snv = [(x[1], x[2], x[3], x[4], x[8], x[9], x[10]) for x in r.record_list() if x[8] == 1]
        assert snv == [x[:7] for x in p.site_list() if x[4] == 1]
        lo, hi = st["region"] or (0, len(s.ref))
        short = 0
        for kind, ch in ((2, 6), (3, 7)):
            for j in range(hi - lo):
                mine = [g for key, g in r.groups.items() if key[0] == lo + j and key[1] == kind]
                two, fwd = sum(g[0] for g in mine), sum(g[1] for g in mine)
                assert two <= int(p.counts[ch, j]) + int(p.counts[8 + ch, j]) and fwd <= int(p.counts[ch, j])
                short += int(p.counts[ch, j]) + int(p.counts[8 + ch, j]) - two
        # the pileup counts every run; this call leaves out the long ones and nothing else
        assert short <= r.info["long_events"] and (st["region"] is not None or short == r.info["long_events"])
        assert r.info["edge_events"] == p.info["edge_events"] and r.info["open_events"] == 0
        assert (r.err == p.err).all() and all(r.info[f] == p.info[f] for f in ("used", "skipped_mapq", "bad", "columns", "filtered_bases"))


# ---------------------------------------------------------------- 3. what the inputs hold
def _of(name, k, with_qual=True):
    s = _sets()[name]
    return vo.call_variants(*vi.oracle_args(s, with_qual), **s.settings[k])


def test_set_names():
    assert tuple(s.name for s in vi.all_sets()) == vi.SET_NAMES
    for s in vi.all_sets():
        assert len(s.ref) <= 13000 and len(s.entries) <= 600 and len(s.settings) >= 2
        assert all(set(st) == set(vi.DEFAULTS) for st in s.settings)


def test_steps_and_lengths_hold_what_they_promise():
    s = _sets()["steps"]
    starts = {e.name: [c for c in range(len(e.classes)) if e.classes[c] in "ID" and (c == 0 or e.classes[c - 1] != e.classes[c])] for e in s.entries}
    assert [starts[f"{c}_starts{n}"] for c in "id" for n in (63, 64, 65)] == [[63], [64], [65]] * 2
    assert starts["i_three_steps"] == [60] and s.entries[6].classes.count("I") == 140 and s.entries[7].classes.count("D") == 140
    assert starts["i_first"] == [0] and starts["d_first"] == [0] and starts["i_then_d_first"] == [0, 2]
    assert s.entries[10].classes.endswith("I") and s.entries[11].classes.endswith("D")
    r = _of("steps", 1)                                               # nothing moves, nothing is open
    assert r.info["events"] == 15 and r.info["open_events"] == 0 and r.info["alleles"] == 15
    assert _of("steps", 0).info["open_events"] == 3                  # i_first, d_first and the I of i_then_d_first
    s = _sets()["lengths"]
    runs = sorted({(max(e.classes.count("I"), e.classes.count("D"))) for e in s.entries})
    assert runs == sorted(vi.LENGTHS + (3, 4))
    r = _of("lengths", 1)
    assert r.info["long_events"] == 3 and r.info["events"] == 30     # 256: two insertions and a deletion
    assert sorted({int(x) for x in r.records["allele_len"]}) == [1, 3, 4, 7, 8, 9, 16, 17, 254, 255]
    assert all(int(x["count"]) == 2 for x in r.records if x["kind"] == 2)      # the same bytes on both strands: one allele
    assert _of("lengths", 3).info["events"] == 6 and _of("lengths", 3).info["long_events"] == 27      # max_indel 3: 1 and 3 stay, 4 goes
    assert _of("lengths", 5).info["long_events"] == 6                # max_indel 254: 255 goes too


def test_grouping_holds_what_it_promises():
    P, b = vi.GROUP_AT, vi.GROUP_BASE
    for k in (0, 1):
        g = _of("grouping", k).groups
        change = lambda i: b[:i] + (b"G" if b[i] != 71 else b"T") + b[i + 1:]      # noqa: E731
        assert g == {(P, 2, 12, b): [73, 38], (P, 2, 12, change(0)): [2, 2], (P, 2, 12, change(11)): [2, 0], (P, 2, 12, change(8)): [3, 3],
                     (P, 2, 12, change(7)): [1, 1], (P, 2, 12, b[:5] + b"N" + b[6:]): [2, 2], (P, 2, 11, b[:11]): [2, 2], (P, 2, 2, b"GG"): [2, 2],
                     (P, 3, 2, b""): [5, 4], (P, 3, 5, b""): [2, 2]}
    r = _of("grouping", 0)
    depth = len(_sets()["grouping"].entries)
    assert [int(x) for x in r.records["allele_len"]] == [2, 11, 12, 12, 12, 12, 12, 12, 2, 5] and set(r.records["depth"]) == {depth}
    assert [r.allele(i)[:1] for i in range(2, 8)] == [b"C", b"C", b"C", b"C", b"C", b"G"]      # by bytes: the changed first byte last
    assert set(int(x) for x in r.records["ref_count"][:8]) == {depth - 87} and int(r.records["ref_count"][8]) == depth - 7
    assert [int(x) for x in _of("grouping", 2).records["count"]] == [73, 3, 5]      # min_alt_count 3
    assert len(_of("grouping", 5).records) == 0 and _of("grouping", 5).info["events"] == 94      # the region begins behind the anchor


def test_repeats_hold_what_they_promise():
    with_la, without = _of("repeats", 0), _of("repeats", 1)
    A = vi.REP_AT - 1
    ndel = len(range(0, 2 * vi.REP_UNITS - 1, 3))
    assert ndel == 27
    assert with_la.groups[A, 3, 2, b""][0] == ndel + 1 and with_la.groups[A, 2, 2, b"AC"] == [2, 2]
    assert {A + d for d in range(0, 79, 3)} <= {k[0] for k in without.groups if k[1:3] == (3, 2)} and (A, 3, 2, b"") in without.groups
    assert without.groups[A, 3, 2, b""] == [1, 1]                                             # one allele at 27 anchors
    H = vi.HOMO_AT - 1
    assert with_la.groups[H, 2, 1, b"A"] == [2, 1] and with_la.groups[H, 3, 1, b""] == [1, 1]      # 200 and 130 columns back
    assert with_la.groups[vi.REP_AT + 30, 3, 2, b""] == [1, 1]                                 # the mismatch column
    assert with_la.groups[vi.REP_AT + 39, 3, 2, b""] == [1, 1]                                 # the D run behind an I run
    assert with_la.info["open_events"] == 3 and without.info["open_events"] == 0 and without.info["events"] == with_la.info["events"] + 3
    # min_alt_count 5: the split allele passes only when it is put together
    assert [tuple(x)[1:4] for x in _of("repeats", 6).record_list()] == [(A, with_la.records[0]["depth"], ndel + 1)]
    assert len(_of("repeats", 7).records) == 0
    # the region (130, 600) loses the deletions to the shift; (90, 120) gains them
    assert (A, 3, 2, b"") not in _of("repeats", 2).groups and len([k for k in _of("repeats", 3).groups if k[1] == 3]) > 15
    assert _of("repeats", 4).groups[A, 3, 2, b""][0] == ndel + 1 and sum(g[0] for g in _of("repeats", 5).groups.values()) == 7 + 2      # d = 0..18 and the two at 109
    t = _of("text_start", 0)
    assert (t.info["edge_events"], t.info["open_events"], t.info["events"], t.info["shifted_events"]) == (2, 4, 1, 1)
    assert t.groups == {(1, 2, 1, b"A"): [1, 1]}
    t = _of("text_start", 1)
    assert (t.info["edge_events"], t.info["open_events"], t.info["events"]) == (3, 0, 4)


def test_thresholds_and_the_rest_hold_what_they_promise():
    P, D, W = vi.THR_AT, vi.THR_DEPTH, vi.THR_WITH
    at = lambda r, p: [tuple(x) for x in r.record_list() if x[1] == p]      # noqa: E731
    assert W * 1000 == 250 * D
    assert at(_of("thresholds", 0), P) == [(0, P, D, W, 3, D - W, 0, 2, 2, 65, 0, 1)] and at(_of("thresholds", 1), P) == []
    assert len(at(_of("thresholds", 2), P)) == 1 and at(_of("thresholds", 3), P) == []
    assert at(_of("thresholds", 4), P)[0][-1] == 2 and at(_of("thresholds", 5), P)[0][-1] == 1
    assert at(_of("thresholds", 6), P)[0][-1] == 2 and at(_of("thresholds", 7), P)[0][-1] == 1
    assert at(_of("thresholds", 8), 100) == [(0, 100, 1, 3, 3, 0, 0, 2, 3, 65, 0, 2)]          # more events than reads: ref_count 0
    assert at(_of("thresholds", 0), 139)[0][2:6] == (4, 4, 3, 0) and at(_of("thresholds", 9), 139)[0][2:6] == (1, 4, 3, 0)
    assert [x[1] for x in _of("thresholds", 10).record_list()] == [100, 139]                   # 1000 permille of the filtered depth
    assert at(_of("thresholds", 11), P) == [] and len(at(_of("thresholds", 12), P)) == 1
    assert _of("thresholds", 0, with_qual=False).record_list() == _of("thresholds", 0).record_list()
    e = _of("errs", 0)
    assert {int(x) for x in e.err} == {0, 1, 2, 3, 5, 6, 7} and {int(x) for x in _of("plain_errs", 0).err} == {0, 1, 2, 3, 5}
    bad = [x for x, code in zip(_sets()["errs"].entries, e.err) if code]
    assert sum("I" in x.classes and "D" in x.classes for x in bad) >= 10     # entries whose events must not be counted
    assert e.info["events"] == 10 and _of("errs", 0, with_qual=False).info["events"] == 30      # err 6 and 7 need qualities
    assert _of("errs", 2).info["skipped_mapq"] == 1
    assert _of("no_events", 0).info["events"] == 0 and len(_of("no_events", 0).records) == 12 and len(_of("no_events", 2).records) == 1
    for k in (0, 1):
        assert len(_of("none_passing", k).records) == 0 and _of("none_passing", k).info["alleles"] == 12
    assert _of("random", 0).info["shifted_events"] > 300 and _of("random", 0).info["open_events"] > 50


# ---------------------------------------------------------------- 4. the declarations and the errors that need no device
def test_declarations():
    from poly_amd import _lib, variants
    assert len(_lib.SIGNATURES["polyhip_call_variants"][1]) == 21 and len(_lib.SIGNATURES["polyhip_call_variants_last_info"][1]) == 1
    assert C.sizeof(variants._CVarParams) == 56 and C.sizeof(variants._CVarInfo) == 112 and variants.VARIANT_DTYPE.itemsize == 40
    assert variants.VARIANT_DTYPE == vo.VARIANT_DTYPE and tuple(n for n, _ in variants._CVarInfo._fields_) == vo.INFO_FIELDS
    header = open(os.path.join(ROOT, "include", "polyhip.h")).read()
    assert "#define POLYHIP_ABI_VERSION 1\n" in header and "#define POLYHIP_VAR_MAX_INDEL 255u" in header
    assert "uint32_t pos, depth, count, count_fwd, ref_count, qsum, allele_len;" in header and "uint8_t kind, ref, alt, gt;" in header
    for n in ("polyhip_call_variants", "polyhip_call_variants_last_info"):
        assert hasattr(_lib.lib(), n) and not hasattr(_lib.lib(), n + "_dev")
    for f in (variants.call_packed, variants.call, variants.call_refs, variants.last_info):
        assert callable(f)


def test_argument_errors_without_gpu():
    """everything the header lists up to the offsets is decided before any device call, in the documented order: each case holds
    every later fault as well"""
    from poly_amd import _lib, variants
    from poly_amd.pileup import _CParams, _CQualParams
    L = _lib.lib()
    s = _sets()["text_start"]
    p = vi.pack(s)
    n, ref = len(s.entries), np.frombuffer(s.ref, np.uint8)
    nv, nb = C.c_uint64(0xAB), C.c_uint64(0xAB)
    err = np.full(n, 0xABABABAB, np.uint32)
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED

    def P(lo=0, hi=len(s.ref), min_mapq=0, permille=0, mbq=0, qoff=33, hom=800, max_indel=0, pad=0):
        return variants._CVarParams(_CQualParams(_CParams(lo, hi, min_mapq, 1, 1, permille), mbq, qoff), 1, hom, max_indel, pad)

    def call(params, null=(), n_claimed=None, arrays=p, vcap=0, acap=0, ref_len=len(s.ref)):
        a = lambda k: None if k in null else arrays[k].ctypes.data      # noqa: E731
        rc = L.polyhip_call_variants(None if params is None else C.byref(params), n if n_claimed is None else n_claimed, a("flags"), a("mapq"),
                                     a("ref_start"), a("ref_end"), a("read_start"), a("alnA"), a("alnB"), a("aln_off"), a("qual"), a("qual_off"),
                                     None if "ref" in null else ref.ctypes.data, ref_len, None if "nvariants" in null else C.byref(nv), None, vcap,
                                     None if "nallele_bytes" in null else C.byref(nb), None, acap, None if "err" in null else err.ctypes.data)
        return rc, L.polyhip_last_error()

    every = ("flags", "mapq", "ref_start", "ref_end", "read_start", "alnA", "alnB", "aln_off", "qual_off", "ref", "nvariants", "nallele_bytes", "err")
    big_q, big = (1 << 32) // 93 + 1, 1 << 32
    down = dict(p, aln_off=p["aln_off"][::-1].copy())
    qdown = dict(p, qual_off=p["qual_off"][::-1].copy())
    worst = dict(null=every + ("qual",), n_claimed=big)
    bad = dict(min_mapq=1, mbq=94, qoff=163, hom=1001, max_indel=256, pad=1)
    cases = (
        (None, worst, INV, b"null params"),
        (P(lo=3, hi=2, permille=1001, **bad), worst, INV, b"region_lo"),
        (P(hi=len(s.ref) + 1, permille=1001, **bad), worst, INV, b"region_hi"),
        (P(permille=1001, **bad), worst, INV, b"min_alt_permille = 1001"),
        (P(**bad), worst, INV, b"min_base_qual = 94"),
        (P(**dict(bad, mbq=93)), worst, INV, b"qual_offset = 163"),
        (P(**dict(bad, mbq=93, qoff=162)), worst, INV, b"hom_permille = 1001"),
        (P(**dict(bad, mbq=93, qoff=162, hom=1000)), worst, INV, b"max_indel = 256"),
        (P(**dict(bad, mbq=93, qoff=162, hom=1000, max_indel=255)), worst, INV, b"pad = 1"),
        (P(min_mapq=1, mbq=1), worst, INV, b"min_base_qual = 1 needs qual"),
        (P(min_mapq=1), worst, UNS, b"4294967296 entries"),
        (P(min_mapq=1), dict(null=every, n_claimed=big_q), UNS, b"%d entries" % big_q),
        (P(min_mapq=1), dict(null=every + ("qual",), n_claimed=big - 1), INV, b"min_mapq = 1 needs mapq"),
        (P(min_mapq=1), dict(null=every), INV, b"min_mapq = 1 needs mapq"),
        (P(), dict(null=("ref",), arrays=down), INV, b"null argument"),
        (P(), dict(null=("nvariants",), arrays=down), INV, b"null argument"),
        (P(), dict(null=("nallele_bytes",), arrays=down), INV, b"null argument"),
        (P(), dict(vcap=1, arrays=down), INV, b"null argument"),
        (P(), dict(acap=1, arrays=down), INV, b"null argument"),
        (P(), dict(null=("flags",), arrays=down), INV, b"null argument"),
        (P(), dict(null=("ref_end",), arrays=down), INV, b"null argument"),
        (P(), dict(null=("alnA",), arrays=down), INV, b"null argument"),
        (P(), dict(null=("read_start",), arrays=down), INV, b"null argument"),
        (P(), dict(null=("qual_off",), arrays=down), INV, b"null argument"),
        (P(), dict(null=("err",), arrays=down), INV, b"null argument"),
        (P(), dict(arrays=down), INV, b"not ascending"),
        (P(), dict(arrays=qdown), INV, b"not ascending"),
    )
    for params, kw, status, word in cases:
        rc, msg = call(params, **kw)
        assert rc == status and word in msg and b"polyhip_call_variants" in msg, (kw, rc, msg)
        assert nv.value == 0xAB and nb.value == 0xAB and (err == 0xABABABAB).all()
    assert L.polyhip_call_variants_last_info(None) == INV
    acgt = np.frombuffer(b"ACGT", np.uint8)
    with pytest.raises(_lib.PolyhipError) as ei:
        variants.call_packed([1], [0], [4], acgt, acgt, [0, 4], b"ACGT", hom_permille=1001)
    assert ei.value.status == INV and "hom_permille" in ei.value.message
    with pytest.raises(ValueError, match="qual comes with"):
        variants.call_packed([1], [0], [4], acgt, acgt, [0, 4], b"ACGT", qual=acgt)
    with pytest.raises(ValueError, match="different numbers"):
        variants.call_packed([1], [0, 0], [4], acgt, acgt, [0, 4], b"ACGT")


# ---------------------------------------------------------------- 5. VCF text
def _variants_of(r, ref):
    from poly_amd import variants
    return variants.Variants(r.records, r.alleles, r.err, np.frombuffer(ref, np.uint8))


def test_vcf_lines_by_hand():
    from poly_amd import vcf
    r = _run(_hand_entries(), HAND_TEXT, left_align=0, hom_permille=600)
    v = _variants_of(r, HAND_TEXT)
    assert [(v.ref_allele(i), v.alt_allele(i)) for i in range(3)] == [(b"C", b"CTT"), (b"A", b"T"), (b"ATA", b"A")]
    text = vcf.write(v, HAND_TEXT, "plasmid", sample="s1")
    assert text.decode().split("\n") == [
        "##fileformat=VCFv4.2",
        "##contig=<ID=plasmid,length=20>",
        "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Reads covering the position\">",
        "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">",
        "##FORMAT=<ID=AD,Number=R,Type=Integer,Description=\"Reads for the reference and for the allele\">",
        "##FORMAT=<ID=ADF,Number=A,Type=Integer,Description=\"Reads for the allele on the forward strand\">",
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1",
        "plasmid\t5\t.\tC\tCTT\t.\t.\tDP=3\tGT:AD:ADF\t1/1:1,2:1",
        "plasmid\t8\t.\tA\tT\t.\t.\tDP=3\tGT:AD:ADF\t0/1:2,1:1",
        "plasmid\t8\t.\tATA\tA\t.\t.\tDP=3\tGT:AD:ADF\t1/1:1,2:1",
        ""]
    rows = vcf.parse(text)
    assert rows == vcf.rows(v, HAND_TEXT, "plasmid") and vcf.parse(text.decode()) == rows
    assert rows[2] == vcf.Row("plasmid", 7, b"ATA", b"A", 3, 1, 2, 1, 2)
    assert vi.called(rows) == [(4, 2, b"TT"), (7, 1, b"T"), (7, 3, 2)]
    # apply: the two 1/1 records; with min_gt = 1 the SNV and the deletion touch the same byte
    assert vcf.apply(HAND_TEXT, rows) == HAND_TEXT[:5] + b"TT" + HAND_TEXT[5:8] + HAND_TEXT[10:] == vcf.apply(HAND_TEXT, v)
    with pytest.raises(ValueError, match="overlaps"):
        vcf.apply(HAND_TEXT, rows, min_gt=1)
    assert vcf.apply(HAND_TEXT, rows[:2], min_gt=1) == HAND_TEXT[:5] + b"TT" + HAND_TEXT[5:7] + b"T" + HAND_TEXT[8:]
    assert vcf.apply(HAND_TEXT, []) == HAND_TEXT
    with pytest.raises(ValueError, match="not what the text holds"):
        vcf.apply(HAND_TEXT[1:], rows)
    with pytest.raises(ValueError, match="not one that vcf.write produces"):
        vcf.parse(b"plasmid\t5\t.\tC\tCTT\t.\t.\tDP=3\n")


def test_vcf_round_trip_on_every_set():
    from poly_amd import vcf
    for s in vi.all_sets():
        r = vo.call_variants(*vi.oracle_args(s), **s.settings[0])
        v = _variants_of(r, s.ref)
        rows = vcf.rows(v, s.ref, s.name)
        assert vcf.parse(vcf.write(v, s.ref, s.name)) == rows and len(rows) == len(r.records)
        for i, row in enumerate(rows):
            assert (row.ref, row.alt) == (v.ref_allele(i), v.alt_allele(i)) and row.ref[:1] == row.alt[:1] or len(row.ref) == len(row.alt) == 1


# ---------------------------------------------------------------- 6. planted variants, through the mapper's CPU oracle
def test_planted_variants_are_recovered():
    """A 3 kb text with ten planted variants (four SNVs, three insertions, three deletions, one deletion inside (AC) x 6 and one
    insertion inside T x 8), 900 reads of 100 bases, 30x (tests/variants_inputs.py::planted).  The oracle chain -- the affine
    mapper's CPU oracle, this call's oracle, vcf.write, vcf.parse, vcf.apply -- recovers 10 of 10, 100 %, with and without left
    alignment (the mapper's traceback already writes a gap at its leftmost column where nothing else disturbs the read), and
    the applied text is the sample's.  tests/test_variants_gpu.py runs the same reads through the GPU."""
    import map_affine_inputs as mai
    import map_affine_oracle as mao
    from poly_amd import vcf
    d = vi.planted()
    T = d["T"]
    assert len(T) == vi.PLANTED_LEN and len(d["reads"]) == vi.PLANTED_READS and len(d["variants"]) == 10
    assert [k for _, k, _ in d["variants"]] == [1, 2, 1, 3, 1, 2, 3, 1, 3, 2] and len(d["sample"]) == len(T) + 3 - 3 + 5 - 4 - 2 + 1
    hits, _ = mao.map_reads(T, d["reads"], mai.MAT, *mai.GAPS[0], mai.PARAMS)
    assert sum(h.flags & 1 for h in hits) == vi.PLANTED_READS
    A = [bytes(h.alignA) if h.flags & 1 else b"" for h in hits]
    B = [bytes(h.alignB) if h.flags & 1 else b"" for h in hits]
    off = np.zeros(len(hits) + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in A])
    for left_align in (1, 0):
        r = vo.call_variants([h.flags for h in hits], None, [h.ref_start for h in hits], [h.ref_end for h in hits], None, b"".join(A), b"".join(B),
                             off, None, None, T, left_align=left_align, **vi.PLANTED_CALL)
        assert r.info["bad"] == 0 and r.info["used"] == vi.PLANTED_READS
        rows = vcf.parse(vcf.write(_variants_of(r, T), T, "construct"))
        found = vi.called(rows)
        print(f"planted variants, left_align = {left_align}: {sum(x in found for x in d['variants'])} of {len(d['variants'])} recovered exactly")
        assert found == list(d["variants"]) and all(x.gt == 2 for x in rows)
        assert vcf.apply(T, rows) == d["sample"]
