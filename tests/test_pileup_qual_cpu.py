"""The CPU oracle of polyhip_pileup_qual (tests/pileup_qual_oracle.py) held to answers written out by hand, and the conditions
that tests/pileup_qual_inputs.py promises to tests/test_pileup_qual_gpu.py asserted on the inputs themselves."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import pileup_inputs as pi  # noqa: E402
import pileup_oracle as po  # noqa: E402
import pileup_qual_inputs as qi  # noqa: E402
import pileup_qual_oracle as qo  # noqa: E402

ARGS = ("flags", "mapq", "ref_start", "ref_end", "read_start", "alnA", "alnB", "aln_off", "qual", "qual_off")


@functools.lru_cache(maxsize=None)
def _run(name, k, min_base_qual):
    s = {x.name: x for x in qi.all_sets()}[name]
    p = qi.pack(s)
    return qo.pileup_qual(*[p[f] for f in ARGS], s.ref, **s.settings[k], min_base_qual=min_base_qual)


# ---------------------------------------------------------------- the oracle against answers by hand
REF = b"ACGTACGTAC"
#            text position     1 2     3 4 5 6 7                   4 5 6   7 8
FWD = dict(A=b"CGAAT--GC", B=b"CG--TACGT", ref_start=1, ref_end=8, read_start=2, flags=1,
           Q=[5, 6, 30, 10, 11, 12, 25, 40, 15, 7])      # two clipped bases in front, one behind; read index 2..8 is aligned
REV = dict(A=b"A-GTTA", B=b"ACG-TA", ref_start=4, ref_end=9, read_start=1, flags=3,
           Q=[3, 4, 35, 8, 2, 22, 41, 9])                # as sequenced: the oriented read's index x is 7 - x here


def _by_hand(min_base_qual):
    ents = (FWD, REV)
    off = np.cumsum([0] + [len(e["A"]) for e in ents]).astype(np.uint64)
    qoff = np.cumsum([0] + [len(e["Q"]) for e in ents]).astype(np.uint64)
    col = lambda f: [e[f] for e in ents]    # noqa: E731
    return qo.pileup_qual(col("flags"), None, col("ref_start"), col("ref_end"), col("read_start"), b"".join(col("A")), b"".join(col("B")), off,
                          bytes(33 + q for e in ents for q in e["Q"]), qoff, REF, min_base_qual=min_base_qual)


def _planes(shape, cells):
    out = np.zeros(shape, np.uint32)
    for (plane, pos), v in cells.items():
        out[plane, pos] = v
    return out


def test_oracle_against_answers_by_hand():
    # forward: C@1 Q30, G@2 Q10, insertion of two after 2, T@3 Q25, deletion of 4..5 after 3, G@6 Q40, C@7 Q15
    # reverse: A@4 Q41, deletion of 5 after 4, G@6 Q22, insertion of one after 6, T@7 Q8, A@8 Q35
    events = {(6, 2): 1, (7, 3): 1, (5, 4): 1, (5, 5): 1, (13, 5): 1, (15, 4): 1, (14, 6): 1}
    kept = {(1, 1): 30, (3, 3): 25, (2, 6): 40, (8 + 0, 4): 41, (8 + 2, 6): 22, (8 + 0, 8): 35}         # counts plane -> quality
    low = {(2, 2): 10, (1, 7): 15, (8 + 3, 7): 8}
    qplane = lambda ch: 4 * (ch // 8) + ch % 8    # noqa: E731
    for threshold, bases, filtered, consensus in ((0, {**kept, **low}, 0, b"NCGTA*GCAN"), (20, kept, 3, b"NCNTA*GNAN"),
                                                 (9, {**kept, (2, 2): 10, (1, 7): 15}, 1, b"NCGTA*GCAN"), (42, {}, 9, b"NNNN**NNNN")):
        r = _by_hand(threshold)
        want_counts = _planes((16, 10), {**events, **{c: 1 for c in bases}})
        want_qsum = _planes((8, 10), {(qplane(ch), p): q for (ch, p), q in bases.items()})
        assert (r.counts == want_counts).all(), threshold
        assert (r.qsum == want_qsum).all(), threshold
        assert r.consensus.tobytes() == consensus, (threshold, r.consensus.tobytes())
        assert list(r.err) == [0, 0]
        assert r.info == dict(entries=2, used=2, skipped_mapq=0, bad=0, columns=15, edge_events=0, sites=len(r.sites), filtered_bases=filtered)
    # position 4 has a forward deleted base and a reverse A: depth 2, the tie goes to the lower channel
    assert _by_hand(0).consensus[4] == ord("A")
    # G@6 on both strands: the two qualities stay apart
    assert _by_hand(0).qsum[2, 6] == 40 and _by_hand(0).qsum[6, 6] == 22
    # another offset: the same bytes read at offset 30 are three higher each
    ents = (FWD, REV)
    r = qo.pileup_qual([1, 3], None, [1, 4], [8, 9], [2, 1], FWD["A"] + REV["A"], FWD["B"] + REV["B"], [0, 9, 15],
                       bytes(33 + q for e in ents for q in e["Q"]), [0, 10, 18], REF, qual_offset=30)
    assert r.qsum[1, 1] == 33 and r.qsum[4, 4] == 44


def test_identity_with_pileup_oracle_at_threshold_zero():
    for s in qi.all_sets():
        if s.name in ("random", "quality_errs"):
            continue
        p = qi.pack(s)
        for k in range(len(s.settings)):
            a = _run(s.name, k, 0)
            b = po.pileup(*[p[f] for f in ("flags", "mapq", "ref_start", "ref_end", "alnA", "alnB", "aln_off")], s.ref, **s.settings[k])
            assert (a.counts == b.counts).all() and (a.consensus == b.consensus).all() and (a.err == b.err).all()
            assert a.site_list() == b.site_list() and {f: a.info[f] for f in b.info} == b.info and a.info["filtered_bases"] == 0


# ---------------------------------------------------------------- what the inputs hold
def test_every_pileup_set_is_there_with_qualities_attached():
    names = [s.name for s in qi.all_sets()]
    assert names[:-2] == [s.name for s in pi.all_sets()] and names[-2:] == ["quality_errs", "crossing"]
    for s, base in zip(qi.all_sets(), pi.all_sets()):
        assert s.entries is base.entries and s.ref is base.ref and s.settings is base.settings
        for e, lead, q in zip(s.entries, s.read_start, s.quals):
            assert len(q) >= lead + qi.read_columns(e.A) and all(qi.Q_LO <= x <= qi.Q_HI for x in q)
    assert (qi.Q_LO, qi.Q_HI) == (ord("!"), ord("J"))


def test_clips():
    lead_trail = set()
    for s in qi.all_sets():
        for e, lead, q in zip(s.entries, s.read_start, s.quals):
            if e.flags & pi.MAPPED and e.A:
                lead_trail.add((lead > 0, len(q) - lead - qi.read_columns(e.A) > 0))
    assert lead_trail == {(False, False), (False, True), (True, False), (True, True)}      # (False, False): m_i is the aligned length
    s = qi.quality_errs()
    e = s.entries[[x.name for x in s.entries].index("exact_length")]
    k = s.entries.index(e)
    assert s.read_start[k] == 0 and len(s.quals[k]) == qi.read_columns(e.A)


def test_read_index_crosses_a_step_inside_runs_on_both_strands():
    seen = set()
    for e, lead in zip(qi.crossing().entries, qi.crossing().read_start):
        cl = e.classes
        for c in "ID":
            at = cl.find(c * 20)
            if at >= 0:
                assert at < 64 < at + 20 and lead > 0                  # the run holds column 64
                assert cl[:at].count("I") + cl[:at].count("D") > 0    # the read index is not the column index there
                seen.add((c, bool(e.flags & pi.REVERSE)))
    assert seen == {("I", False), ("I", True), ("D", False), ("D", True)}
    assert all(e == 0 for e in _run("crossing", 0, 0).err)


def test_thresholds_filter_some_and_all():
    for s in qi.all_sets():
        if len(s.entries) < 2:
            continue
        none, some, every = (_run(s.name, 0, t) for t in qi.MIN_BASE_QUALS)
        bases = int(none.counts[[0, 1, 2, 3, 4, 8, 9, 10, 11, 12]].sum())
        assert none.info["filtered_bases"] == 0
        assert 0 < some.info["filtered_bases"] < every.info["filtered_bases"], s.name
        assert bases > 0 or s.settings[0]["region"] is not None
        if s.name == "quality_errs":       # the one set with a quality above 'J': range_ends_ok's Q = 93 passes any threshold
            assert int(every.counts[[0, 1, 2, 3, 4, 8, 9, 10, 11, 12]].sum()) == 1 and int(every.qsum.sum()) == 93
            continue
        # 42 is above every quality of the strings: no base is left, only deleted bases and events
        assert int(every.counts[[0, 1, 2, 3, 4, 8, 9, 10, 11, 12]].sum()) == 0 and int(every.qsum.sum()) == 0
        assert set(every.consensus.tobytes()) <= set(b"*N")
        assert (every.counts[[5, 6, 7, 13, 14, 15]] == none.counts[[5, 6, 7, 13, 14, 15]]).all()
    assert int(_run("shapes", 0, 42).counts[[5, 6, 7, 13, 14, 15]].sum()) > 0
    assert b"*" in _run("shapes", 0, 42).consensus.tobytes()


def test_quality_err_values():
    s = qi.quality_errs()
    r = _run("quality_errs", 0, 0)
    err = {e.name: int(x) for e, x in zip(s.entries, r.err)}
    assert err == dict(good=0, good_reverse=0, exact_length=0, err6_one_short=6, err6_one_short_reverse=6, err6_no_quality=6,
                       err6_read_start_beyond=6, err5_before_err6=5, err2_before_err6=2, err7_aligned_low=7, err7_leading_clip_only=7,
                       err7_trailing_clip_only=7, err7_reverse_clip_only=7, err6_before_err7=6, range_ends_ok=0,
                       err7_third_step_of_clip=7, long_ok=0, unmapped_bad_quality=0, low_mapq_bad_quality=7, err3_before_err6=3)
    by_name = {e.name: (e, lead, q) for e, lead, q in zip(s.entries, s.read_start, s.quals)}
    in_range = lambda x: qi.Q_LO <= x <= qi.Q_LO + 93    # noqa: E731
    for name in ("err7_leading_clip_only", "err7_trailing_clip_only", "err7_reverse_clip_only", "err7_third_step_of_clip"):
        e, lead, q = by_name[name]                       # the byte that raises err 7 lies in a clipped part only
        x0, x1 = lead, lead + qi.read_columns(e.A)
        aligned = q[len(q) - x1:len(q) - x0] if e.flags & pi.REVERSE else q[x0:x1]
        assert all(in_range(x) for x in aligned) and not all(in_range(x) for x in q), name
    assert len(by_name["err6_no_quality"][2]) == 0
    e, lead, q = by_name["err5_before_err6"]
    assert lead + qi.read_columns(e.A) > len(q)          # it qualifies for 6 as well
    assert len(by_name["err7_third_step_of_clip"][2]) > 128
    assert _run("quality_errs", 1, 0).err[[e.name for e in s.entries].index("low_mapq_bad_quality")] == 0       # skipped by min_mapq
    assert r.info["bad"] == sum(1 for v in err.values() if v) and r.info["used"] == 5
    q = by_name["range_ends_ok"][2]
    assert min(q) == qi.Q_LO and max(q) == qi.Q_LO + 93 and int(r.qsum.max()) >= 93


def test_contention_copies_carry_different_qualities():
    s = {x.name: x for x in qi.all_sets()}["contention"]
    assert len(s.entries) == 257 and len({e.A for e in s.entries}) == 1
    aligned = {q[lead:lead + qi.read_columns(e.A)] for e, lead, q in zip(s.entries, s.read_start, s.quals)}
    assert len(aligned) == 257
    r = _run("contention", 0, 20)
    first = s.entries[0].ref_start                        # a position all 257 cover with a base: some pass 20, some do not
    assert 0 < int(r.counts[:4, first].sum()) < 257 and int(_run("contention", 0, 0).counts[:4, first].sum()) == 257
