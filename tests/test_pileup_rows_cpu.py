"""The CPU oracle of polyhip_pileup_rows (tests/pileup_rows_oracle.py) held to rows written out by hand, to the parser of
poly_amd/pileup_text.py and to the depth and event counts of tests/pileup_oracle.py; poly_amd/pileup_text.py pinned on the
reference's own fixtures (tests/golden/pileup/); and the conditions that tests/pileup_rows_inputs.py promises to
tests/test_pileup_rows_gpu.py asserted on the inputs themselves.

Two things the format itself decides: the row of a position without reads (``all_positions``) reads ``0 \\t * \\t *``, so the
parser gives it one read result and one quality byte, both the placeholder ``*``: such rows are held to exactly that, every
other row to ``len(quality) == read_count`` and ``len(read_results) == read_count + runs``.  And the reference's
``test.pileup`` holds 20 lines, the third with a read count of 1401: 20 rows is what it parses to."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import pileup_oracle as po  # noqa: E402
import pileup_qual_inputs as qi  # noqa: E402
import pileup_rows_inputs as ri  # noqa: E402
import pileup_rows_oracle as ro  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "pileup")
ARGS = ("flags", "mapq", "ref_start", "ref_end", "read_start", "alnA", "alnB", "aln_off", "qual", "qual_off")


def _pileup_text():
    """poly_amd/pileup_text.py on its own: importing the package would load the library, which a CPU test does not need"""
    spec = importlib.util.spec_from_file_location("pileup_text_alone", os.path.join(os.path.dirname(HERE), "poly_amd", "pileup_text.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


pt = _pileup_text()
SETS = {s.name: s for s in ri.all_sets()}
CASES = [(s.name, k, q) for s in ri.all_sets() for k in range(len(s.settings)) for q in (True, False)]


@functools.lru_cache(maxsize=None)
def _run(name, k, with_qual):
    s = SETS[name]
    st = s.settings[k]
    p, kw = ri.arguments(s, st, with_qual)
    return ro.pileup_rows(*[p[f] for f in ARGS], s.qs.ref, st["name"], order=p["order"], **kw)


# ---------------------------------------------------------------- the oracle against rows by hand
REF = b"TACGTAC\x07TGAC"
HAND = (  # flags, mapq, ref_start, ref_end, read_start, A, B, quality as sequenced
    (1, 80, 2, 3, 0, b"C", b"C", b"I"),                       # one text column: ^q.$
    (1, 200, 2, 5, 1, b"CAC-T", b"C--GT", b"!5678#"),         # .+2AC-1G behind '^' and a mapq of 200; the D column borrows the next base's '8'
    (1, 60, 5, 8, 0, b"A-T\x07", b"AC-\x07", b"ABC"),         # .-1C, then *+1T; the text byte 0x07 prints as N
    (3, 60, 0, 5, 0, b"T---T", b"TACGT", b"XY"),              # reverse: ,-3acg; sequenced index 1 - x
    (1, 60, 10, 11, 0, b"GGA", b"--A", b"abc"),               # a run that opens the entry: dropped
    (1, 60, 8, 10, 0, b"cG", b"TG", b"JJ"),                   # a mismatch in lower case on the forward strand prints upper case
)
ROWS = (b"s\t1\tT\t1\t^],-3acg\tY\n", b"s\t2\tA\t1\t*\tX\n", b"s\t3\tC\t3\t^q.$^~.+2AC-1G*\tI5X\n", b"s\t4\tG\t2\t**\t8X\n",
        b"s\t5\tT\t2\t.$,$\t8X\n", b"s\t6\tA\t1\t^].-1C\tA\n", b"s\t7\tC\t1\t*+1T\tB\n", b"s\t8\tN\t1\t.$\tC\n", b"s\t9\tT\t1\t^]C\tJ\n",
        b"s\t10\tG\t1\t.$\tJ\n", b"s\t11\tA\t1\t^].$\tc\n", b"s\t12\tC\t0\t*\t*\n")


def _hand(**kw):
    off = np.cumsum([0] + [len(e[5]) for e in HAND]).astype(np.uint64)
    qoff = np.cumsum([0] + [len(e[7]) for e in HAND]).astype(np.uint64)
    col = lambda k: [e[k] for e in HAND]    # noqa: E731
    qual = kw.pop("qual", b"".join(col(7)))
    mapq = kw.pop("mapq", col(1))
    return ro.pileup_rows(col(0), mapq, col(2), col(3), col(4), b"".join(col(5)), b"".join(col(6)), off, qual, qoff, REF, b"s", **kw)


def test_rows_by_hand():
    got = _hand(all_positions=1)
    assert got.text == b"".join(ROWS)
    assert list(got.err) == [0] * 6 and list(got.row_off) == list(np.cumsum([0] + [len(r) for r in ROWS]))
    assert got.info == dict(entries=6, used=6, skipped_mapq=0, bad=0, columns=20, tokens=15, rows=12, text_bytes=len(got.text),
                            dropped_events=1, max_row_bytes=len(ROWS[2]))
    sparse = _hand()
    assert sparse.text == b"".join(ROWS[:11]) and sparse.row_off[11] == sparse.row_off[12] and sparse.info["rows"] == 11


def test_rows_by_hand_order_region_and_origin():
    got = _hand(order=[5, 4, 3, 2, 1, 0], region=(2, 5), pos_origin=2)
    assert got.text == b"s\t1\tC\t3\t*^~.+2AC-1G^q.$\tX5I\ns\t2\tG\t2\t**\tX8\ns\t3\tT\t2\t,$.$\tX8\n"
    assert got.info["dropped_events"] == 1 and got.info["tokens"] == 7      # the dropped run counts whatever the region
    # the anchor inside the region and the deleted bases outside, and the converse
    assert _hand(region=(0, 1)).text == ROWS[0] and _hand(region=(1, 2)).text == ROWS[1]


def test_rows_by_hand_without_qualities_or_mapq():
    got = _hand(qual=None, mapq=None)
    assert got.rows[2] == b"s\t3\tC\t3\t^~.$^~.+2AC-1G*\t~~~\n" and got.rows[0] == b"s\t1\tT\t1\t^~,-3acg\t~\n"
    other = _hand(qual=bytes(x + 31 for e in HAND for x in e[7]), qual_offset=64)      # the output stays at offset 33
    assert other.text == _hand().text


def test_quality_errors_follow_the_quality_pileup():
    short = list(HAND)
    short[1] = short[1][:7] + (b"!567",)                     # read_start 1 + 4 read bases > 4
    off = np.cumsum([0] + [len(e[5]) for e in short]).astype(np.uint64)
    qoff = np.cumsum([0] + [len(e[7]) for e in short]).astype(np.uint64)
    col = lambda k: [e[k] for e in short]    # noqa: E731
    a = (col(0), col(1), col(2), col(3), col(4), b"".join(col(5)), b"".join(col(6)), off)
    got = ro.pileup_rows(*a, b"".join(col(7)), qoff, REF, b"s")
    assert list(got.err) == [0, 6, 0, 0, 0, 0] and got.rows[2] == b"s\t3\tC\t2\t^q.$*\tIX\n"
    assert list(ro.pileup_rows(*a, None, None, REF, b"s").err) == [0] * 6            # without qualities there is no err 6


# ---------------------------------------------------------------- every row parses; depth and events are the counts'
@pytest.mark.parametrize("name,k,with_qual", CASES)
def test_rows_parse_and_agree_with_the_counts(name, k, with_qual):
    s, got = SETS[name], _run(name, k, with_qual)
    st = s.settings[k]
    p, kw = ri.arguments(s, st, with_qual)
    lo, hi = st["region"] or (0, len(s.qs.ref))
    parsed = pt.parse(got.text)
    assert got.info["max_row_bytes"] <= pt.MAX_LINE_SIZE and len(parsed) == got.info["rows"] == len(got.rows)
    if not any(r[0] in "+-" and r[2:3].isdigit() for x in parsed for r in x.read_results):      # a run of 10 or more does not round-trip
        assert pt.write_pileups(parsed) == got.text
    by_pos = {x.position - 1 + st["pos_origin"]: x for x in parsed}
    assert len(by_pos) == len(parsed)
    for pos, x in by_pos.items():
        assert x.sequence == st["name"].decode("latin-1")
        if x.read_count == 0:                              # the row of a position without reads: the format's two placeholders
            assert st["all_positions"] == 1 and x.read_results == ["*"] and x.quality == "*"
            continue
        assert len(x.quality) == x.read_count
        assert len(x.read_results) == x.read_count + got.runs.get(pos, 0), pos
    if with_qual:
        return                                             # err 6 and 7 leave entries out that the plain pileup counts
    counts = po.pileup(p["flags"], p["mapq"], p["ref_start"], p["ref_end"], p["alnA"], p["alnB"], p["aln_off"], s.qs.ref, region=(lo, hi),
                       min_mapq=st["min_mapq"])
    assert (counts.err == got.err).all()
    depth = counts.counts[0:6].sum(axis=0) + counts.counts[8:14].sum(axis=0)
    plus = minus = 0
    for j in range(hi - lo):
        x = by_pos.get(lo + j)
        assert (x.read_count if x else 0) == depth[j], (j, depth[j])
        assert (x is not None) == (depth[j] > 0 or st["all_positions"] == 1)
        ins = sum(r[0] == "+" for r in x.read_results) if x else 0
        dels = sum(r[0] == "-" for r in x.read_results) if x else 0
        plus, minus = plus + ins, minus + dels
        ch6, ch7 = int(counts.counts[6, j]) + int(counts.counts[14, j]), int(counts.counts[7, j]) + int(counts.counts[15, j])
        if got.info["dropped_events"] == 0:
            assert (ins, dels) == (ch6, ch7), j
        else:
            assert ins <= ch6 and dels <= ch7, j
    if st["region"] is None:                               # the runs that open an entry: the counts keep all but those anchored at -1
        events = int(counts.counts[[6, 7, 14, 15]].sum())
        assert events + counts.info["edge_events"] == plus + minus + got.info["dropped_events"]
    assert {f: got.info[f] for f in ("entries", "used", "skipped_mapq", "bad", "columns")} == {
        f: counts.info[f] for f in ("entries", "used", "skipped_mapq", "bad", "columns")}


def test_edges_differ_by_the_dropped_runs():
    got = _run("edges", 0, False)
    assert got.info["dropped_events"] == 7                 # i_first, d_first at 0 and at 1, i_only, and the I and the D of i_d
    p, _ = ri.arguments(SETS["edges"], SETS["edges"].settings[0], False)
    counts = po.pileup(p["flags"], p["mapq"], p["ref_start"], p["ref_end"], p["alnA"], p["alnB"], p["aln_off"], SETS["edges"].qs.ref)
    assert counts.info["edge_events"] == 5 and int(counts.counts[[6, 7, 14, 15]].sum()) == 2        # the two entries at 1 keep theirs, at 0
    assert not any(r[0] in "+-" for x in pt.parse(got.text) for r in x.read_results)


# ---------------------------------------------------------------- pileup_text on the reference's fixtures
def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as fh:
        return fh.read()


def test_pileup_text_reads_and_writes_the_fixture():
    data = _golden("test.pileup")
    rows = pt.parse(data)
    assert data.count(b"\n") == 20 and data.endswith(b"\n")          # the fixture holds 20 lines, so 20 rows is all a parser can give
    assert len(rows) == 20 and rows[2].read_count == 1401 and rows[0].sequence and isinstance(rows[0].position, int)
    assert pt.write_pileups(rows) == data
    assert len(pt.parse_n(data, 2)) == 2 and pt.parse_n(data, 2) == rows[:2]
    assert pt.read(os.path.join(GOLDEN, "test.pileup")) == rows
    with pytest.raises(OSError):
        pt.read(os.path.join(GOLDEN, "DOESNT_EXIST.pileup"))


def test_pileup_text_write_and_read_back(tmp_path):
    rows = pt.parse(_golden("test.pileup"))
    path = tmp_path / "tmp.pileup"
    pt.write(rows, path)
    assert path.read_bytes() == _golden("test.pileup") and pt.read(path) == rows


@pytest.mark.parametrize("name,message", [("test_not_enough_fields.pileup", "values, expected 6."), ("test_position_non_int.pileup", "Error on line"),
                                          ("test_readcount_non_int.pileup", "Error on line"),
                                          ("test_read_off.pileup", "Rune within +,- not found on line"),
                                          ("test_unknown_rune.pileup", "Rune not found on line")])
def test_pileup_text_refuses_the_broken_fixtures(name, message):
    with pytest.raises(pt.PileupError, match=message.replace("+", r"\+").replace(".", r"\.")):
        pt.parse(_golden(name))


def test_pileup_text_quirks():
    row = pt.parse(b"s\t7\tA\t4\t^I.$,+2AC-1g*\tIIII\n")[0]
    assert row.read_results == ["^I.$", ",", "+2AC", "-1g", "*"] and (row.position, row.read_count, row.quality) == (7, 4, "IIII")
    assert pt.parse(b"s\t1\tA\t1\t.\tI\ns\t2\tA\t1\t.\tI") == pt.parse(b"s\t1\tA\t1\t.\tI\n")       # no newline: dropped, no error
    long = b"s\t1\tA\t1\t." + b"\tI" + b"I" * 70000 + b"\n"
    with pytest.raises(pt.PileupError, match="buffer full"):
        pt.parse(long)
    assert len(pt.parse(long, max_line_size=len(long))) == 1
    with pytest.raises(pt.PileupError) as e:
        pt.parse(b"s\t1\tA\t1\t.\tI\nbroken\n")
    assert len(e.value.rows) == 1                          # the rows before the error come with it
    ten = pt.parse(b"s\t1\tA\t1\t.+10ACGTACGTAC.\tII\n")[0]   # the reference slices n + 2 bytes: a run of 10 loses its last letter
    assert ten.read_results == [".", "+10ACGTACGTA", "."]


# ---------------------------------------------------------------- what the input sets are there for
def test_the_existing_sets_are_all_here():
    assert tuple(s.name for s in ri.existing_sets()) == tuple(s.name for s in qi.all_sets())
    assert tuple(s.name for s in ri.own_sets()) == ("run_lengths", "digits", "depths", "tokens")
    for s, q in zip(ri.existing_sets(), qi.all_sets()):
        assert s.qs is q and {(st["region"], st["min_mapq"]) for st in s.settings} == {(st["region"], st["min_mapq"]) for st in q.settings}
        assert {st["all_positions"] for st in s.settings} == {0, 1}


def _tokens_of(got):
    return [r for x in pt.parse(got.text) for r in x.read_results]


def test_run_lengths_set():
    got = _run("run_lengths", 0, True)
    toks = got.text
    for k in ri.RUN_LENGTHS:
        assert b"+%d" % k in toks and b"-%d" % k in toks
    assert not got.err.any() and got.info["dropped_events"] == 0
    both = [r for r in got.rows.values() if any(b"+%d" % k in r and b"-%d" % k in r for k in ri.RUN_LENGTHS)]
    assert both                                            # an I run and the D run behind it in one token
    assert {e.flags for e in SETS["run_lengths"].qs.entries} == {1, 3}


def test_digits_set():
    s = SETS["digits"]
    printed = lambda k: [int(r.split(b"\t")[1]) for r in _run("digits", k, True).rows.values()]    # noqa: E731
    assert {9, 10, 99, 100, 999, 1000} <= set(printed(0)) and 1100 in printed(0) and printed(1) == list(range(1, 1101))
    assert s.settings[3]["pos_origin"] == 900 and {99, 100} <= set(printed(3)) and 1000 not in printed(3)
    assert printed(4) == list(range(6, 16)) and printed(5)[0] == 1
    assert all(st["pos_origin"] <= (st["region"] or (0, 0))[0] for st in s.settings)


def test_depths_set():
    s = SETS["depths"]
    assert len(s.qs.entries) == sum(d for _, d in ri.DEPTHS) and [d for _, d in ri.DEPTHS] == [9, 10, 99, 100, 300]
    orders = [st["order"] for st in s.settings]
    n = len(s.qs.entries)
    assert orders[0] is None and orders[2] == tuple(range(n)) and orders[3] == tuple(reversed(range(n))) and sorted(orders[1]) == list(range(n))
    assert orders[1] not in (orders[2], orders[3])
    texts = [_run("depths", k, True).text for k in range(4)]
    assert texts[0] == texts[2] and len({texts[0], texts[1], texts[3]}) == 3      # the order of the reads shows in the bytes
    for p, d in ri.DEPTHS:
        row = pt.parse(_run("depths", 0, True).rows[p])[0]
        assert row.read_count == d and len(set(zip(row.read_results, row.quality))) >= min(d, 180)     # reads of a row differ
        rev = pt.parse(_run("depths", 3, True).rows[p])[0]
        assert rev.read_results == row.read_results[::-1] and rev.quality == row.quality[::-1]


def test_tokens_set():
    s = SETS["tokens"]
    got = _run("tokens", 0, True)
    toks = _tokens_of(got)
    assert "^q.$" in toks and any(t.startswith("^") and t.endswith("$") and t[2] in "acgtn" for t in toks)      # head and tail in one token
    assert got.rows[5].split(b"\t")[4] in (b"^]*", b"^]*$") and b"^]*" in got.rows[6]                           # entries of D columns only
    assert any(t[0] == "+" for t in toks) and any(t[0] == "-" for t in toks) and not got.err.any()
    by = {st["region"]: _run("tokens", k, True) for k, st in enumerate(s.settings) if st["region"] and st["all_positions"] == 0 and st["region"][1] > 0}
    assert b"-3" in by[(13, 14)].text and by[(13, 14)].info["tokens"] == 1        # the anchor inside, the deleted bases outside
    assert b"-3" not in by[(14, 17)].text and by[(14, 17)].text.count(b"*") >= 3  # the converse
    assert b"+2" in by[(33, 34)].text and b"+2" not in by[(34, 40)].text
    names = [st["name"] for st in s.settings]
    assert any(len(x) == 1 for x in names) and any(len(x) == 255 for x in names)
    assert all(0x21 <= c <= 0x7e for x in names for c in x)
    firsts = got.rows[20].split(b"\t")[4]
    assert firsts == b"^!.^~.^~.^~."                                              # mapq 0, 93, 94, 255
    null = _run("tokens", [st["mapq_null"] for st in s.settings].index(True), True)
    assert null.rows[20].split(b"\t")[4] == b"^~.^~.^~.^~." and b"^q" not in null.text
    k64 = [st["qual_offset"] for st in s.settings].index(64)
    assert s.settings[k64]["rebase"] == 31 and _run("tokens", k64, True).text == got.text
    skipped = _run("tokens", [st["min_mapq"] for st in s.settings].index(94), True)
    assert skipped.info["used"] == 2 and skipped.info["skipped_mapq"] == len(s.qs.entries) - 2
    empty = {st["all_positions"]: _run("tokens", k, True) for k, st in enumerate(s.settings) if st["region"] == (78, 80)}
    assert empty[0].text == b"" and empty[0].info["tokens"] == 0 and empty[1].info["rows"] == 2 and empty[1].text.count(b"\t0\t*\t*\n") == 2
    assert _run("tokens", [st["region"] for st in s.settings].index((0, 0)), True).row_off.tolist() == [0]
    assert got.info["max_row_bytes"] == max(len(r) for r in got.rows.values())
