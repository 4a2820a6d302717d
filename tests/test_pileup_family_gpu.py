"""polyhip_pileup, polyhip_pileup_qual, polyhip_pileup_rows and polyhip_call_variants judge an entry alike: they share one entry
walk, one entry view and one staging of the entry arrays (csrc/pileup_walk.h), and this holds them to it.  On the input sets
whose entries take every path of the walk -- the column shapes (ends at 63 / 64 / 65 columns, runs that start at lane 0), every
err value, the events at the start of the text, the quality errs and the runs in which the read index crosses a step -- err must
be the same array from all three calls that take the arrays without qualities, and from all three that take them with
qualities, and so must what their last_info says about the entries.  Each call is compared with its own oracle elsewhere
(test_pileup_gpu.py, test_pileup_qual_gpu.py, test_pileup_rows_gpu.py, test_variants_gpu.py)."""
import functools
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import pileup_inputs as pi  # noqa: E402
import pileup_qual_inputs as qi  # noqa: E402

pytestmark = pytest.mark.gpu

SET_NAMES = ("shapes", "errs", "edges", "quality_errs", "crossing")
SHARED_INFO = ("used", "skipped_mapq", "bad", "columns")
MIN_MAPQ = (0, 20)                                # 20 is the sets' own threshold: it skips entries of shapes, errs and quality_errs
SKIPS_AT_20 = ("shapes", "errs", "quality_errs")  # the entries of edges and crossing all carry mapq 60


@functools.lru_cache(maxsize=None)
def _set(name) -> qi.QualSet:
    plain = {"shapes": pi.shapes, "errs": pi.errs, "edges": pi.edges}
    if name in plain:
        return qi.attach(plain[name](), SET_NAMES.index(name))
    return {"quality_errs": qi.quality_errs, "crossing": qi.crossing}[name]()


def _judgements(name, min_mapq, with_qual) -> dict:
    """call -> (err, the shared info counters) of the three calls that take the set's arrays with or without qualities"""
    from poly_amd import pileup, variants
    s = _set(name)
    p = qi.pack(s)
    core = (p["flags"], p["ref_start"], p["ref_end"])
    strings = (p["alnA"], p["alnB"], p["aln_off"])
    q = dict(read_start=p["read_start"], qual=p["qual"], qual_off=p["qual_off"]) if with_qual else {}
    out = {}
    if with_qual:
        got = pileup.pileup_qual_packed(*core, p["read_start"], *strings, p["qual"], p["qual_off"], s.ref, p["mapq"], min_mapq=min_mapq)
        out["polyhip_pileup_qual"] = got.err, pileup.last_qual_info()
    else:
        got = pileup.pileup_packed(*core, *strings, s.ref, p["mapq"], min_mapq=min_mapq)
        out["polyhip_pileup"] = got.err, pileup.last_info()
    got = pileup.rows_packed(*core, *strings, s.ref, b"seq1", p["mapq"], min_mapq=min_mapq, **q)
    out["polyhip_pileup_rows"] = got.err, pileup.last_rows_info()
    got = variants.call_packed(*core, *strings, s.ref, p["mapq"], min_mapq=min_mapq, **q)
    out["polyhip_call_variants"] = got.err, variants.last_info()
    return {call: (err.tolist(), {f: info[f] for f in SHARED_INFO}) for call, (err, info) in out.items()}


@pytest.mark.parametrize("with_qual", (False, True), ids=("plain", "qual"))
@pytest.mark.parametrize("min_mapq", MIN_MAPQ)
@pytest.mark.parametrize("name", SET_NAMES)
def test_the_calls_judge_an_entry_alike(name, min_mapq, with_qual):
    got = _judgements(name, min_mapq, with_qual)
    assert len(got) == 3
    (first, (err, info)), *others = got.items()
    n = len(_set(name).entries)
    assert len(err) == n and info["used"] + info["skipped_mapq"] + info["bad"] <= n
    assert (info["skipped_mapq"] > 0) == (min_mapq > 0 and name in SKIPS_AT_20), info
    for call, (e, i) in others:
        differ = [k for k in range(n) if e[k] != err[k]]
        assert not differ, f"{call} and {first} differ on entry {differ[0]} ({_set(name).entries[differ[0]].name}): {e[differ[0]]} / {err[differ[0]]}"
        assert i == info, (call, i, first, info)


def test_the_sets_reach_every_err():
    """what the comparison above stands on: between them the sets raise every err value the walks know, with the qualities'
    own (6 and 7) only where qualities are given"""
    seen = {q: set() for q in (False, True)}
    for name in SET_NAMES:
        for with_qual in (False, True):
            err, _ = next(iter(_judgements(name, 0, with_qual).values()))
            seen[with_qual] |= set(err)
    assert seen[False] == {0, 1, 2, 3, 5} and seen[True] == {0, 1, 2, 3, 5, 6, 7}, seen
