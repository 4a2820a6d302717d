"""polyhip_map_reads_affine on the GPU at the shapes tests/map_shapes.py builds, against its CPU oracle
(tests/map_affine_oracle.py, through tests/map_gap_shapes.py): all nine arrays, both aligned strings of every read and the six
shared counters are compared exactly, with no exclusions, at both gap settings of map_affine_inputs.GAPS.  With
gap_open == gap_extend == map_shapes.GAP the same call has to give the linear oracle's answer (map_shapes.expected).  That
each input reaches the branch it is named for is asserted in tests/test_map_shapes_cpu.py and
tests/test_map_gap_shapes_cpu.py."""
import os
import re
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_gap_shapes as mg  # noqa: E402
import map_shapes as ms  # noqa: E402
from map_check import COUNTERS, _assert_equal, _pack, _params, layout, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu

gaps = pytest.mark.parametrize("gaps", mg.GAPS + ((ms.GAP, ms.GAP),), ids=lambda g: f"{g[0]}_{g[1]}")
affine_gaps = pytest.mark.parametrize("gaps", mg.GAPS, ids=lambda g: f"{g[0]}_{g[1]}")


def _index(s, layout=None):
    from poly_amd import bwt
    index = bwt.New(s.T)
    if layout is not None:      # (a text that is not over ACGT has the general layout whatever is asked for)
        assert index.Layout() == ("nucleotide" if layout == "auto" and set(s.T) <= set(b"ACGT") else "general")
    return index


def _map(index, scoring, s, gaps, **kw):
    from poly_amd import mapper
    buf, offs = _pack(s.reads)
    return mapper.map_reads_affine_packed(index, scoring, *gaps, buf, offs, _params(s.P), max_len=s.max_len, **kw)


def _assert_info(info):
    """the six shared counters equal the oracle's, and every mapped read was traced, no other"""
    from poly_amd import mapper
    got = mapper.last_affine_info()
    assert {k: got[k] for k in COUNTERS} == {k: info[k] for k in COUNTERS}
    assert got["pairs_traced"] == got["reads_mapped"]
    return got


def _want(gaps, name, *args):
    """the affine oracle's answer; at equal gaps the linear oracle's"""
    if gaps[0] == gaps[1]:
        return ms.expected(name, *args)
    return mg.affine_expected(name, *args, go=gaps[0], ge=gaps[1])


def _check(scoring, gaps, name, *args, layout=None, **kw):
    s = ms.shape(name, *args)
    hits, info = _want(gaps, name, *args)
    index = _index(s, layout)
    got = _map(index, scoring, s, gaps, **kw)
    assert got.status == 0
    _assert_equal(got, hits)
    return index, got, _assert_info(info)


def _chunk_bytes(index, scoring, s, gaps):
    """what one chunk of 256 reads needs, as the error of a limit that is too small states it"""
    from poly_amd import _lib
    with pytest.raises(_lib.PolyhipError) as ei:
        _map(index, scoring, s, gaps, work_limit=1)
    assert ei.value.status == _lib.ERR_INVALID
    m = re.search(r"a chunk of (\d+) reads \((\d+) bytes\)", ei.value.message)
    assert m and int(m.group(1)) == min(len(s.reads), 256)
    return int(m.group(2))


# ---------------------------------------------------------------- 1. cluster length at the ballot width
@gaps
@pytest.mark.parametrize("max_occ", [4, ms.NO_LIMIT])
def test_ballot_width_clusters(layout, gaps, max_occ, nuc4_scoring):
    _check(nuc4_scoring, gaps, "ballot", max_occ, layout=layout)


# ---------------------------------------------------------------- 2. clusters many ballots long, windows of 900 columns
@gaps
def test_long_clusters(layout, gaps, nuc4_scoring):
    _check(nuc4_scoring, gaps, "long_clusters", layout=layout)


# ---------------------------------------------------------------- 3. max_cand windows of one read in one wave, band 0
@gaps
@pytest.mark.parametrize("max_cand", [64, 63, 5, 1])
def test_more_clusters_than_lanes(layout, gaps, max_cand, nuc4_scoring):
    """64 windows of about 60 columns per read in the score pass, `second` over 63 losers, the winner's traceback window"""
    _check(nuc4_scoring, gaps, "many_clusters", max_cand, layout=layout)


# ---------------------------------------------------------------- 4. text ends and the band limit
@gaps
def test_text_shorter_than_the_read(layout, gaps, nuc4_scoring):
    _check(nuc4_scoring, gaps, "short_text", layout=layout)


@gaps
def test_band_zero_at_the_text_ends(layout, gaps, nuc4_scoring):
    _check(nuc4_scoring, gaps, "band0_ends", layout=layout)


def test_both_limits_in_one_call(layout, nuc4_scoring):
    """max_len 4096 with band LIMITS_BAND, the forward read only, gaps (-12, -2)"""
    go, ge = mg.LIMITS_GAPS
    s = mg.limits_forward(mg.LIMITS_BAND)
    hits, info = mg.cut_expected("limits_forward", mg.LIMITS_BAND, go=go, ge=ge)
    assert s.max_len == 4096 == len(s.reads[0]) and len(s.reads) == 1
    got = _map(_index(s, layout), nuc4_scoring, s, (go, ge))
    assert got.status == 0
    _assert_equal(got, hits)
    _assert_info(info)


# ---------------------------------------------------------------- 5. max_len given by the caller
@gaps
@pytest.mark.parametrize("name", ["max_len_exceeded", "max_len_generous", "max_len_below_seed"])
def test_max_len_of_the_caller(layout, gaps, name, nuc4_scoring):
    _check(nuc4_scoring, gaps, name, layout=layout)


# ---------------------------------------------------------------- 6. alphabet
@gaps
def test_error_of_the_text_at_rank_3(layout, gaps, nuc4_scoring):
    index, _, _ = _check(nuc4_scoring, gaps, "text_error_rank3", layout=layout)
    assert index.Layout() == "general"   # (the N: the text is not over ACGT)


@gaps
def test_zero_bytes(layout, gaps, nuc4_scoring):
    _check(nuc4_scoring, gaps, "zero_bytes", layout=layout)


@affine_gaps
def test_mixed_case(gaps):
    s = ms.shape("mixed_case")
    hits, info = mg.affine_expected("mixed_case", go=gaps[0], ge=gaps[1])
    index = _index(s)
    assert index.Layout() == "general"
    got = _map(index, mg.case_mat().scoring(), s, gaps)
    assert got.status == 0
    _assert_equal(got, hits)
    _assert_info(info)


# ---------------------------------------------------------------- 7. min_score on the boundary
@gaps
@pytest.mark.parametrize("above", [0, 1])
def test_min_score_on_the_boundary(layout, gaps, above, nuc4_scoring):
    """a bound equal to the winner's score under these gaps, read off the oracle, and that score + 1"""
    bound = _want(gaps, "min_score", 1)[0][0].score + above
    _, got, info = _check(nuc4_scoring, gaps, "min_score", bound, layout=layout)
    assert info["reads_mapped"] == 1 - above and bool(got.flags[0] & 1) == (not above)


# ---------------------------------------------------------------- 8. a chunk without hits between two with hits
@gaps
def test_a_whole_chunk_without_hits(layout, gaps, nuc4_scoring):
    s = ms.shape("empty_middle_chunk")
    index = _index(s, layout)
    need = _chunk_bytes(index, nuc4_scoring, s, gaps)
    _, got, info = _check(nuc4_scoring, gaps, "empty_middle_chunk", layout=layout, work_limit=need)
    assert info["chunks"] == 3 and info["tb_chunks"] == 2          # the middle chunk traced nothing
    assert (got.aln_off[256:513] == got.aln_off[256]).all() and 0 < got.aln_off[256] < got.aln_off[-1]


# ---------------------------------------------------------------- 9. a winner of more than 32 bands of 32 rows
@gaps
def test_winner_of_2000_rows(layout, gaps, nuc4_scoring):
    s = mg.le2048_first3()
    if gaps[0] == gaps[1]:
        hits, info = ms.oracle_map(s.T, s.reads, ms.matrix(s.matrix), ms.GAP, s.P, s.max_len)
    else:
        hits, info = mg.cut_expected("le2048_first3", go=gaps[0], ge=gaps[1])
    got = _map(_index(s, layout), nuc4_scoring, s, gaps)
    assert got.status == 0 and got.read_end[0] - got.read_start[0] > 32 * 32
    _assert_equal(got, hits)
    _assert_info(info)
