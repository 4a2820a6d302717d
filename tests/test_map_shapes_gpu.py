"""The read mapper on the GPU at the shapes tests/map_shapes.py builds, against its CPU oracle (tests/map_oracle.py): as in
tests/test_map_gpu.py every output array, both aligned strings of every read and the info counters are compared exactly,
with no exclusions.  That each input reaches the branch it is named for is asserted in tests/test_map_shapes_cpu.py.
Every case runs through the host flavour (polyhip_map_reads); `dev=True` runs it through polyhip_map_reads_dev as well."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_shapes as ms  # noqa: E402
from map_check import COUNTERS, _Dev, _assert_equal, _assert_info, _pack, _params, layout, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case_scoring():
    from poly_amd import align, alphabet, matrix
    a = alphabet.NewAlphabet(list(ms.CASE_ALPHABET))
    return align.NewScoring(matrix.NewSubstitutionMatrix(a, a, ms.case_scores()), ms.GAP)


def _index(s, layout=None):
    from poly_amd import bwt
    index = bwt.New(s.T)
    if layout is not None:
        assert index.Layout() == ("nucleotide" if layout == "auto" else "general")
    return index


def _host(index, scoring, s, **kw):
    from poly_amd import mapper
    buf, offs = _pack(s.reads)
    return mapper.map_reads_packed(index, scoring, buf, offs, _params(s.P), max_len=s.max_len, **kw)


def _check(scoring, name, *args, layout=None, dev=False):
    """shape(name, *args) through the host flavour (and the device flavour): everything equals the oracle's answer"""
    s = ms.shape(name, *args)
    hits, info = ms.expected(name, *args)
    index = _index(s, layout)
    got = _host(index, scoring, s)
    assert got.status == 0
    _assert_equal(got, hits)
    _assert_info(info)
    if dev:
        got = _Dev(index, scoring, s.reads, s.P, max_len=s.max_len)
        assert got.status == 0
        _assert_equal(got, hits)
        _assert_info(info)
    return index


# ---------------------------------------------------------------- 1. cluster length at the ballot width
def test_ballot_width_clusters(layout, nuc4_scoring):
    """one cluster of 63, 64, 65, 127, 128, 129 hits per read: map_cluster_kernel's counting loop ends after a partial
    ballot, after an empty one (a multiple of 64: the last read's ends with the hit array) and after one more hit"""
    _check(nuc4_scoring, "ballot", layout=layout, dev=True)


# ---------------------------------------------------------------- 2. clusters many ballots long, traceback path 7
def test_long_clusters(layout, nuc4_scoring):
    from poly_amd import align
    _check(nuc4_scoring, "long_clusters", layout=layout)
    assert align.sw_traceback_last_path() == 7


# ---------------------------------------------------------------- 3. more clusters than lanes
@pytest.mark.parametrize("max_cand", [64, 63, 5, 1])
def test_more_clusters_than_lanes(layout, max_cand, nuc4_scoring):
    """hundreds of clusters per read through the 64 rank-per-lane slots: insertion at lane 0 in mid-stream, candidates
    falling off the last lane, equal votes across the cut decided by (strand, d0); band 0"""
    _check(nuc4_scoring, "many_clusters", max_cand, layout=layout, dev=True)


# ---------------------------------------------------------------- 4. text ends and the band limit
def test_text_shorter_than_the_read(layout, nuc4_scoring):
    _check(nuc4_scoring, "short_text", layout=layout)


def test_band_zero_at_the_text_ends(layout, nuc4_scoring):
    _check(nuc4_scoring, "band0_ends", layout=layout)


def test_both_limits_in_one_call(nuc4_scoring):
    """max_len 4096 with band 1024 (halved while the workspace is above 4 GiB); the workspace is printed"""
    from poly_amd import mapper
    index = _index(ms.shape("limits"))
    band = 1024
    while True:
        s = ms.shape("limits", band)
        work = mapper.workspace_bytes(index, nuc4_scoring, _params(s.P), len(s.reads), s.max_len)
        print(f"max_len {s.max_len}, band {band}, {len(s.reads)} reads, max_cand {s.P.max_cand}: workspace {work} bytes")
        if work <= 4 << 30:
            break
        band //= 2
    assert work > 0 and band >= 1
    _check(nuc4_scoring, "limits", band)


# ---------------------------------------------------------------- 5. max_len given by the caller
@pytest.mark.parametrize("name", ["max_len_exceeded", "max_len_generous", "max_len_below_seed"])
def test_max_len_of_the_caller(layout, name, nuc4_scoring):
    _check(nuc4_scoring, name, layout=layout, dev=True)


# ---------------------------------------------------------------- 6. off[0] != 0
def test_offsets_not_starting_at_zero(nuc4_scoring):
    from poly_amd import mapper
    s = ms.shape("offset_base")
    hits, info = ms.expected("offset_base")
    index = _index(s)
    buf, offs = ms.offset_packed()
    got = mapper.map_reads_packed(index, nuc4_scoring, buf, offs, _params(s.P))
    assert got.status == 0 and int(got.aln_off[0]) == 0
    _assert_equal(got, hits)
    _assert_info(info)
    got = _Dev(index, nuc4_scoring, s.reads, s.P, packed=(buf, offs))
    assert got.status == 0 and int(got.aln_off[0]) == 0
    _assert_equal(got, hits)
    _assert_info(info)


# ---------------------------------------------------------------- 7. alphabet
def test_error_of_the_text_at_rank_3(nuc4_scoring):
    index = _check(nuc4_scoring, "text_error_rank3")
    assert index.Layout() == "general"   # (the N: the text is not over ACGT)


def test_zero_bytes(nuc4_scoring):
    _check(nuc4_scoring, "zero_bytes")


def test_mixed_case(case_scoring):
    index = _check(case_scoring, "mixed_case")
    assert index.Layout() == "general"


# ---------------------------------------------------------------- 8. min_score on the boundary
@pytest.mark.parametrize("bound", [700, 701])
def test_min_score_on_the_boundary(bound, nuc4_scoring):
    _check(nuc4_scoring, "min_score", bound)


# ---------------------------------------------------------------- 9. a chunk without hits between two with hits
def test_a_whole_chunk_without_hits(nuc4_scoring):
    """768 reads in chunks of 256 (a workspace of 0.34 of the full one); the middle chunk has no hit at all.  With strings,
    without, and with one byte of string capacity too few"""
    from poly_amd import _lib
    s = ms.shape("empty_middle_chunk")
    hits, info = ms.expected("empty_middle_chunk")
    index = _check(nuc4_scoring, "empty_middle_chunk")
    whole = _Dev(index, nuc4_scoring, s.reads, s.P)
    _assert_equal(whole, hits)
    assert _assert_info(info)["chunks"] == 1

    def third(full):
        return int(full * 0.34)

    got = _Dev(index, nuc4_scoring, s.reads, s.P, work_bytes=third)
    assert got.status == 0
    _assert_equal(got, hits)
    assert _assert_info(info)["chunks"] == 3
    assert (got.aln_off == whole.aln_off).all()
    got = _Dev(index, nuc4_scoring, s.reads, s.P, work_bytes=third, strings=False)
    assert got.status == 0 and got.alignA is None
    _assert_equal(got, hits, strings=False)
    assert _assert_info(info)["chunks"] == 3
    needed = sum(len(h.alignA) for h in hits)
    assert int(whole.aln_off[-1]) == needed
    got = _Dev(index, nuc4_scoring, s.reads, s.P, work_bytes=third, capacity=needed - 1)
    assert got.status == _lib.ERR_INVALID
    assert (got.aln_off == whole.aln_off).all()
    _assert_equal(got, hits, strings=False)
    assert _assert_info(info)["chunks"] == 3


# ---------------------------------------------------------------- 10. more pairs than one traceback workspace
def test_traceback_fork(nuc4_scoring):
    """36,000 reads (500 distinct ones, 72 times) with four candidates each: 144,000 pairs in ONE chunk of the mapper, whose
    traceback workspace holds MAP_TB_PAIRS = 131,072.  In traceback_impl (sw_traceback.hip) that is `npairs > chunk` on
    PATH_WAVE with `half_chunk` = 65,536 >= 16,384, so `overlap` is true: the chunks of 65,536 pairs alternate between the
    caller's stream and the library's (`aux.fork`, `st = (chunk_no & 1) ? aux.s : caller_st`, `aux.join`), and
    map_reduce_kernel then reads the string slots both streams wrote.  The 2.2 million hits also take this translation
    unit's radix histogram scan (256 counters per 4,096 hits) through its recursive level."""
    from poly_amd import align, mapper
    s = ms.shape("traceback_fork")
    hits, info = ms.expected("traceback_fork")
    index = _index(s)
    buf, offs = _pack(s.reads * s.tile)
    got = mapper.map_reads_packed(index, nuc4_scoring, buf, offs, _params(s.P))
    assert got.status == 0
    _assert_equal(got, hits * s.tile)
    have = _assert_info({k: info[k] * s.tile for k in COUNTERS})
    print(f"{len(offs) - 1} reads, tiling {s.tile}: {have}")
    assert have["pairs_aligned"] > ms.TB_PAIRS + 4096 and have["hits"] > 65_536 and have["chunks"] == 1
    assert align.sw_traceback_last_path() == 4


# ---------------------------------------------------------------- 11. max_occ = 0xFFFFFFFF: no limit
def test_max_occ_without_limit(layout, nuc4_scoring):
    from poly_amd import mapper
    _check(nuc4_scoring, "ballot", ms.NO_LIMIT, layout=layout, dev=True)
    assert mapper.last_info()["seeds_over_max_occ"] == 0


# ---------------------------------------------------------------- 12. the traceback kernel by read length
@pytest.mark.parametrize("name", list(ms.TB_CLASSES))
def test_traceback_by_read_length(name, nuc4_scoring):
    from poly_amd import align
    s = ms.shape("traceback_class", name)
    if name == "le152":
        assert max(len(r) for r in s.reads) <= 152
    _check(nuc4_scoring, "traceback_class", name)
    assert align.sw_traceback_last_path() == s.note["path"]
