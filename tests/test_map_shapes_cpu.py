"""The inputs of tests/map_shapes.py reach the conditions they are named for -- asserted on the CPU oracle alone, so that
tests/test_map_shapes_gpu.py is known to take the mapper's kernels through those branches: clusters of exactly 63 / 64 /
65 / 127 / 128 / 129 hits, clusters many ballots long, more clusters than a wave has lanes with ties across the cut, the
ranks and error codes of the alphabet cases, the thresholds of the chunked and the forking call."""
import dataclasses
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_oracle as mo  # noqa: E402
import map_shapes as ms  # noqa: E402


def _all_clusters(name, *args):
    """every cluster of every read in rank order (the oracle without the cut to max_cand)"""
    s = ms.shape(name, *args)
    hits, _ = mo.map_reads(s.T, s.reads, ms.matrix(s.matrix), ms.GAP, dataclasses.replace(s.P, max_cand=1 << 30))
    return [h.cands for h in hits]


def test_ballot_votes_are_at_the_ballot_width():
    s = ms.shape("ballot")
    hits, info = ms.expected("ballot")
    assert (s.P.seed_len, s.P.seed_stride, s.P.max_occ, s.P.band, s.P.both_strands) == (16, 1, 4, 4, True)
    assert [len(r) for r in s.reads] == [78, 79, 80, 142, 143, 144, 80, 143, 144, 79]
    assert all(h.clusters == 1 and h.flags & 1 for h in hits)
    assert [(h.cands[0][0], h.cands[0][1]) for h in hits] == \
        [(63, 0), (64, 0), (65, 0), (127, 0), (128, 0), (129, 0), (65, 1), (128, 1), (129, 1), (64, 1)]
    # the last read's 64 hits are on its strand 1: the cluster ends where the sorted hit array ends
    assert hits[-1].cands[0][:2] == (64, 1) and info["hits"] == sum(h.cands[0][0] for h in hits)
    assert info["seeds_over_max_occ"] == 0
    # no limit on the occurrences: the same answer
    assert ms.expected("ballot", ms.NO_LIMIT) == (hits, info)


def test_long_clusters_span_many_ballots():
    s = ms.shape("long_clusters")
    hits, _ = ms.expected("long_clusters")
    assert [len(r) for r in s.reads] == [150, 296, 270] and (s.P.seed_len, s.P.seed_stride, s.P.max_occ, s.P.band) == (12, 2, 8, 300)
    assert all(h.clusters == 2 and h.flags & 1 and h.second == h.score for h in hits)
    assert hits[2].flags == 3
    votes = [c[0] for h in hits for c in h.cands]
    print("votes", votes)
    assert max(votes) > 11 * 64 and sum(v > 64 for v in votes) >= 5   # up to twelve rounds of the counting loop
    assert 257 <= max(len(r) for r in s.reads) <= 1024                  # the byte-profile wave traceback's rows


@pytest.mark.parametrize("max_cand", [64, 63, 5, 1])
def test_more_clusters_than_lanes(max_cand):
    s = ms.shape("many_clusters", max_cand)
    hits, info = ms.expected("many_clusters", max_cand)
    every = _all_clusters("many_clusters", max_cand)
    assert (s.P.seed_len, s.P.seed_stride, s.P.max_occ, s.P.band, s.P.max_cand) == (6, 1, 64, 0, max_cand)
    assert len(s.reads) == 9 and all(len(r) == 60 for r in s.reads)
    assert all(h.clusters > 300 and len(h.cands) == max_cand for h in hits)
    assert info["clusters"] > 3000 and info["pairs_aligned"] == 9 * max_cand
    for h, cl in zip(hits, every):
        assert h.clusters == len(cl) > 64 and [c[:3] for c in cl[:max_cand]] == [c[:3] for c in h.cands]
    for h, cl in zip(hits[:4], every[:4]):
        # the true diagonal has every seed's vote; clusters that come earlier in (strand, d0) order exist: it arrives in the
        # middle of the stream and is inserted in front of everything kept so far
        assert h.cands[0][0] == 55 and cl[1][0] < 55
        assert any((c[1], c[2]) < (cl[0][1], cl[0][2]) for c in cl[1:])
    assert every[0][0][2] == 0 and every[2][0][3] + 60 == len(s.T)          # a read at position 0 and one ending at n
    assert hits[3].flags == 3
    if max_cand >= 63:
        # equal votes on both sides of the cut: (strand, d0) decides which cluster is kept
        assert all(cl[max_cand - 1][0] == cl[max_cand][0] == 2 for cl in every)
    # band 0: every window is the read's span, clipped to the text
    assert all(c[5] - c[4] == min(60, c[2] + 60, len(s.T) - c[2]) for h in hits for c in h.cands)


def test_text_ends_and_band_limit():
    s = ms.shape("short_text")
    hits, _ = ms.expected("short_text")
    assert len(s.T) == 60 and s.P.band == 1024 and [len(r) for r in s.reads] == [120, 40, 65]   # a text shorter than the read
    assert [h.cands[0][2] for h in hits] == [-20, 10, -5] and [h.flags for h in hits] == [1, 1, 3]
    assert all(h.clusters == 1 and h.cands[0][4:6] == (0, 60) for h in hits)
    assert [(h.ref_start, h.ref_end) for h in hits] == [(0, 60), (10, 50), (0, 60)]
    s = ms.shape("band0_ends")
    hits, _ = ms.expected("band0_ends")
    n = len(s.T)
    assert s.P.band == 0 and [(h.flags, h.ref_start, h.ref_end) for h in hits] == \
        [(1, 0, 100), (1, n - 100, n), (3, 0, 90), (3, n - 90, n)]
    s = ms.shape("limits")
    hits, _ = ms.expected("limits")
    assert s.max_len == 4096 == max(len(r) for r in s.reads) and s.P.band == 1024 and s.P.max_cand == 1 and len(s.reads) == 2
    assert [h.flags for h in hits] == [1, 3] and all(h.score > 15000 for h in hits)


def test_max_len_of_the_caller():
    s = ms.shape("max_len_exceeded")
    hits, info = ms.expected("max_len_exceeded")
    assert s.max_len == 120 and [len(r) for r in s.reads] == [100, 150, 100]
    assert [(h.flags, h.err) for h in hits] == [(1, 0), (0, ms.TOO_LONG), (3, 0)]
    assert (hits[1].score, hits[1].votes, hits[1].ref_end, hits[1].alignA) == (0, 0, 0, b"")
    assert info["seeds"] == 2 * 2 * len(range(0, 100 - s.P.seed_len + 1, s.P.seed_stride))   # the long read's are not counted
    s = ms.shape("max_len_generous")
    hits, _ = ms.expected("max_len_generous")
    assert s.max_len == 1000 and max(len(r) for r in s.reads) == 150
    assert [h.flags for h in hits] == [1, 3, 1, 3, 0, 0] and len(s.reads[4]) == s.P.seed_len
    s = ms.shape("max_len_below_seed")
    hits, info = ms.expected("max_len_below_seed")
    assert s.max_len == 10 < s.P.seed_len and max(len(r) for r in s.reads) == 10
    assert all((h.flags, h.err) == (0, 0) for h in hits) and info["seeds"] == 0


def test_offsets_that_do_not_start_at_zero():
    s = ms.shape("offset_base")
    buf, offs = ms.offset_packed()
    assert int(offs[0]) == ms.OFFSET_BASE == 37 and len(buf) > int(offs[-1])
    assert [buf[int(a):int(b)].tobytes() for a, b in zip(offs[:-1], offs[1:])] == s.reads
    assert sum(h.flags & 1 for h in ms.expected("offset_base")[0]) == 4


def test_alphabet_cases():
    # the erring candidate is the last of four, and the error is the text's
    s = ms.shape("text_error_rank3")
    hits, info = ms.expected("text_error_rank3")
    assert s.T.count(b"N") == 1 and 7000 <= s.T.index(b"N") < 7300
    for h in hits[:2]:
        assert len(h.cands) == 4 and [c[6] for c in h.cands] == [700, 700, 700, 0] and h.cands[3][0] < h.cands[2][0]
        assert h.cands[3][4] <= s.T.index(b"N") < h.cands[3][5]
        assert (h.err, h.flags, h.score) == ((2 << 8) | ord("N"), 0, 0)
    assert [h.cands[0][1] for h in hits[:2]] == [0, 1]
    assert len(hits[2].cands) == 4 and hits[2].flags == 1 and hits[2].score == hits[2].second and hits[2].err == 0
    assert info["reads_mapped"] == 1
    # the reverse complement of Z is 0x00: its strand 1 seeds hit the run of zero bytes
    s = ms.shape("zero_bytes")
    hits, _ = ms.expected("zero_bytes")
    assert s.reads[:2] == [b"Z" * 30, b"\x00" * 30] and b"\x00" * 40 in s.T
    assert hits[0].clusters > 0 and all(c[1] == 1 for c in hits[0].cands)
    assert {c[1] for c in hits[1].cands} == {0, 1}
    assert [(h.err, h.flags) for h in hits] == [(0x100, 0), (0x100, 0), (0, 1)]
    # upper and lower case: the complement keeps the case
    s = ms.shape("mixed_case")
    hits, _ = ms.expected("mixed_case")
    assert set(s.T) == set(ms.CASE_ALPHABET.encode()) and s.matrix == "case"
    assert all(any(c in b"acgt" for c in r) and any(c in b"ACGT" for c in r) for r in s.reads)
    assert [h.flags for h in hits] == [1, 3] * 6 and all(h.err == 0 for h in hits)
    assert ms.rc(b"ACGTacgtn") == b"nacgtACGT"


def test_min_score_on_the_boundary():
    (h,), info = ms.expected("min_score", 700)
    assert (h.score, h.second, h.flags, h.clusters) == (700, 700, 1, 4) and info["reads_mapped"] == 1
    (h,), info = ms.expected("min_score", 701)
    assert (h.score, h.flags, h.clusters, h.err) == (0, 0, 4, 0) and [c[6] for c in h.cands] == [700] * 4
    assert info["clusters"] == 4 and info["pairs_aligned"] == 4 and info["reads_mapped"] == 0
    assert len(ms.shape("min_score", 701).reads[0]) == 140


def test_a_whole_chunk_without_hits():
    s = ms.shape("empty_middle_chunk")
    hits, _ = ms.expected("empty_middle_chunk")
    assert len(s.reads) == 768
    assert all(h.clusters == 0 and h.over == 0 for h in hits[256:512])         # no hit in the middle 256 reads
    assert any(len(r) < s.P.seed_len for r in s.reads[256:512]) and any(len(r) == 120 for r in s.reads[256:512])
    assert sum(h.flags & 1 for h in hits[:256]) > 200 and sum(h.flags & 1 for h in hits[512:]) > 200


def test_fork_shape_passes_the_traceback_workspace():
    s = ms.shape("traceback_fork")
    hits, info = ms.expected("traceback_fork")
    assert len(s.reads) == 500 and len(set(s.reads)) == 500 and s.tile * 500 == 36_000
    assert 153 <= min(len(r) for r in s.reads) and max(len(r) for r in s.reads) <= 256    # rows of the wave traceback, path 4
    assert all(len(h.cands) == 4 and h.flags & 1 for h in hits) and any(h.flags & 2 for h in hits)
    assert s.tile * info["pairs_aligned"] > ms.TB_PAIRS + 4096
    assert s.tile * info["hits"] > 65_536                                                  # the histogram scan's second level


@pytest.mark.parametrize("name", list(ms.TB_CLASSES))
def test_traceback_classes(name):
    s = ms.shape("traceback_class", name)
    hits, _ = ms.expected("traceback_class", name)
    lo, hi = {"le152": (1, 152), "le256": (153, 256), "le1024": (257, 1024), "le2048": (1025, 2048)}[name]
    assert len(s.reads) == 20 and lo <= max(len(r) for r in s.reads) <= hi
    assert s.note["path"] == {"le152": 6, "le256": 4, "le1024": 7, "le2048": 4}[name]
    assert sum(h.flags & 1 for h in hits) >= 18 and sum(1 for h in hits if h.flags & 2) >= 8
    assert any(b"-" in h.alignA or b"-" in h.alignB for h in hits)                         # indels among the mutations
