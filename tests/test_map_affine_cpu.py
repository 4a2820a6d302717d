"""No GPU: the affine read mapper's inputs (tests/map_affine_inputs.py) hold what tests/test_map_affine_gpu.py relies on,
asserted on the two CPU oracles (tests/map_oracle.py with linear gaps, tests/map_affine_oracle.py with affine ones)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_affine_inputs as mai  # noqa: E402
import map_inputs as mi  # noqa: E402
import map_oracle as mo  # noqa: E402
import sw_affine_oracle as ao  # noqa: E402

FIELDS = ["score", "second", "flags", "votes", "ref_start", "ref_end", "read_start", "read_end", "err", "alignA", "alignB"]
DIR_CAP = 1 << 30       # bytes of direction bits the library holds at once
MAX_LEN_CAP = 4096      # polyhip_map_reads' limits
BAND_CAP = 1024


def _gaps(h):
    return h.alignA.count(b"-") + h.alignB.count(b"-")


def test_the_set_has_about_300_reads_in_two_chunks():
    d = mai.dataset()
    assert 256 < len(d["reads"]) <= 320
    assert set(d["special"]) == {"short", "clip0", "clipn", "tie_fwd", "tie_rev", "polyA", "err", "X", "rcX", "Z"}


def test_x_goes_to_the_copy_with_the_insertion_under_linear_gaps_only():
    d = mai.dataset()
    lin, _ = mai.expected_linear()
    aff, _ = mai.expected(-12, -2)
    for name in ("X", "rcX"):
        i = d["special"][name]
        assert lin[i].best_rank == 0 and _gaps(lin[i]) == 6 and lin[i].second != 0
        assert lin[i].score == 150 * 5 - 12 and lin[i].second == 148 * 5 - 8
        assert aff[i].best_rank != 0 and _gaps(aff[i]) == 0 and aff[i].second != 0
        assert aff[i].score == 148 * 5 - 8
        assert lin[i].ref_start != aff[i].ref_start
        assert bool(aff[i].flags & 2) == (name == "rcX")


def test_z_is_mapped_under_linear_gaps_and_not_under_affine_ones():
    d = mai.dataset()
    lin, aff = mai.z_scores()
    P = mai.z_params()
    assert aff < P.min_score < lin
    z = d["reads"][d["special"]["Z"]]
    info = dict.fromkeys(mai.COUNTERS, 0)
    assert mo.map_read(d["T"], z, mi.nuc4(), -2, P, info).flags & 1
    hits, _ = mai.affine_each(d["T"], mai.z_reads(), -12, -2, P)
    assert hits[0].flags == 0 and hits[0].score == 0 and hits[0].best_rank >= 0   # it has candidates, none scores enough
    assert hits[1].flags & 1 and hits[2].flags & 1                                # X and rc(X) still do


def test_affine_gaps_change_strings_and_make_gap_runs():
    lin, _ = mai.expected_linear()
    aff, _ = mai.expected(-5, -2)
    mapped = [i for i, h in enumerate(aff) if h.flags & 1 and lin[i].flags & 1]
    changed = [i for i in mapped if (aff[i].alignA, aff[i].alignB) != (lin[i].alignA, lin[i].alignB)]
    assert len(mapped) >= 200 and len(changed) * 10 >= len(mapped)
    assert any(b"--" in h.alignA or b"--" in h.alignB for h in aff)


def test_equal_gaps_are_the_linear_mapper():
    lin, linfo = mai.expected_linear()
    aff, ainfo = mai.expected(-2, -2)
    assert ainfo == linfo
    for i, (a, b) in enumerate(zip(aff, lin)):
        for f in FIELDS + ["best_rank", "cands"]:
            assert getattr(a, f) == getattr(b, f), (i, f)


def test_every_class_of_read_occurs():
    d = mai.dataset()
    s = d["special"]
    for go, ge in mai.GAPS:
        hits, info = mai.expected(go, ge)
        assert info["reads_mapped"] >= 230 and info["seeds_over_max_occ"] > 0
        assert sum(1 for h in hits if h.flags & 2) >= 100
        assert all(hits[i].flags == 0 and not hits[i].cands for i in d["unrelated"])
        assert hits[s["short"]].flags == 0 and hits[s["err"]].err == (1 << 8) | ord("N")
        assert hits[s["tie_fwd"]].second == hits[s["tie_fwd"]].score and hits[s["tie_fwd"]].best_rank == 0
        assert hits[s["clip0"]].ref_start == 0 and hits[s["clipn"]].ref_end == len(d["T"])


def _range_ok(mat, go, max_len, band):
    absmax = max(abs(mat.smin), abs(mat.smax), -go)
    return absmax * (max_len + (max_len + 3 * band)) < 1 << 30


def test_kernel_range_and_direction_bits_of_every_gpu_input():
    rb = ao.rows_per_band()
    d = mai.dataset()
    g = mai.general_case()
    cases = [(mai.MAT, go, max(len(r) for r in d["reads"]), mai.PARAMS.band) for go, _ in mai.GAPS + ((-2, -2),)]
    cases.append((g["mat"], g["go"], max(len(r) for r in g["reads"]), g["P"].band))
    cases.append((mai.MAT, -5, 300, mai.PARAMS.band))       # max_len above the longest read
    for mat, go, max_len, band in cases:
        assert max_len <= MAX_LEN_CAP and band <= BAND_CAP
        assert _range_ok(mat, go, max_len, band)
        # one winner's direction bits at the largest window: 4 bits per cell, whole bands of rows
        words = -(-max_len // rb) * (max_len + 3 * band) * (rb // 8)
        assert 0 < words * 4 <= DIR_CAP
    # the range test of the GPU file: big_matrix with gap_open = -2^17 and band 16 leaves the range at max_len = 4072
    big = ao.big_matrix()
    assert not _range_ok(big, -(1 << 17), 4072, 16) and _range_ok(big, -(1 << 17), 4071, 16) and 4072 <= MAX_LEN_CAP
    words = -(-4071 // rb) * (4071 + 3 * 16) * (rb // 8)
    assert words * 4 * 4 <= DIR_CAP                        # ... whose four reads' direction bits are held at once


def test_no_winner_inputs_have_none():
    d = mai.dataset()
    seen = {}
    for name, (reads, P) in mai.no_winner_cases().items():
        for go, ge in mai.GAPS:
            hits, infos = mai.affine_each(d["T"], reads, go, ge, P)
            assert all(h.flags == 0 and h.score == 0 and h.alignA == b"" for h in hits), name
            seen[name] = mai.total(infos)
    assert seen["short"]["seeds"] == 0
    assert seen["unrelated"]["seeds"] > 0 and seen["unrelated"]["pairs_aligned"] == 0
    assert seen["below_min_score"]["pairs_aligned"] > 12 and seen["below_min_score"]["reads_mapped"] == 0
    assert seen["err"]["pairs_aligned"] >= 1
    # the sandwich: chunks of 256 reads, the middle one without a winner, winners on both sides
    reads, middle = mai.sandwich()
    hits, info, mh = mai.sandwich_expected(-5, -2)
    assert len(reads) >= 512 + 1 and len(hits) == len(reads)
    assert all(h.flags == 0 for h in hits[256:512]) and mh == hits[256:512]
    assert any(h.flags & 1 for h in hits[:256]) and any(h.flags & 1 for h in hits[512:])


def test_general_case_uses_a_table_too_large_for_lds():
    g = mai.general_case()
    assert (len(g["mat"].first) + 1) * (len(g["mat"].second) + 1) * 4 + 512 > 60 * 1024
    assert not g["P"].both_strands and sum(h.flags & 1 for h in g["hits"]) >= 30
    assert any(b"-" in h.alignA or b"-" in h.alignB for h in g["hits"])
    assert all(0 < c < 13 for c in g["T"])      # no '$' (36), nothing outside the matrix
