"""The inputs of tests/map_gap_shapes.py reach the conditions they are named for -- asserted on the CPU oracles alone
(tests/map_affine_oracle.py, tests/map_pairs_oracle.py), so that tests/test_map_affine_shapes_gpu.py and
tests/test_map_pairs_shapes_gpu.py are known to take the kernels through those branches: the counts, ranks, trips and lanes of
the combinations, what every chunk of a sandwich holds, where the rescue windows are clipped, the err values.  No pair shape is
vacuous.  The module also prints what the oracle costs per shape (pytest -s shows it)."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_gap_shapes as mg  # noqa: E402
import map_pairs_inputs as mpi  # noqa: E402
import map_pairs_oracle as mpo  # noqa: E402
import map_shapes as ms  # noqa: E402

GAP_IDS = [f"{go}_{ge}" for go, ge in mg.GAPS]
AFFINE_SHAPES = [("ballot",), ("ballot", ms.NO_LIMIT), ("long_clusters",), ("many_clusters", 64), ("many_clusters", 63),
                 ("many_clusters", 5), ("many_clusters", 1), ("short_text",), ("band0_ends",), ("max_len_exceeded",),
                 ("max_len_generous",), ("max_len_below_seed",), ("text_error_rank3",), ("zero_bytes",), ("mixed_case",),
                 ("min_score", 1), ("empty_middle_chunk",)]
SECONDS = {}


def _timed(label, fn, *args, **kw):
    """fn(*args, **kw), its seconds kept under `label` when this is the call that computes it (the builders cache)"""
    t0 = time.perf_counter()
    out = fn(*args, **kw)
    SECONDS.setdefault(label, time.perf_counter() - t0)
    return out


def _affine(name, *args, gaps):
    return _timed(f"affine {name}{args} {gaps}", mg.affine_expected, name, *args, go=gaps[0], ge=gaps[1])


def _pairs(name, *args):
    return _timed(f"{name}{args}", mg.PAIR_SHAPES[name], *args)


def _t(r, k1, k2):
    return k1 * len(r.h2.cands) + k2


# ================================================================ what the suite already pays for (first: pairs_sandwich reuses it)
def test_existing_oracle_seconds():
    import map_affine_inputs as mai
    _timed("existing map_affine_inputs.expected(-5, -2)", mai.expected, *mg.GAPS[0])
    res, _ = _timed("existing map_pairs_inputs.expected(-5, -2)", mpi.expected, *mg.GAPS[0])
    assert len(res) == len(mpi.dataset()["reads1"])


# ================================================================ the affine oracle on map_shapes' shapes
@pytest.mark.parametrize("gaps", mg.GAPS, ids=GAP_IDS)
def test_affine_answers_share_the_seed_stage_with_the_linear_ones(gaps):
    """steps 1-4 do not know the gaps: clusters, ranks, windows and the shared counters but reads_mapped are the linear
    oracle's; the caller's max_len is applied in the same way"""
    for shape in AFFINE_SHAPES:
        hits, info = _affine(*shape, gaps=gaps)
        lin_hits, lin_info = ms.expected(*shape)
        assert len(hits) == len(ms.shape(*shape).reads) == len(lin_hits)
        for k in ("seeds", "seeds_over_max_occ", "hits", "clusters", "pairs_aligned"):
            assert info[k] == lin_info[k], (shape, k)
        for h, g in zip(hits, lin_hits):
            assert [c[:6] for c in h.cands] == [c[:6] for c in g.cands] and h.clusters == g.clusters and h.err == g.err, shape
    hits, _ = _affine("max_len_exceeded", gaps=gaps)
    assert [(h.flags, h.err) for h in hits] == [(1, 0), (0, ms.TOO_LONG), (3, 0)] and not hits[1].cands


@pytest.mark.parametrize("gaps", mg.GAPS, ids=GAP_IDS)
@pytest.mark.parametrize("max_cand", [64, 63, 5, 1])
def test_affine_windows_of_one_read_fill_a_wave(gaps, max_cand):
    hits, info = _affine("many_clusters", max_cand, gaps=gaps)
    assert all(len(h.cands) == max_cand for h in hits) and info["pairs_aligned"] == 9 * max_cand
    assert all(1 <= c[5] - c[4] <= 60 for h in hits for c in h.cands)            # band 0: windows of the read's span, clipped
    assert all(h.flags & 1 for h in hits)
    for h in hits:
        losers = [c[6] for k, c in enumerate(h.cands) if k != h.best_rank]
        assert h.second == max(losers, default=0) and len(losers) == max_cand - 1
    if max_cand >= 5:
        assert all(h.best_rank == 0 and h.score == 300 and 0 < h.second < 300 for h in hits[:4])
        assert any(h.best_rank > 0 for h in hits[4:])                             # an unrelated read's winner is not rank 0


@pytest.mark.parametrize("gaps", mg.GAPS, ids=GAP_IDS)
def test_affine_text_ends(gaps):
    s = ms.shape("short_text")
    hits, _ = _affine("short_text", gaps=gaps)
    # a window with fewer columns than the read has rows
    assert all(h.cands[0][4:6] == (0, 60) for h in hits) and [len(r) for r in s.reads] == [120, 40, 65]
    assert [(h.flags, h.ref_start, h.ref_end) for h in hits] == [(1, 0, 60), (1, 10, 50), (3, 0, 60)]
    assert [(h.read_start, h.read_end) for h in hits] == [(20, 80), (0, 40), (5, 65)]
    hits, _ = _affine("band0_ends", gaps=gaps)
    n = len(ms.shape("band0_ends").T)
    assert [(h.flags, h.ref_start, h.ref_end) for h in hits] == [(1, 0, 100), (1, n - 100, n), (3, 0, 90), (3, n - 90, n)]
    assert [h.cands[0][4:6] for h in hits] == [(0, 100), (n - 100, n), (0, 90), (n - 90, n)]


@pytest.mark.parametrize("gaps", mg.GAPS, ids=GAP_IDS)
def test_affine_alphabet_cases(gaps):
    hits, info = _affine("text_error_rank3", gaps=gaps)
    for h in hits[:2]:          # the erring candidate is the last of four, and the error is the text's
        assert len(h.cands) == 4 and [c[6] for c in h.cands] == [700, 700, 700, 0]
        assert (h.err, h.flags, h.score) == ((2 << 8) | ord("N"), 0, 0)
    assert hits[2].flags == 1 and hits[2].err == 0 and info["reads_mapped"] == 1
    hits, _ = _affine("zero_bytes", gaps=gaps)
    assert [(h.err, h.flags) for h in hits] == [(0x100, 0), (0x100, 0), (0, 1)]
    hits, _ = _affine("mixed_case", gaps=gaps)
    assert [h.flags for h in hits] == [1, 3] * 6 and all(h.err == 0 for h in hits)
    assert any(b"-" not in h.alignA and h.alignA != h.alignB for h in hits)      # the same base in the other case is aligned


@pytest.mark.parametrize("gaps", mg.GAPS, ids=GAP_IDS)
def test_affine_min_score_on_the_boundary(gaps):
    (h,), _ = _affine("min_score", 1, gaps=gaps)
    assert h.score == 700 == h.second and h.flags == 1
    (at,), info = _affine("min_score", h.score, gaps=gaps)
    assert at.flags == 1 and info["reads_mapped"] == 1
    (above,), info = _affine("min_score", h.score + 1, gaps=gaps)
    assert (above.flags, above.score, above.err) == (0, 0, 0) and [c[6] for c in above.cands] == [700] * 4 and info["reads_mapped"] == 0


@pytest.mark.parametrize("gaps", mg.GAPS, ids=GAP_IDS)
def test_affine_chunk_without_a_winner(gaps):
    hits, _ = _affine("empty_middle_chunk", gaps=gaps)
    assert len(hits) == 768 and not any(h.flags or h.cands for h in hits[256:512])
    assert sum(h.flags & 1 for h in hits[:256]) > 200 and sum(h.flags & 1 for h in hits[512:]) > 200


@pytest.mark.parametrize("gaps", mg.GAPS, ids=GAP_IDS)
def test_affine_winner_of_more_than_32_bands(gaps):
    s = mg.le2048_first3()
    hits, _ = _timed(f"affine le2048_first3 {gaps}", mg.cut_expected, "le2048_first3", go=gaps[0], ge=gaps[1])
    assert 1025 <= len(s.reads[0]) <= 2048 and len(s.reads) == 3 and s.reads == ms.shape("traceback_class", "le2048").reads[:3]
    assert all(h.flags & 1 for h in hits) and hits[0].read_end - hits[0].read_start > 32 * 32
    assert any(b"-" in h.alignA or b"-" in h.alignB for h in hits)


def test_affine_limits():
    """max_len 4096 with band 1024: the forward read, gaps (-12, -2)"""
    s = mg.limits_forward()
    (h,), info = _timed("affine limits_forward", mg.cut_expected, "limits_forward", mg.LIMITS_BAND, go=mg.LIMITS_GAPS[0], ge=mg.LIMITS_GAPS[1])
    assert mg.LIMITS_BAND == 1024 == s.P.band and mg.LIMITS_GAPS == (-12, -2)
    assert s.max_len == 4096 == len(s.reads[0]) and len(s.reads) == 1 and s.reads[0] == ms.shape("limits").reads[0]
    assert h.flags == 1 and h.score > 15000 and h.cands[0][5] - h.cands[0][4] > 4096 + 1024 and info["pairs_aligned"] == 1


# ================================================================ pair shapes
def test_many_combinations():
    s = _pairs("pairs_many_combos")
    by = dict(zip(s.names, s.results))
    lane = ms.shape("many_clusters", 64).P
    assert (s.P.seed_len, s.P.seed_stride, s.P.max_occ, s.P.band, s.P.max_cand, s.P.min_score) == (6, 1, 64, 0, 64, 1) and s.P == lane
    assert (s.PP.min_insert, s.PP.max_insert, s.PP.rescue) == (200, 450, True)
    # (a) 64 x 64, the winner in the second half of the 64 trips, its mate 1 at a late rank with the best score
    r = by["late_trip"]
    assert (len(r.h1.cands), len(r.h2.cands), r.combos) == (64, 64, 4096) and r.case == "pair" and r.tlen == 320
    assert _t(r, *r.ranks) >= 64 * 32 and r.ranks[0] >= 32 and r.h1.votes == 2 and r.h1.best_rank == r.ranks[0]
    assert len(r.proper_combos) > 1 and any(_t(r, c[1], c[2]) < _t(r, *r.ranks) for c in r.proper_combos)   # earlier ones lose
    # (b) nc2 (nc1) does not divide 64, and the two ranks differ
    r = by["short_mate2"]
    assert len(r.h1.cands) == 64 and 1 < len(r.h2.cands) < 64 and 64 % len(r.h2.cands) != 0 and r.case == "pair" and r.tlen == 300
    assert r.ranks[0] >= 32 and r.ranks[0] != r.ranks[1] and _t(r, *r.ranks) // 64 > 0
    assert r.ranks[0] >= len(r.h2.cands)                          # swapped, the quotient is no rank of mate 2
    r = by["short_mate1"]
    assert len(r.h2.cands) == 64 and 1 < len(r.h1.cands) < 64 and 64 % len(r.h1.cands) != 0 and r.case == "pair" and r.tlen == 300
    assert r.ranks[0] != r.ranks[1] and r.ranks[1] > 8
    # (c) two proper combinations of equal, maximal sum in different trips and lanes; the smaller t wins, from the higher lane
    r = by["tie_trips"]
    top = max(c[0] for c in r.proper_combos)
    ties = sorted(_t(r, c[1], c[2]) for c in r.proper_combos if c[0] == top)
    assert (len(r.h1.cands), len(r.h2.cands)) == (64, 64) and len(ties) == 2 and top == 591
    t1, t2 = ties
    assert t1 // 64 != t2 // 64 and t1 % 64 != t2 % 64 and t1 % 64 > t2 % 64
    assert r.case == "pair" and _t(r, *r.ranks) == t1 and r.ranks == (0, 1) and r.tlen == 300
    # (d) no combination at all, a rescue anchored on a winner of rank >= 32 (mate 1's, then mate 2's)
    for name, x in (("late_anchor", 0), ("late_anchor_flip", 1)):
        r = by[name]
        a, y = (r.h1, r.h2)[x], (r.h1, r.h2)[1 - x]
        assert r.combos == 0 and not r.proper_combos and r.case == "rescue" and r.anchor == x + 1 and len(r.attempts) == 1
        assert len(a.cands) == 64 and a.best_rank == r.ranks[x] >= 32 and a.votes == 2 and a.score > 200
        assert a.ref_start == (mg.COMBOS_D_AT, mg.COMBOS_F_AT)[x] and a.ref_end == a.ref_start + 60   # where the mate was taken from
        assert not y.cands and y.flags & 8 and y.score == 25 and r.info["rescue_attempts"] == 1
    assert by["late_anchor"].h1.flags == 5 and by["late_anchor_flip"].h2.flags == 7
    assert s.info["rescue_attempts"] == 2 == s.info["rescued"] and s.info["proper_pairs"] == len(s.results) == 6


@pytest.mark.parametrize("max_cand", [63, 5, 1])
def test_many_combinations_with_fewer_candidates(max_cand):
    s = _pairs("pairs_many_combos", max_cand)
    full = dict(zip(s.names, mg.pairs_many_combos().results))
    by = dict(zip(s.names, s.results))
    assert s.P.max_cand == max_cand and all(len(h.cands) <= max_cand for r in s.results for h in (r.h1, r.h2))
    assert len(by["late_trip"].h1.cands) == max_cand == len(by["tie_trips"].h2.cands)
    if max_cand == 63:      # the late ranks are still kept
        assert [r.ranks for r in s.results] == [r.ranks for r in full.values()] and by["late_trip"].combos == 63 * 63
    else:                   # they are cut: the true place is no candidate, the pair is made by chance, by a rescue or not at all
        assert by["late_trip"].ranks != full["late_trip"].ranks and by["late_anchor"].h1.score < full["late_anchor"].h1.score
        # the tie: among five candidates both fragments are whole; of one each the clean copies are left, 2000 bases apart
        assert (by["tie_trips"].case, by["tie_trips"].ranks) == (("pair", (0, 1)) if max_cand == 5 else ("rescue", (0, -1)))
    assert s.info["pairs_aligned"] == sum(len(h.cands) for r in s.results for h in (r.h1, r.h2)) > 0 and s.info["reads_mapped"] > 6


def test_many_combinations_without_rescue():
    s = _pairs("pairs_many_combos", 64, False)
    by = dict(zip(s.names, s.results))
    assert s.info["rescue_attempts"] == 0 == s.info["rescued"] and s.info["proper_pairs"] == 4
    assert by["late_anchor"].case == "fallback" and by["late_anchor"].h1.flags == 1 and by["late_anchor"].h2.flags == 0
    assert by["late_trip"].ranks == mg.pairs_many_combos().results[0].ranks


def _requests(chunk):
    return sum(1 for r in chunk for a in r.attempts if a.res is not None)


def _winners(chunk):
    return sum((h.flags & 1) for r in chunk for h in (r.h1, r.h2))


@pytest.mark.parametrize("variant", mg.SANDWICHES)
def test_sandwich_chunks(variant):
    s = _pairs("pairs_sandwich", variant)
    chunks = s.note["chunks"]
    assert len(s.reads1) == len(s.reads2) == 3 * mg.CHUNK == len(s.results) and [len(c) for c in chunks] == [mg.CHUNK] * 3
    assert s.P == mpi.PARAMS and s.PP == mpi.PAIR and s.max_len == mpi.MAX_LEN
    assert s.results == [r for c in chunks for r in c]
    req, win = [_requests(c) for c in chunks], [_winners(c) for c in chunks]
    assert s.info["rescue_attempts"] == sum(req) and s.info["reads_mapped"] == sum(win)
    if variant == "empty_middle":
        assert req[0] > 20 and win[0] > 200 and sum(r.case == "rescue" for r in chunks[0]) > 20
        assert req[1] == 0 and win[1] == 0 and not any(h.cands or h.err for r in chunks[1] for h in (r.h1, r.h2))
        assert all(r.case == "pair" and not r.attempts for r in chunks[2][:-8])         # no request up to the last pairs
        assert all(r.case == "rescue" for r in chunks[2][-8:]) and req[2] >= 8 and win[2] == 2 * mg.CHUNK
    elif variant == "winners_middle":
        assert req[1] == 0 and win[1] == 2 * mg.CHUNK and all(r.case == "pair" for r in chunks[1]) and req[0] > 20 and req[2] > 20
    else:
        assert req[0] == 0 and win[0] == 2 * mg.CHUNK and req[1] == 0 and win[1] == 0 and req[2] > 20 and win[2] > 200


def test_offsets_that_do_not_start_at_zero():
    s = _pairs("pairs_offsets")
    (buf1, offs1), (buf2, offs2) = s.note["packed"]
    assert (int(offs1[0]), int(offs2[0])) == mg.OFFSET_BASES == (37, 5) and len(buf1) > int(offs1[-1]) and len(buf2) > int(offs2[-1])
    assert [buf1[int(a):int(b)].tobytes() for a, b in zip(offs1[:-1], offs1[1:])] == s.reads1
    assert [buf2[int(a):int(b)].tobytes() for a, b in zip(offs2[:-1], offs2[1:])] == s.reads2
    assert bytes(buf1[:37]) == b"G" * 37 and bytes(buf2[:5]) == b"C" * 5
    assert (s.reads1, s.reads2, s.names) == mpi.named_pairs() and s.info["rescued"] > 5 and s.info["proper_pairs"] > s.info["rescued"]


def test_rescue_through_the_complement_table():
    s = _pairs("pairs_alphabet")
    by = dict(zip(s.names, s.results))
    assert len(s.mat.first) == 126 and set(s.T) - {mg.ALPHA_OUTSIDE} <= set(mg.ALPHA_SYMBOLS) and s.T.count(bytes([mg.ALPHA_OUTSIDE])) == 1
    assert mg.rc(b"RYKMBVDHrykmbvdhACGTacgt") == b"acgtACGTdhbvkmryDHBVKMRY" and mg.rc(b"Z\x00") == b"\x00\x00"
    for name in ("mixed", "lower", "iupac"):
        r = by[name]
        assert r.case == "rescue" and r.anchor == 1 and r.h1.flags == 5 and r.h2.flags == 15 and r.tlen == 290 and not r.h2.cands
        assert r.h2.score >= s.P.min_score and (r.h2.ref_end - r.h2.ref_start, r.h2.read_end - r.h2.read_start) == (60, 60)
    q = {name: mg.rc(s.reads2[s.names.index(name)]) for name in s.names}              # what the rescue aligns
    assert set(q["lower"]) <= set(b"acgt") and set(q["iupac"]) <= set(b"RYKMBVDH") and len(set(q["iupac"])) == 8
    assert any(c in b"acgt" for c in q["mixed"]) and any(c in b"RYKMBVDH" for c in q["mixed"]) and any(c in b"rykmbvdh" for c in q["mixed"])
    # a byte whose complement is 0x00, and a byte of the window outside the second alphabet: the attempt errs, nothing says so
    for name, err in (("zero", 1 << 8), ("window_outside", (2 << 8) | mg.ALPHA_OUTSIDE)):
        r = by[name]
        (a,) = r.attempts
        assert a.res is not None and a.res.err == err and a.strand == 1 and r.case == "fallback" and r.info["rescue_attempts"] == 1
        assert (r.h1.flags, r.h1.err, r.h2.flags, r.h2.err, r.h2.cands) == (1, 0, 0, 0, [])
    assert 0 in q["zero"] and b"Z" in s.reads2[s.names.index("zero")]
    a = by["window_outside"].attempts[0]
    assert a.wlo <= s.T.index(bytes([mg.ALPHA_OUTSIDE])) < a.whi
    assert s.info["rescue_attempts"] == 5 and s.info["rescued"] == 3


def test_text_shorter_than_the_rescue_window():
    s = _pairs("pairs_short_text")
    by = dict(zip(s.names, s.results))
    n = len(s.T)
    assert 300 <= n <= 400 and (s.PP.min_insert, s.PP.max_insert) == (200, 450) and s.P.band == 0
    r = by["ends"]
    assert r.case == "pair" and r.proper_combos == [(1000, 0, 0, n)] and r.tlen == n
    assert (r.h1.flags, r.h1.ref_start, r.h2.flags, r.h2.ref_end) == (5, 0, 7, n)
    for name, y in (("both_clipped", 0), ("both_clipped_flip", 0)):
        r = by[name]
        (a,) = r.attempts
        assert a.raw[0] < 0 == a.wlo and a.raw[1] > n == a.whi and a.whi - a.wlo < a.raw[1] - a.raw[0]   # cut at both ends at once
        assert r.case == "rescue" and r.tlen == n and (r.h1, r.h2)[y].flags & 8 and not (r.h1, r.h2)[y].cands
    assert by["both_clipped"].h1.flags == 13 and by["both_clipped_flip"].h1.flags == 15
    r = by["mate1_longer"]
    assert len(s.reads1[s.names.index("mate1_longer")]) == 410 == s.max_len > n
    assert r.h1.flags == 1 and (r.h1.ref_start, r.h1.ref_end, r.h1.read_start, r.h1.read_end) == (0, n, 20, 370)
    assert r.case == "fallback" and [a.res is not None for a in r.attempts] == [True, True] and r.attempts[1].raw[0] < 0 and r.attempts[1].raw[1] > n
    assert s.info["rescue_attempts"] == 4 and s.info["rescued"] == 2 and s.info["proper_pairs"] == 3


def test_pair_with_an_error_at_rank_3():
    s = _pairs("pairs_rank3_error")
    base = ms.shape("text_error_rank3")
    assert s.T == base.T and s.reads1 == base.reads and s.P == base.P
    for name in ("fwd_errs", "rev_errs"):
        r = dict(zip(s.names, s.results))[name]
        assert [c[6] for c in r.h1.cands] == [700, 700, 700, 0] and (r.h1.err, r.h1.flags) == ((2 << 8) | ord("N"), 0)
        assert r.combos == 0 and not r.proper_combos and not r.attempts and r.case == "fallback" and r.tlen == 0
        assert r.h2.flags & 1 and r.h2.err == 0 and r.h2.score == 600 and not r.h2.flags & 12
    r = s.results[2]
    assert r.case == "pair" and r.combos == 4 and len(r.proper_combos) == 1 and r.tlen == 400 and r.ranks == (0, 0)
    assert s.info["rescue_attempts"] == 0 and s.info["reads_mapped"] == 4 and s.info["proper_pairs"] == 1


def test_pair_shapes_keep_the_oracles_invariants():
    for name in mg.PAIR_SHAPES:
        s = _pairs(name)
        T, r1, r2, P, PP, max_len, (res, info) = s
        assert len(r1) == len(r2) == len(res) > 0 and info == {k: sum(r.info[k] for r in res) for k in mpo.COUNTERS}
        assert info["pairs_aligned"] > 0 and info["reads_mapped"] > 0
        for r, a, b in zip(res, r1, r2):
            assert bool(r.h1.flags & 4) == bool(r.h2.flags & 4) == r.proper == (r.tlen > 0)
            if r.proper:
                f1, f2 = r.h1.flags, r.h2.flags
                ins = mpo.proper_insert(f1 >> 1 & 1, r.h1.ref_end - r.h1.read_end, len(a), f2 >> 1 & 1, r.h2.ref_end - r.h2.read_end,
                                        len(b), PP)
                assert ins == r.tlen


# ================================================================ what the oracle costs (last: every shape has been built)
def test_oracle_seconds_per_shape():
    """prints the seconds of every first call above, the two datasets the suite already pays for among them"""
    for label, sec in SECONDS.items():
        print(f"{sec:8.2f} s  {label}")
    print(f"{sum(v for k, v in SECONDS.items() if not k.startswith('existing')):8.2f} s  all new shapes")
    assert SECONDS and all(np.isfinite(v) for v in SECONDS.values())
