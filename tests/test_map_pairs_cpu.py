"""The paired-end mapper's inputs hold what they are named for (no GPU): on the oracle (tests/map_pairs_oracle.py) every named
pair of tests/map_pairs_inputs.py is in the case of the definition it was made for, and the oracle keeps its own invariants."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_pairs_inputs as mpi  # noqa: E402
import map_pairs_oracle as mpo  # noqa: E402

GO, GE = mpi.GAPS[0]


def _named(max_cand=4):
    return mpi.expected_named(max_cand)[0]


def _single_best(r, x):
    """the rank step 6 would pick for mate x on its own"""
    scores = [c[6] for c in (r.h1, r.h2)[x].cands]
    return max(range(len(scores)), key=lambda k: (scores[k], -k))


def test_the_dataset_is_what_the_issue_asks_for():
    d = mpi.dataset()
    assert len(d["T"]) == mpi.N and len(d["sampled"]) == 200 and len(d["reads1"]) == len(d["reads2"]) >= 220
    lens = [(len(d["reads1"][i]), len(d["reads2"][i])) for i in d["sampled"]]
    assert sum(a != b for a, b in lens) > 150 and all(90 <= x <= 160 for p in lens for x in p)
    assert all(200 <= ins <= 450 for _, ins, _ in d["origin"])
    # rescue windows stay under 500 columns
    for go, ge in mpi.GAPS:
        for r in mpi.expected(go, ge)[0]:
            assert all(a.whi - a.wlo <= 432 for a in r.attempts)
    cases = [r.case for r in mpi.expected(GO, GE)[0]]
    assert min(cases.count(c) for c in ("pair", "rescue", "fallback")) >= 20


def test_pairing_overrides_the_best_single_placement():
    for name, x in (("repeat_pairing", 1), ("repeat_pairing_flip", 0)):
        r = _named()[name]
        assert r.case == "pair" and r.proper and len((r.h1, r.h2)[x].cands) == 3
        assert r.ranks[x] != _single_best(r, x) == 0            # on its own the mate goes to the repeat's first copy
        assert (r.h1, r.h2)[x].second == (r.h1, r.h2)[x].score    # ... which scores the same


def test_equal_sums_go_to_the_smallest_ranks():
    r = _named()["tie_k1k2"]
    assert r.case == "pair" and len(r.proper_combos) == 2 and r.proper_combos[0][0] == r.proper_combos[1][0]
    assert r.ranks == (0, 0) and sorted(c[3] for c in r.proper_combos) == [310, 440] and r.tlen == 310


def test_insert_bounds_are_inclusive():
    n = _named()
    assert (n["ins_min"].case, n["ins_min"].tlen) == ("pair", 200) and (n["ins_max"].case, n["ins_max"].tlen) == ("pair", 450)
    for name in ("ins_min_minus1", "ins_max_plus1"):
        r = n[name]
        assert r.case == "fallback" and not r.proper and r.tlen == 0 and r.h1.flags & 1 and r.h2.flags & 1
        assert not (r.h1.flags | r.h2.flags) & 12
        # the rescue found the mate where it is, one base outside
        assert len(r.attempts) == 2 and all(a.res.score >= 550 and a.insert < 0 for a in r.attempts)


def test_orientations_that_are_never_proper():
    for name in ("dovetail", "same_strand", "discordant"):
        r = _named()[name]
        assert r.combos == 1 and not r.proper_combos and r.case == "fallback" and r.tlen == 0
        assert len(r.attempts) == 2 and all(a.res is not None and a.insert < 0 for a in r.attempts)     # both attempts failed
        assert r.h1.flags & 1 and r.h2.flags & 1 and not (r.h1.flags | r.h2.flags) & 12
    n = _named()
    assert n["same_strand"].h1.flags == n["same_strand"].h2.flags == 1
    assert n["dovetail"].h1.ref_start > n["dovetail"].h2.ref_start and n["dovetail"].h2.flags == 3


def test_rescues():
    n = _named()
    for name, anchor, anchor_strand in (("rescue_anchor_fwd", 1, 0), ("rescue_anchor_rev", 2, 1), ("rescue_anchor_rev_flip", 1, 1),
                                        ("rescue_short", 1, 0)):
        r = n[name]
        a, y = (r.h1, r.h2)[anchor - 1], (r.h1, r.h2)[2 - anchor]
        assert r.case == "rescue" and r.anchor == anchor and r.proper and r.tlen > 0 and len(r.attempts) == 1
        assert a.flags == 1 | anchor_strand << 1 | 4 and y.flags == 1 | (1 - anchor_strand) << 1 | 4 | 8
        assert y.votes == 0 and y.cands == [] and y.second == 0 and y.alignA        # no seed of the rescued mate survived
    d = mpi.dataset()
    assert len(d["reads2"][d["named"]["rescue_short"]]) == 12 < mpi.PARAMS.seed_len
    assert n["rescue_short"].h2.score == 60


def test_two_successful_attempts():
    n = _named()
    for name, anchor in (("rescue_both_a1", 1), ("rescue_both_a2", 2), ("rescue_both_tie", 1)):
        r = n[name]
        assert r.case == "rescue" and r.combos == 1 and len(r.attempts) == 2 and all(a.insert == 350 for a in r.attempts)
        t1, t2 = (a.total for a in r.attempts)
        assert (t1 == t2) if name.endswith("tie") else (t1 > t2) == (anchor == 1)
        assert r.anchor == anchor
        y = (r.h1, r.h2)[2 - anchor]
        assert y.flags & 8 and y.second == 600 and len(y.cands) == 1      # the rescued mate had a candidate of its own, elsewhere


def test_clipped_windows():
    n = _named()
    a = n["clip0"].attempts[0]
    assert n["clip0"].case == "rescue" and a.raw[0] < 0 == a.wlo and n["clip0"].tlen == 290
    a = n["clipn"].attempts[0]
    assert n["clipn"].case == "rescue" and a.raw[1] > mpi.N == a.whi and n["clipn"].tlen == 300
    r = n["clip_empty"]
    assert r.case == "fallback" and len(r.attempts) == 1 and r.attempts[0].wlo >= r.attempts[0].whi and r.attempts[0].res is None
    assert r.info["rescue_attempts"] == 0 and r.h1.flags == 1 and r.h2.flags == 0


def test_errors_of_a_mate():
    n = _named()
    r = n["err_N"]
    assert r.h2.err == (1 << 8) | ord("N") and r.h2.flags == 0 and r.h1.flags == 1 and r.case == "fallback" and not r.attempts
    r = n["too_long"]
    assert r.h1.err == 0xFFFFFFFF and r.h1.flags == 0 and r.h2.flags == 3 and not r.attempts and r.combos == 0
    r = n["rescue_err"]          # the attempt met the N; nothing of it is reported
    assert r.attempts[0].res.err != 0 and r.h2.err == 0 and r.h2.flags == 0 and r.case == "fallback" and r.info["rescue_attempts"] == 1
    r = n["unrelated"]
    assert r.h1.flags == r.h2.flags == 0 and not r.attempts and r.info["pairs_aligned"] == 0
    r = n["empty_mate"]
    assert r.h1.flags == 1 and r.h2.flags == 0 and not r.attempts


def test_more_combinations_than_lanes():
    r = _named(9)["combos81"]
    assert r.combos == 81 and len(r.h1.cands) == len(r.h2.cands) == 9 and len(r.proper_combos) == 9
    assert r.case == "pair" and r.ranks == (8, 8) and r.ranks[0] * 9 + r.ranks[1] >= 64      # beyond one wave's first pass
    assert r.h1.second < r.h1.score and _single_best(r, 0) == 8
    assert _named(4)["combos81"].info["pairs_aligned"] == 0                                      # max_occ 8 drops its seeds


def test_one_candidate():
    res = mpi.expected_named(1)[1]
    assert all(len(h.cands) <= 1 and h.second == (0 if not h.flags & 8 else h.second) for r in res for h in (r.h1, r.h2))
    n = _named(1)
    # the mate inside the repeat keeps the first copy only: pairing has nothing to choose, the rescue finds the right copy
    assert n["repeat_pairing"].case == "rescue" and n["repeat_pairing"].h2.flags & 8 and n["repeat_pairing"].tlen == 410


def test_invariants_of_the_oracle():
    runs = [mpi.expected(go, ge) for go, ge in mpi.GAPS] + [mpi.expected(GO, GE, False)] + [mpi.expected_named(c)[1:] for c in (1, 4, 9)]
    for k, (res, info) in enumerate(runs):
        PP = mpi.PAIR
        assert info["reads_mapped"] == sum((h.flags & 1) for r in res for h in (r.h1, r.h2))
        assert info["proper_pairs"] == sum(r.proper for r in res) and info["rescued"] == sum(r.case == "rescue" for r in res)
        assert info["rescue_attempts"] == sum(1 for r in res for a in r.attempts if a.res is not None)
        if k == 2:
            assert info["rescue_attempts"] == info["rescued"] == 0
        for r in res:
            f1, f2 = r.h1.flags, r.h2.flags
            assert bool(f1 & 4) == bool(f2 & 4) == r.proper and (r.tlen > 0) == r.proper
            assert bool((f1 | f2) & 8) == (r.case == "rescue") and not (f1 & f2 & 8)
            for h in (r.h1, r.h2):
                assert (h.flags & 1) or (h.score, h.second, h.votes, h.ref_end, h.read_end, h.alignA, h.alignB) == (0, 0, 0, 0, 0, b"", b"")
                assert not h.err or h.flags == 0
            if r.proper:      # step 2 on what was placed: left = ref_end - read_end along the end cell's diagonal
                d = mpi.dataset()
                i = res.index(r)
                if k < 3:
                    m = (len(d["reads1"][i]), len(d["reads2"][i]))
                else:
                    r1, r2, _ = mpi.named_pairs()
                    m = (len(r1[i]), len(r2[i]))
                lefts = [h.ref_end - h.read_end for h in (r.h1, r.h2)]
                assert (f1 >> 1 & 1) != (f2 >> 1 & 1)
                ins = mpo.proper_insert(f1 >> 1 & 1, lefts[0], m[0], f2 >> 1 & 1, lefts[1], m[1], PP)
                assert ins == r.tlen and PP.min_insert <= ins <= PP.max_insert
