"""polyhip_mark_duplicates and polyhip_coord_order on the GPU against the plain-Python oracle (tests/dedup_oracle.py): exact
equality of every output on the hand-built inputs (tests/dedup_inputs.py), idempotence, invariance under a shuffle, and a pileup
without the duplicates on reads the GPU mapper placed."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import dedup_inputs as di  # noqa: E402
import dedup_oracle as do  # noqa: E402
import map_affine_inputs as mai  # noqa: E402
from map_check import _pack, _params, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SET_NAMES = tuple(s.name for s in di.all_sets())


def _assert_same(got, want, what):
    from poly_amd import dedup
    for f in ("dup", "rep", "weight", "err"):
        have, need = getattr(got, f), getattr(want, f)
        assert have.dtype == need.dtype and have.shape == need.shape, (what, f, have.dtype, have.shape, need.shape)
        bad = np.nonzero(have != need)[0]
        assert bad.size == 0, f"{what}: {f}: {len(bad)} entries differ, first {bad[0]}: got {have[bad[0]]}, want {need[bad[0]]}"
    assert dedup.last_info() == want.info, what


# ---------------------------------------------------------------- 1. the hand-built inputs
@pytest.mark.parametrize("name", SET_NAMES)
def test_hand_built_inputs(name):
    from poly_amd import dedup
    s = di.by_name(name)
    for mode in s.modes:
        _assert_same(dedup.mark_packed(**s.kwargs(mode)), do.mark(**s.kwargs(mode)), (name, mode))


@pytest.mark.parametrize("name", SET_NAMES)
def test_coord_order(name):
    from poly_amd import dedup
    s = di.by_name(name)
    sf = di.sam_flags(s)
    for paired in (False, True) if len(sf) % 2 == 0 else (False,):
        for rid in (s.rid, None):
            got = dedup.coord_order_packed(sf, s.ref_start, rid, paired)
            assert got.dtype == np.uint32 and got.tolist() == do.coord_order(sf, s.ref_start, rid, paired).tolist(), (name, paired)


def test_coord_order_unmapped_mates_and_wide_keys():
    from poly_amd import dedup
    s = di.by_name("pair_mate_unmapped_or_err2")
    sf = di.sam_flags(s)
    assert [(int(sf[i]) & 4, int(sf[i ^ 1]) & 4) for i in range(len(sf))].count((4, 0)) == 1 and list(sf[-2:]) == [4, 4]
    got = dedup.coord_order_packed(sf, s.ref_start, s.rid, True)
    assert got.tolist() == do.coord_order(sf, s.ref_start, s.rid, True).tolist() and got.tolist()[-2:] == [8, 9]
    # rid and ref_start at both ends of their range, an unplaced entry among them, ties in index order
    top = di.TOP
    sf, fs, rid = [0, 4, 0, 0, 4, 0, 0, 4], [top, 5, 0, top, top, 0, top, 0], [top, 0, 0, 0, top, top, top, 0]
    for paired in (False, True):
        assert dedup.coord_order_packed(sf, fs, rid, paired).tolist() == do.coord_order(sf, fs, rid, paired).tolist()
    assert dedup.coord_order_packed(sf, fs, rid).tolist() == [2, 3, 5, 0, 6, 1, 4, 7]
    assert dedup.coord_order_packed([4] * 5, [5, 4, 3, 2, 1]).tolist() == [0, 1, 2, 3, 4]


# ---------------------------------------------------------------- 2. properties
def _take(s, keep):
    kw = s.kwargs({})
    return {k: (v[keep] if isinstance(v, np.ndarray) and k not in ("qual", "qual_off") else v) for k, v in kw.items()}


@pytest.mark.parametrize("paired", [False, True])
def test_marking_again_finds_nothing(paired):
    from poly_amd import dedup
    s = di.random_set()
    first = dedup.mark_packed(**s.kwargs({"paired": paired}))
    assert first.dup.sum() > 1000
    keep = first.dup == 0
    if paired:                                        # mates stay together: a slot goes when either mate is a duplicate
        keep = np.repeat(keep[0::2] & keep[1::2], 2)
        assert first.dup[~keep].sum() == first.dup.sum()
    again = dedup.mark_packed(**_take(s, keep), paired=paired)
    assert again.dup.sum() == 0 and again.rep.tolist() == list(range(int(keep.sum())))
    info = dedup.last_info()
    assert info["dup_pairs"] == info["dup_fragments"] == 0 and info["entries"] == int(keep.sum())


@pytest.mark.parametrize("paired", [False, True])
def test_shuffled_entries_give_the_same_sets(paired):
    from poly_amd import dedup
    s = di.random_set()
    n = len(s.flags)
    rng = np.random.default_rng(di.SEED + 4)
    perm = rng.permutation(n // 2).repeat(2) * 2 + np.tile([0, 1], n // 2) if paired else rng.permutation(n)
    base = dedup.mark_packed(**s.kwargs({"paired": paired}))
    kw = _take(s, perm)
    got = dedup.mark_packed(**kw, paired=paired)
    _assert_same(got, do.mark(**kw, paired=paired), ("shuffled", paired))         # the winners follow the tie rule

    # as reads every candidate is a fragment and a set is an end set.  As pairs the sets compared are the pair sets: which
    # pair mate a tie makes the head of an end set, and so the representative of its fragments, is up to the order
    cand = ((s.flags & 1) == 1) & (base.err == 0)
    mask = cand & cand[np.arange(n) ^ 1] if paired else cand

    def sets(rep, ids):
        groups = {}
        for i, r in enumerate(rep.tolist()):
            if mask[ids[i]]:
                groups.setdefault(int(ids[r]), set()).add(int(ids[i]))
        return sorted(sorted(g) for g in groups.values())

    assert sets(got.rep, perm) == sets(base.rep, np.arange(n)) and got.dup.sum() == base.dup.sum()
    assert sorted(got.dup[np.argsort(perm)][~mask].tolist()) == sorted(base.dup[~mask].tolist())


# ---------------------------------------------------------------- 3. end to end: a pileup without the duplicates
def test_end_to_end_pileup_without_duplicates(nuc4_scoring):
    """the conditions -- every read mapped, every copy at its template's end, clips of 1..5 bases on both strands -- are
    asserted on the mapper's CPU oracle in tests/test_dedup_cpu.py::test_planted_copies_share_their_templates_end"""
    from poly_amd import bwt, dedup, mapper, pileup
    d = di.planted()
    T = d["T"]
    result = mapper.map_reads_affine_packed(bwt.New(T), nuc4_scoring, *mai.GAPS[di.PLANTED_GAPS], *_pack(d["reads"]), _params(mai.PARAMS))
    m = dedup.mark(result, di.PLANTED_READ)
    want = do.mark(result.flags, result.ref_start, result.ref_end, result.read_start, result.read_end, di.PLANTED_READ)
    _assert_same(m, want, "planted")
    assert m.dup.tolist() == [0] * 200 + [1] * 100
    assert m.rep[200:].tolist() == [k for k in d["template"] for _ in range(di.PLANTED_COPIES)]
    kw = dict(min_alt_count=di.PLANTED_MIN_ALT)
    with_dups, without = pileup.pileup(result, T, **kw), pileup.pileup(result, T, dup=m.dup, **kw)
    keep = np.nonzero(m.dup == 0)[0]
    A, B = [result.alignA[i] for i in keep], [result.alignB[i] for i in keep]
    off = np.zeros(len(keep) + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for a in A])
    deleted = pileup.pileup_packed(result.flags[keep], result.ref_start[keep], result.ref_end[keep], np.frombuffer(b"".join(A), np.uint8),
                                   np.frombuffer(b"".join(B), np.uint8), off, T, **kw)
    for f in ("counts", "consensus", "sites"):
        assert (getattr(without, f) == getattr(deleted, f)).all() and getattr(without, f).shape == getattr(deleted, f).shape, f
    assert without.nsites == deleted.nsites and (without.err == 0).all() and pileup.last_info()["used"] == 200
    snv = lambda p: {(int(x["pos"]), int(x["alt"])) for x in p.sites if x["kind"] == pileup.KIND_SNV}      # noqa: E731
    planted = set(zip(d["sites"], d["alts"]))
    assert planted <= snv(with_dups) and not planted & snv(without) and not {p for p, _ in snv(without)} & set(d["sites"])
    for p in d["sites"]:                              # six reads said so, one of them is left
        alt = b"ACGT".index(d["alts"][d["sites"].index(p)])
        assert with_dups.counts[alt, p] + with_dups.counts[8 + alt, p] == 6 and without.counts[alt, p] + without.counts[8 + alt, p] == 1
    # the flags the caller handed in are not touched
    assert (result.flags[200:] & 1).all()
