"""The inputs of tests/k5_shapes.py have the properties they are named for -- asserted on the CPU oracle and on the numpy
restatement of K5's candidate rule (k5_shapes.candidates / period / equal_bytes), so that tests/test_k5_shapes_gpu.py is
known to take the three least-rotation kernels through their data-dependent paths on both strands: the candidate count
and the period of every family member and of its reverse complement, which of the two strands is the smaller one (the
strand seqhash.Hash keeps: only there does a wrong second-strand index change the hash), what a batch of 40,000 short
sequences holds.

Three inputs of tests/test_seqhash_gpu.py that are named for a property they do not have are recorded at the end."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import k5_shapes as ks  # noqa: E402
import oracle as orc  # noqa: E402

MEMBERS = ks.members()
IDS = [f"{m.family}-{m.size}-{i}" for i, m in enumerate(MEMBERS)]


def _within(v, r):
    return r[0] <= v <= r[1]


# ---------------------------------------------------------------- the restatement itself
def _naive_candidates(s: bytes) -> int:
    n = len(s)
    w = [bytes(s[(p + k) % n] for k in range(4)) for p in range(n)]
    m = min(w)
    hit = [x == m for x in w]
    if n >= 4 and len(set(m)) == 1:
        hit = [h and not hit[p - 1] for p, h in enumerate(hit)]
    return sum(hit)


def test_the_models_on_small_strings():
    assert ks.candidates(b"AAAC" * 3) == 3 and ks.period(b"AAAC" * 3) == 4
    assert ks.candidates(b"AAAAC") == 1 and ks.candidates(b"AAAACAAAAC") == 2 and ks.candidates(b"AACAA") == 1
    assert ks.candidates(b"A" * 9) == 0 and ks.period(b"A" * 9) == 1
    assert ks.candidates(b"CCCCACCCC") == 1 and ks.candidates(b"TTAGCCCAT") == 1
    assert ks.period(b"ACGT") == 4 and ks.period(b"ACAC") == 2 and ks.period(b"ACACA") == 5
    assert ks.equal_bytes(b"AAAC" * 3) == 12 and ks.equal_bytes(b"AAACGAAACT") == 4 and ks.equal_bytes(b"AAACG") == 0
    rng = np.random.default_rng(1)
    for _ in range(300):
        n = int(rng.integers(4, 60))
        s = ks.rand(rng, (b"AC", b"ACGT")[n % 2], n)
        if rng.random() < 0.4:
            s = (s[:max(1, n // 4)] * 5)[:n + n % 3]
        assert ks.candidates(s) == _naive_candidates(s), s
        assert ks.period(s) == min(d for d in range(1, len(s) + 1) if len(s) % d == 0 and s == s[d:] + s[:d]), s
        # the least rotation starts at a candidate -- the first of those the rounds leave (none: a homopolymer, index 0)
        at = orc.booth_least_rotation(s)
        assert at in ks.candidate_positions(s) if ks.candidates(s) else at == 0, s
        assert ks.revcomp(ks.revcomp(s)) == s and ks.period(ks.revcomp(s)) == ks.period(s)


# ---------------------------------------------------------------- the families
def test_every_family_comes_in_both_sizes():
    assert {m.family for m in MEMBERS} == set(ks.FAMILIES)
    for f in ks.FAMILIES:
        assert {m.size for m in MEMBERS if m.family == f} == {1, 2}, f
    assert ks.GLOBAL_MIN == 122_857 and ks.GLOBAL_MIN + 24 == 120 * 1024 + 1
    assert len(ks.edge_below()) == 122_856 and [len(m.seq) for m in MEMBERS if m.family == "edge"] == [7168, 122_857]
    # the candidate-count families pass the list's 1,024 entries by one at size one
    for f in ("closed_full", "open_full"):
        assert {ks.candidates(m.seq) for m in MEMBERS if m.family == f and m.size == 1} == {ks.LIST_CAP + 1}
    for size in (1, 2):
        names = [n for n, _ in ks.inputs(size)]
        assert len(names) == len(set(names)) and sum(len(b[0]) for b in ks.batches(size)) == len(names)
        assert sorted(n for b in ks.batches(size) for n in b[0]) == sorted(names)


@pytest.mark.parametrize("mb", MEMBERS, ids=IDS)
def test_family_member(mb):
    fam, t, r = ks.FAMILIES[mb.family], mb.seq, ks.revcomp(mb.seq)
    n = len(t)
    assert set(t) <= set(b"ACGT") and len(r) == n and ks.revcomp(r) == t
    assert n <= ks.WAVE_SEQ_MAX if mb.size == 1 else n >= ks.GLOBAL_MIN
    c, cr, p, eq, eqr = ks.candidates(t), ks.candidates(r), ks.period(t), ks.equal_bytes(t), ks.equal_bytes(r)
    print(mb.family, mb.size, n, "candidates", c, cr, "period", p, "equal bytes", eq, eqr)
    # the forward strand, and its counterpart on the reverse complement
    assert _within(c, mb.cand) and _within(cr, mb.rc_cand), (c, cr)
    assert n % p == 0 and ks.period(r) == p
    if fam.closed is not None:
        assert (p < n) == fam.closed
    if fam.stalls is not None:
        assert (eq > ks.STALL_BYTES) == fam.stalls
    if mb.family in ("closed_full", "brim") and p < n:   # the candidates are one block apart: the restart's condition
        assert n % c == 0 and (n // c) % p == 0 and cr == c
    if mb.family == "closed_block":                     # either the restart on a long block or copies that stay equal
        assert (n // c) % p == 0 if n % c == 0 and c * p == n else eq > ks.STALL_BYTES
    # the two strands differ, and the strand the family is built on is the one the hash keeps -- as the second strand when
    # the reverse complement is what is passed in
    a, b = orc.rotate_sequence(t), orc.rotate_sequence(r)
    assert a != b and (a > b) == mb.loses


def test_closed_block_has_both_forms():
    """a closed repeat with one candidate per copy restarts on its block, one with several runs out of rounds"""
    for size in (1, 2):
        forms = {ks.candidates(m.seq) * ks.period(m.seq) == len(m.seq) for m in MEMBERS if m.family == "closed_block" and m.size == size}
        assert forms == {True, False}


@pytest.mark.parametrize("size", [1, 2])
def test_hashed_inputs_have_two_different_strands(size):
    """Hash(circular, double-stranded) keeps the smaller of the two rotated strands: with equal strands, or where the
    forward strand wins, a wrong second-strand index does not reach the hash.  Every input is there as t and as
    revcomp(t), the strands differ, so the second strand is the strictly smaller one in exactly one of the two."""
    ins = dict(ks.inputs(size))
    for name, t in ins.items():
        if name.endswith(".rc"):
            continue
        r = ins[name + ".rc"]
        assert r == ks.revcomp(t) and set(t) <= set(b"ACGT")
        a, b = orc.rotate_sequence(t), orc.rotate_sequence(r)
        assert a != b, name
        second_wins = [orc.rotate_sequence(ks.revcomp(x)) < orc.rotate_sequence(x) for x in (t, r)]
        assert sorted(second_wins) == [False, True], name
        # ... and the oracle's hash is the smaller strand's, whichever is passed in
        h = orc.seqhash(t, "DNA", True, True)
        assert h == orc.seqhash(r, "DNA", True, True)
        assert h[7:] == orc.seqhash(min(a, b), "DNA", False, False)[7:], name


@pytest.mark.parametrize("size", [1, 2])
def test_forward_winner_with_a_full_reverse_list(size):
    """the check that the GPU test can fail at all: an input whose own strand wins while its reverse complement has more
    than 1,024 candidates.  Its single-stranded hash differs from its reverse complement's, the double-stranded one is
    the same for both (the GPU test asserts that of HashBatch)."""
    picked = ks.forward_wins_full_reverse(size)
    assert any(name.startswith("open_full") for name, _ in picked)
    for name, t in picked:
        r = ks.revcomp(t)
        assert ks.candidates(r) > ks.LIST_CAP
        assert orc.seqhash(t, "DNA", True, False) != orc.seqhash(r, "DNA", True, False)
        assert orc.seqhash(t, "DNA", True, True) == orc.seqhash(r, "DNA", True, True)


# ---------------------------------------------------------------- many short sequences
def test_many_short():
    n_seq = 40_000
    seqs, kinds = ks.many_short(n_seq)
    lens = np.array([len(s) for s in seqs])
    assert len(seqs) == len(kinds) == n_seq and lens.max() <= 300
    assert 10 <= (lens == 0).sum() <= 40 and 10 <= (lens == 1).sum() <= 40
    assert all(set(s) <= set(b"ACGT") for s in seqs)
    assert 0.05 * n_seq <= sum(1 for k in kinds if k) <= 0.15 * n_seq
    # every small family at least once, with the property it is named for
    held = {k: 0 for k in ks.SMALL}
    for s, k in zip(seqs, kinds):
        if k and k in ks.small_kind(s):
            held[k] += 1
    print(held)
    assert all(v >= 20 for v in held.values()), held
    # neighbours in batch order: a long sequence right before a short one and the other way round
    d = np.diff(lens)
    assert (d > 100).sum() > 0.4 * n_seq and (d < -100).sum() > 0.4 * n_seq
    # ... and between the sequences one wave takes in turn (8,192 apart), while every wave takes several
    assert n_seq > 4 * ks.WAVE_STRIDE
    dw = lens[ks.WAVE_STRIDE:] - lens[:-ks.WAVE_STRIDE]
    assert (dw > 100).sum() > 0.4 * len(dw) and (dw < -100).sum() > 0.4 * len(dw)
    # the workgroup kernels read n / 8192 = 4 marks at a time and go round their grid of 8,192 workgroups more than once;
    # with the wave limit at 100 bytes about half the marks of a chunk are set
    assert n_seq // 8192 == 4 and n_seq > 8192 * 4
    marked = (lens > 100).reshape(-1, 4).sum(axis=1)
    assert set(np.unique(marked)) >= {1, 2} and marked.max() < 4 and (marked == 2).mean() > 0.9
    # no sequence of two or more bytes has equal strands
    for s in seqs:
        assert len(s) < 2 or orc.rotate_sequence(s) != orc.rotate_sequence(ks.revcomp(s))


# ---------------------------------------------------------------- why the new inputs exist
def test_named_cases_that_are_not_what_they_were_named_for():
    """tests/test_seqhash_gpu.py test_wave_and_workgroup_kernels_agree: the two inputs once commented "list full" and
    "least word wraps" have ONE forward candidate (the seam makes one run AAAA) -- only their reverse complements, which
    nothing searched, have a full list --, and in GATTACA x 700 + GAT the seam's ...ACAGATGA wins the first round over
    every ...ACAGATTA, so no round stalls."""
    for t, rc_count in zip(ks.ONE_CANDIDATE_IN_NAME_OF_MANY, (1499, 2028)):
        assert ks.candidates(t) == 1 and ks.candidates(ks.revcomp(t)) == rc_count
    t = ks.STALLED_IN_NAME_ONLY
    assert ks.candidates(t) == 700 and ks.period(t) == len(t) and ks.equal_bytes(t) == 4
