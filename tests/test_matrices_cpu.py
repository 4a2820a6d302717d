"""The canned substitution tables of search/align/matrix/matrices.go as a fixture (tests/golden/matrices.json, written by
tests/golden/make_golden.py), and the CPU oracle pinned on a published protein alignment that does not come from this code
base: Durbin, Eddy, Krogh & Mitchison, Biological Sequence Analysis (1998), section 2.3, HEAGAWGHEE vs PAWHEAE with
BLOSUM50 and a linear gap of -8 (local score 28, global score 1)."""
import json
import os

import numpy as np
import pytest

import oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrices.json")
PROTEIN = "-ABCDEFGHIJKLMNPQRSTVWXYZ*"


@pytest.fixture(scope="module")
def tables():
    with open(GOLDEN) as f:
        return json.load(f)


def _omat(t):
    return orc.SubstitutionMatrix(t["alphabet"], t["alphabet"], t["scores"])


def test_fixture_shape(tables):
    assert len(tables) == 78
    assert tables["NUC_4"]["alphabet"] == "-ACGT"
    assert tables["NUC_4_4"]["alphabet"] == "-ACMGRSVTWYHKDBN"
    for name, t in tables.items():
        s = np.array(t["scores"])
        n = len(t["alphabet"])
        assert len(set(t["alphabet"])) == n, name
        assert s.shape == (n, n), name
        assert (s == s.T).all(), name
        assert (s[0] == 0).all() and (s[:, 0] == 0).all(), name   # the gap symbol '-' scores 0 against everything
        if name not in ("NUC_4", "NUC_4_4"):
            assert t["alphabet"] == PROTEIN, name
            j = PROTEIN.index("J")
            assert (s[j] == 0).all() and (s[:, j] == 0).all(), name  # J (I/L) is listed but not defined


def _at(t, a, b):
    return t["scores"][t["alphabet"].index(a)][t["alphabet"].index(b)]


def test_hand_checked_entries(tables):
    assert _at(tables["BLOSUM62"], "W", "W") == 11
    assert _at(tables["BLOSUM62"], "A", "A") == 4
    assert _at(tables["BLOSUM62"], "W", "C") == -2
    assert _at(tables["PAM250"], "W", "W") == 17
    assert _at(tables["PAM250"], "C", "C") == 12
    assert _at(tables["IDENTITY"], "A", "C") == -10000
    assert _at(tables["IDENTITY"], "A", "A") == 1
    assert _at(tables["NUC_4_4"], "A", "N") == -2
    assert _at(tables["NUC_4_4"], "A", "M") == 1
    ranges = {"BLOSUM62": (-4, 11), "PAM30": (-17, 13), "PAM500": (-9, 34), "IDENTITY": (-10000, 1), "MATCH": (-1, 1)}
    for name, (lo, hi) in ranges.items():
        s = np.array(tables[name]["scores"])
        assert (int(s.min()), int(s.max())) == (lo, hi), name


def test_nuc4_matches_the_package(tables):
    from poly_amd import matrix
    assert tables["NUC_4"]["scores"] == matrix.NUC_4
    assert tables["NUC_4"]["scores"] == orc.NUC_4_SCORES


def _dp(a, b, t, gap, local):
    """an independent textbook DP (score only) over the fixture's table"""
    idx = {c: i for i, c in enumerate(t["alphabet"])}
    s = t["scores"]
    prev = [0 if local else j * gap for j in range(len(b) + 1)]
    best = 0
    for i in range(1, len(a) + 1):
        cur = [0 if local else i * gap]
        for j in range(1, len(b) + 1):
            h = max(prev[j - 1] + s[idx[a[i - 1]]][idx[b[j - 1]]], prev[j] + gap, cur[j - 1] + gap)
            cur.append(max(h, 0) if local else h)
            best = max(best, cur[j])
        prev = cur
    return best if local else prev[-1]


def test_durbin_local(tables):
    """Durbin et al. section 2.3 (figure 2.5): the best local alignment is AWGHE / AW-HE, score 28"""
    t = tables["BLOSUM50"]
    score, sa, sb, ea, eb = orc.smith_waterman("HEAGAWGHEE", "PAWHEAE", _omat(t), -8)
    assert score == 28 == _dp("HEAGAWGHEE", "PAWHEAE", t, -8, True)
    assert (sa, sb) == ("AWGHE", "AW-HE")   # the only alignment that scores 28
    assert (ea, eb) == (9, 5)
    # the same pair the other way round: the table is symmetric, so the score and the alignment mirror
    assert orc.smith_waterman("PAWHEAE", "HEAGAWGHEE", _omat(t), -8)[:3] == (28, "AW-HE", "AWGHE")


def test_durbin_global(tables):
    """Durbin et al. section 2.3 (figure 2.4): global score 1, alignment HEAGAWGHE-E / --P-AW-HEAE.  The reference's
    traceback stops as soon as either index reaches 0 (align.go:141), so the two leading H E / - - columns are not emitted"""
    t = tables["BLOSUM50"]
    score, sa, sb = orc.needleman_wunsch("HEAGAWGHEE", "PAWHEAE", _omat(t), -8)
    assert score == 1 == _dp("HEAGAWGHEE", "PAWHEAE", t, -8, False)
    assert (sa, sb) == ("HEAGAWGHE-E"[2:], "--P-AW-HEAE"[2:])


@pytest.mark.parametrize("name", ["BLOSUM62", "PAM30", "PAM500", "GONNET", "NUC_4_4"])
def test_oracle_scores_match_an_independent_dp(tables, name):
    """the oracle's SW / NW scores over random sequences of a table's own alphabet (gap and J included) equal the
    independent DP above"""
    t = tables[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    letters = list(t["alphabet"])
    om = _omat(t)
    for k in range(20):
        a = "".join(rng.choice(letters, int(rng.integers(0, 40))))
        b = "".join(rng.choice(letters, int(rng.integers(0, 40))))
        gap = [-1, -4, -9, 0, 1][k % 5]
        assert orc.smith_waterman(a, b, om, gap)[0] == _dp(a, b, t, gap, True), (a, b, gap)
        assert orc.needleman_wunsch(a, b, om, gap)[0] == _dp(a, b, t, gap, False), (a, b, gap)
