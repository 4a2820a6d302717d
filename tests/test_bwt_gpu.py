"""search/bwt on the GPU against the CPU oracle (tests/bwt_oracle.py) and the reference's own tables
(tests/golden/bwt/).  Every test runs in both occurrence layouts: "auto" (nucleotide for <= 4 distinct bytes) and
"general" (POLYHIP_BWT_GENERAL=1 forces the byte layout on DNA too)."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bwt_oracle as bo  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(HERE, "golden", "bwt", "reference_tables.json")))
PANGRAM = GOLD["pangram_base"] * GOLD["pangram_repeat"]


@pytest.fixture(params=["auto", "general"])
def layout(request, monkeypatch):
    if request.param == "general":
        monkeypatch.setenv("POLYHIP_BWT_GENERAL", "1")
    else:
        monkeypatch.delenv("POLYHIP_BWT_GENERAL", raising=False)
    return request.param


def _new(seq, layout):
    from poly_amd import bwt
    idx = bwt.New(seq)
    distinct = len(set(seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)))
    assert idx.Layout() == ("nucleotide" if layout == "auto" and distinct <= 4 else "general")
    return idx


def _dna(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


# ---------------------------------------------------------------- the reference's tables
def test_reference_tables(layout):
    idx = _new(PANGRAM, layout)
    o = bo.Oracle(PANGRAM.encode(), width=16)
    assert idx.Len() == len(PANGRAM)
    assert idx.GetTransform() == GOLD["transform"]
    for pat, want in GOLD["count"]:
        assert idx.Count(pat) == want, pat
    for pat, want in GOLD["locate_sorted"]:
        got = idx.Locate(pat)
        if not want:
            assert got is None, pat
            continue
        assert got == o.locate(pat.encode()), pat          # the reference's row order, unsorted
        assert sorted(got) == want, pat
    for a, b, want in GOLD["extract"]:
        assert idx.Extract(a, b) == want
    assert idx.Extract(0, idx.Len()) == PANGRAM
    bang = PANGRAM + GOLD["reconstruction_extra"]
    assert _new(bang, layout).Extract(0, len(bang)) == bang


def test_reference_examples_and_errors(layout):
    ex = GOLD["examples"]
    idx = _new(ex["sequence"], layout)
    assert sorted(idx.Locate("GCC")) == ex["locate_sorted_GCC"]
    assert idx.Count("CG") == ex["count_CG"]
    assert sorted(idx.Locate("CG")) == ex["locate_sorted_CG"]
    assert idx.Extract(48, 54) == ex["extract_48_54"]
    ban = _new("banana", layout)
    assert ban.GetTransform() == ex["transform_banana"] and ban.Len() == GOLD["len"]["len"]
    for a, b, msg in GOLD["errors"]["extract_banana"]:
        if msg is None:
            assert ban.Extract(a, b) == "banana"
        else:
            with pytest.raises(ValueError) as ei:
                ban.Extract(a, b)
            assert str(ei.value) == msg
    for call in (ban.Count, ban.Locate):
        with pytest.raises(ValueError) as ei:
            call("")
        assert str(ei.value) == GOLD["errors"]["empty_pattern"]
    seq, pat, want = GOLD["errors"]["lf_search_invalid_char"]
    s, e, err = _new(seq, layout).Intervals([pat])
    assert [int(s[0]), int(e[0]), int(err[0])] == want + [0]


# ---------------------------------------------------------------- suffix array and L
def _check_index(seq: bytes, layout, max_rounds=None):
    idx = _new(seq, layout)
    T = bo.text(seq)
    sa = bo.suffix_array(T) if len(T) > 12 else bo.suffix_array_brute(T)
    got = idx.SuffixArray()
    assert got.shape == sa.shape and (got == sa).all(), f"suffix array differs (n={len(seq)})"
    assert idx.GetTransform() == bo.last_column(T, sa)
    if max_rounds is not None:
        assert idx.Rounds() <= max_rounds, (idx.Rounds(), max_rounds)
    return idx


@pytest.mark.parametrize("n", [1, 2, 3, 31, 447, 448, 449, 895, 896, 4095, 4096, 4097, 65_537, 1_000_003, 5_000_000])
def test_suffix_array_random_dna(layout, n):
    _check_index(_dna(np.random.default_rng(n), n), layout)


def test_suffix_array_one_symbol(layout):
    n = 1 << 20
    # longest repeat n - 1: ceil(log2(n - 1)) + 1 rounds at most (round 0 already covers 64 symbols)
    idx = _check_index(b"A" * n, layout, max_rounds=math.ceil(math.log2(n - 1)) + 1)
    assert idx.Count("A" * 1000) == n - 999
    assert idx.Count("A" * n) == 1 and idx.Count("A" * (n + 1)) == 0


def test_suffix_array_tandem_repeats(layout):
    k = 1 << 18
    _check_index(b"ACGT" * k, layout, max_rounds=math.ceil(math.log2(4 * k)) + 1)
    _check_index((GOLD["pangram_base"] * 40).encode(), layout, max_rounds=math.ceil(math.log2(112 * 40)) + 1)


@pytest.mark.parametrize("case", ["specials", "two", "all255", "high"])
def test_suffix_array_general_alphabets(layout, case):
    rng = np.random.default_rng({"specials": 1, "two": 2, "all255": 3, "high": 4}[case])
    if case == "specials":
        alpha = np.frombuffer(b"\x00!#\x80\xffAz", np.uint8)
    elif case == "two":
        alpha = np.frombuffer(b"\x00\xff", np.uint8)
    elif case == "all255":
        alpha = np.array([b for b in range(256) if b != 0x24], np.uint8)
    else:
        alpha = np.arange(0x80, 0x100, dtype=np.uint8)
    for n in (1, 100, 70_001, 600_000):
        seq = alpha[rng.integers(0, len(alpha), n)].tobytes()
        if case == "all255" and n >= 255:
            seq = bytes(alpha) + seq[255:]
        idx = _check_index(seq, layout)
        o = bo.Oracle(seq, width=8)
        pats = [seq[i:i + 5] for i in rng.integers(0, max(n - 5, 1), 200)] + [bytes([b]) for b in alpha[:40]]
        pats += [b"$" + seq[:3], seq[-2:] + b"$", b"\x24\x24", bytes([0x24, 0x00])]
        s, e, err = idx.Intervals(pats)
        for p, a, b in zip(pats, s, e):
            assert (int(a), int(b)) == o.interval(p), p


# ---------------------------------------------------------------- counts and locate at size
@pytest.fixture(scope="module")
def genome():
    rng = np.random.default_rng(20)
    n = 5_000_000
    seq = _dna(rng, n)
    npat, m = 1_000_000, 32
    g = np.frombuffer(seq, np.uint8)
    starts = rng.integers(0, n - m, npat)
    pats = g[starts[:, None] + np.arange(m)]
    mut = pats[npat // 2:]
    pos = rng.integers(0, m, (len(mut), 2))
    for q in range(2):
        mut[np.arange(len(mut)), pos[:, q]] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(mut))]
    o = bo.Oracle(seq, width=m)
    ws, we = o.intervals_fixed(pats)
    return seq, pats, o, ws, we


def test_counts_at_size(layout, genome):
    seq, pats, o, ws, we = genome
    idx = _new(seq, layout)
    assert (idx.SuffixArray() == o.sa).all()
    offs = np.arange(0, pats.size + 1, pats.shape[1], dtype=np.uint64)
    s, e, err = idx.intervals_packed(pats.reshape(-1), offs)
    assert not err.any()
    assert (s == ws).all() and (e == we).all(), f"{int(((s != ws) | (e != we)).sum())} intervals differ"
    # Locate on a 50k sample, in row order
    rng = np.random.default_rng(3)
    sample = rng.choice(len(pats), 50_000, replace=False)
    sub = pats[sample]
    first, got = idx.locate_packed(sub.reshape(-1), np.arange(0, sub.size + 1, sub.shape[1], dtype=np.uint64))
    want = np.concatenate([o.sa[a:b] for a, b in zip(ws[sample], we[sample])])
    assert int(first[-1]) == len(want) and (got == want).all()


def test_pattern_kinds(layout, genome):
    seq = genome[0][:200_000]
    idx = _new(seq, layout)
    o = bo.Oracle(seq, width=24)
    pats = [b"A", b"C", b"G", b"T", b"N", b"AN", b"a", b"$", b"$A", b"T$", seq[-5:] + b"$" + seq[:5],
            b"$" + seq[:20], seq[-3:] + b"$"]
    s, e, err = idx.Intervals(pats)
    for p, a, b in zip(pats, s, e):
        assert (int(a), int(b)) == o.interval(p), p
    assert sum(int(b) - int(a) for a, b in zip(s[:4], e[:4])) == len(seq)   # the 1-mers cover every row but '$'
    # an empty pattern in a batch: flagged, the others unaffected
    s2, e2, err2 = idx.Intervals([b"ACG", b"", b"TTA"])
    assert list(err2) == [0, 1, 0] and (int(s2[1]), int(e2[1])) == (0, 0)
    assert (int(s2[0]), int(e2[0])) == o.interval(b"ACG") and (int(s2[2]), int(e2[2])) == o.interval(b"TTA")
    # longer than T: cyclic
    small = _new(b"GATTACA", layout)
    ob = bo.Oracle(b"GATTACA", width=40)
    for p in (b"GATTACA$GATTACA$GA", b"A$GATTACA$GATTACA$GATTACA", b"GATTACA$GATTACA$GATTACAA", b"CA$GAT"):
        assert small.Count(p) == ob.count(p) == bo.interval_brute(b"GATTACA", p)[1] - bo.interval_brute(b"GATTACA", p)[0]
        assert (small.Locate(p) or []) == ob.locate(p)


def test_extract_errors_in_order(layout):
    seq = "GATTACAGATTACA"
    idx = _new(seq, layout)
    n = len(seq)
    reqs = [(5, 4), (4, 4), (-3, -5), (20, 3), (0, n + 1), (-1, n + 1), (-1, 3), (-5, 0), (0, n), (3, 9), (n - 1, n)]
    res, err = idx.extract_raw(reqs)
    assert list(err) == [1, 1, 1, 1, 2, 2, 3, 3, 0, 0, 0]
    assert [r for r in res if r is not None] == [seq.encode(), seq[3:9].encode(), seq[-1:].encode()]
    big = _dna(np.random.default_rng(9), 300_001)
    assert _new(big, layout).Extract(0, len(big)) == big


def test_locate_capacity(layout):
    from poly_amd import _lib
    idx = _new("banana", layout)
    with pytest.raises(_lib.PolyhipError) as ei:
        idx.LocateBatch(["a", "na"], capacity=4)
    assert ei.value.status == _lib.ERR_INVALID and "need 5 entries" in ei.value.message
    buf, offs = np.frombuffer(b"ana", np.uint8), np.array([0, 1, 3], np.uint64)
    first = np.zeros(3, np.uint64)
    out = np.zeros(4, np.uint32)
    err = np.zeros(2, np.uint32)
    st = _lib.lib().polyhip_bwt_locate(idx.handle(), buf.ctypes.data, offs.ctypes.data, 2, first.ctypes.data,
                                       out.ctypes.data, 4, err.ctypes.data)
    assert st == _lib.ERR_INVALID and list(first) == [0, 3, 5] and not out.any()
    first, got = idx.LocateBatch(["a", "na"], capacity=5)
    assert list(first) == [0, 3, 5] and list(got) == [5, 3, 1, 4, 2]


@pytest.mark.parametrize("npat", [4096, 4097])
def test_locate_at_the_scan_tile_edge(layout, npat):
    """The offsets of a Locate batch are a uint64 scan over the patterns: 4096 of them are the most its single block takes,
    4097 the fewest that go through block sums."""
    rng = np.random.default_rng(npat)
    seq = _dna(rng, 200)
    idx = _new(seq, layout)
    o = bo.Oracle(seq, width=4)
    pats = [_dna(rng, int(m)) for m in rng.integers(1, 5, npat)]      # 1-mers with ~50 rows down to 4-mers, some absent
    want = [np.array(o.locate(p), np.int64) for p in pats]
    first, got = idx.LocateBatch(pats)
    assert (first == np.concatenate([[0], np.cumsum([len(w) for w in want])])).all()
    assert (got == np.concatenate(want)).all()


# ---------------------------------------------------------------- device-resident entry points
def test_dev_entry_points(layout):
    import torch
    from poly_amd import bwt, mash
    dev = torch.device("cuda:0")
    n = 300_000
    seq_t = torch.empty(n, dtype=torch.uint8, device=dev)
    mash.synth_dna_dev(0xB0, seq_t)
    seq = seq_t.cpu().numpy().tobytes()
    idx = bwt.new_dev(seq_t)
    ref = _new(seq, layout)
    assert idx.Layout() == ref.Layout()
    assert (idx.SuffixArray() == ref.SuffixArray()).all()
    L_t = torch.empty(n + 1, dtype=torch.uint8, device=dev)
    bwt.transform_dev(idx, L_t)
    torch.cuda.synchronize()
    assert L_t.cpu().numpy().tobytes() == ref.GetTransform()
    rng = np.random.default_rng(4)
    pats = [seq[i:i + 12] for i in rng.integers(0, n - 12, 5000)] + [b"", b"ACGTN"]
    buf, offs = bwt._pack(pats)
    pat_t = torch.from_numpy(buf.copy()).to(dev)
    off_t = torch.from_numpy(offs.view(np.int64).copy()).to(dev)
    s_t = torch.empty(len(pats), dtype=torch.int32, device=dev)
    e_t, err_t = torch.empty_like(s_t), torch.empty_like(s_t)
    bwt.count_dev(idx, pat_t, off_t, s_t, e_t, err_t)
    hs, he, herr = ref.Intervals(pats)
    assert (s_t.cpu().numpy().view(np.uint32) == hs).all() and (e_t.cpu().numpy().view(np.uint32) == he).all()
    assert (err_t.cpu().numpy() == herr.astype(np.int32)).all()
    first_t = torch.empty(len(pats) + 1, dtype=torch.int64, device=dev)
    total = int((he.astype(np.int64) - hs).sum())
    out_t = torch.empty(total, dtype=torch.int32, device=dev)
    bwt.locate_dev(idx, s_t, e_t, first_t, out_t)
    torch.cuda.synchronize()
    first = first_t.cpu().numpy()
    assert int(first[-1]) == total
    sa = ref.SuffixArray()
    want = np.concatenate([sa[a:b] for a, b in zip(hs, he)])
    assert (out_t.cpu().numpy().view(np.uint32) == want).all()
    # Extract: two valid requests and one failing
    st_t = torch.tensor([10, 5, -1], dtype=torch.int64, device=dev)
    en_t = torch.tensor([20, 5, 4], dtype=torch.int64, device=dev)
    oo_t = torch.tensor([0, 10, 10, 10], dtype=torch.int64, device=dev)
    ob_t = torch.zeros(10, dtype=torch.uint8, device=dev)
    er_t = torch.empty(3, dtype=torch.int32, device=dev)
    bwt.extract_dev(idx, st_t, en_t, oo_t, ob_t, er_t)
    torch.cuda.synchronize()
    assert ob_t.cpu().numpy().tobytes() == seq[10:20] and list(er_t.cpu().numpy()) == [0, 1, 3]
    # the reference's New error from a device text
    bad = torch.tensor(list(b"ACG$T"), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError) as ei:
        bwt.new_dev(bad)
    assert str(ei.value) == GOLD["errors"]["new_nullchar"][1]
