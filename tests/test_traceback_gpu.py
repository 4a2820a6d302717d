"""K3b parity: the full align.SmithWaterman (score + aligned strings) in HIP vs the
CPU oracle's restatement of align.go:171-232.  Strings must be identical, including the
reference's tie-breaking (first row-major maximum; diagonal, then up, then left).

Mirrors search/align/align_test.go:139-292 and example_test.go:49-111."""
import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

MAT3 = [[0, 0, 0, 0, 0], [0, 3, -3, -3, -3], [0, -3, 3, -3, -3], [0, -3, -3, 3, -3], [0, -3, -3, -3, 3]]


@pytest.fixture(scope="module")
def al():
    from poly_amd import align, alphabet, matrix
    return align, alphabet, matrix


@pytest.fixture(autouse=True, params=["half", "int32"])
def tb_cell(request, monkeypatch):
    """every test runs twice: with the byte-profile traceback in its half-float two-band form where it applies (gfx950,
    scores below 2048: the default) and with POLYHIP_TB_F16=0 (the 32-bit form everywhere)"""
    if request.param == "int32":
        monkeypatch.setenv("POLYHIP_TB_F16", "0")
    else:
        monkeypatch.delenv("POLYHIP_TB_F16", raising=False)
    return request.param


def _scoring(al, symbols, scores, gap):
    align, alphabet, matrix = al
    a = alphabet.NewAlphabet(list(symbols))
    return align.NewScoring(matrix.NewSubstitutionMatrix(a, a, scores), gap)


def _pack(seqs):
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), np.uint8).copy(), offs


def _oracle_sw_threaded(pairs, om, gap):
    """orc.smith_waterman of every (read, reference) pair on all host cores (ctypes releases the GIL): (score, alnA, alnB,
    endA, endB) per pair, strings as bytes"""
    import concurrent.futures as cf
    import os

    def one(ab):
        s, sa, sb, ea, eb = orc.smith_waterman(ab[0], ab[1], om, gap)
        return s, sa if isinstance(sa, bytes) else sa.encode(), sb if isinstance(sb, bytes) else sb.encode(), ea, eb
    with cf.ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as ex:
        return list(ex.map(one, pairs))


def _mutate(rng, seq: bytes, sub=0.05, indel=0.01) -> bytes:
    out = bytearray()
    for c in seq:
        r = rng.random()
        if r < indel / 2:
            continue
        if r < indel:
            out.append(int(rng.choice(list(b"ACGT"))))
        out.append(int(rng.choice(list(b"ACGT"))) if rng.random() < sub else c)
    return bytes(out)


def _check(al, scoring, omat, gap, reads, ref=None, refs=None):
    align = al[0]
    A, offA = _pack(reads)
    if refs is None:
        B, _ = _pack([ref])
        got = align.sw_align_packed(scoring, A, offA, B, None)
        refs = [ref] * len(reads)
    else:
        B, offB = _pack(refs)
        got = align.sw_align_packed(scoring, A, offA, B, offB)
    for p, (a, b) in enumerate(zip(reads, refs)):
        try:
            sc, sa, sb, ea, eb = orc.smith_waterman(a, b, omat, gap)
        except orc.AlphabetError:
            assert int(got[3][p]) != 0 and got[4][p] == b"" and got[5][p] == b""
            continue
        sa = sa if isinstance(sa, bytes) else sa.encode("latin-1")
        sb = sb if isinstance(sb, bytes) else sb.encode("latin-1")
        g = (int(got[0][p]), got[4][p], got[5][p])
        assert g == (sc, sa, sb), f"pair {p}: got {g} want {(sc, sa, sb)}"


def test_TestSmithWaterman(al):
    """search/align/align_test.go:139-292"""
    align = al[0]
    sc = _scoring(al, "-ACGT", MAT3, -2)
    assert align.SmithWaterman("TGTTACGG", "GGTTGACTA", sc) == (13, "GTT-AC", "GTTGAC")      # :158-175
    assert align.SmithWaterman("ACACACTA", "AGCACACA", sc) == (17, "A-CACACTA", "AGCACAC-A")  # :177-194
    for a, b in (("", "GAT"), ("GAT", ""), ("", ""), ("G", "A")):                                # :199-291
        assert align.SmithWaterman(a, b, sc) == (0, "", "")
    assert align.SmithWaterman("G", "G", sc) == (3, "G", "G")


def test_examples(al):
    """search/align/example_test.go:49-111"""
    align = al[0]
    pm1 = (2 * np.eye(5, dtype=int) - 1).tolist()
    assert align.SmithWaterman("GATTACA", "GCATGCU", _scoring(al, "ACGTU", pm1, -1)) == (2, "AT", "AT")
    assert align.SmithWaterman("GATTACA", "GCATGCT", _scoring(al, "ACGT-", al[2].NUC_4, -1)) == (15, "GATTAC", "GCATGC")
    with pytest.raises(al[1].Error, match="Symbol X not in alphabet"):
        align.SmithWaterman("GAXTACA", "GCATGCT", _scoring(al, "ACGT-", al[2].NUC_4, -1))


def test_config4_shape(al):
    """BASELINE config 4 shape: 150 bp reads (5 % subs, 1 % indels) vs one 5 kb reference, NUC_4, gap -2:
    the windowed re-DP (at most 902 of 5000 columns) must reproduce the full-matrix traceback"""
    rng = np.random.default_rng(0xC4)
    ref = orc.synth_dna(0xC4, 5000).tobytes()
    reads = []
    for _ in range(400):
        p = int(rng.integers(0, 5000 - 150))
        reads.append(_mutate(rng, ref[p:p + 150])[:152])
    reads += [orc.synth_dna(99, 150).tobytes(), b"", b"A", ref[:152], ref[-150:], ref[2000:2150]]
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    _check(al, sc, om, -2, reads, ref=ref)


@pytest.mark.parametrize("chunks", ["3", "8"])
def test_host_flavour_chunk_pipeline_equals_single_shot(al, monkeypatch, chunks):
    """polyhip_sw_align_batch sends large batches through two slots in chunks of pairs (the strings of one chunk
    cross PCIe while the next is aligned); POLYHIP_SW_HOST_CHUNKS forces the chunk count here.  Same scores, end
    cells, errors and strings as the single shot (a ragged batch with bad symbols and empty reads whose size is no
    multiple of the chunk count), a sample against the oracle."""
    align = al[0]
    rng = np.random.default_rng(int(chunks))
    ref = orc.synth_dna(0xC4, 3000).tobytes()
    reads = []
    for i in range(20_003):
        p = int(rng.integers(0, 3000 - 150))
        r = _mutate(rng, ref[p:p + int(rng.integers(1, 151))])[:152]
        if i % 997 == 0:
            r = b"" if i % 2 else r[:5] + b"N" + r[6:]
        reads.append(r)
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    A, offA = _pack(reads)
    B, _ = _pack([ref])
    monkeypatch.setenv("POLYHIP_SW_HOST_CHUNKS", "1")
    one = align.sw_align_packed(sc, A, offA, B, None)
    monkeypatch.setenv("POLYHIP_SW_HOST_CHUNKS", chunks)
    got = align.sw_align_packed(sc, A, offA, B, None)
    for g, w in zip(got[:4], one[:4]):
        assert (g == w).all()
    assert got[4] == one[4] and got[5] == one[5]
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    for p in range(0, len(reads), 401):
        try:
            s_, sa, sb, _, _ = orc.smith_waterman(reads[p], ref, om, -2)
        except orc.AlphabetError:
            assert int(got[3][p]) != 0 and got[4][p] == b""
            continue
        sa = sa if isinstance(sa, bytes) else sa.encode("latin-1")
        sb = sb if isinstance(sb, bytes) else sb.encode("latin-1")
        assert (int(got[0][p]), got[4][p], got[5][p]) == (s_, sa, sb), p


@pytest.mark.parametrize("chunks", ["1", "3", "8"])
def test_packed_strings_equal_the_slots(al, monkeypatch, chunks):
    """polyhip_sw_align_batch_packed (strings compacted on the device, only their own bytes cross PCIe) against the
    fixed-stride-slot flavour on a ragged batch with bad symbols, empty reads and zero-score pairs -- same scores, end cells,
    errors and strings whatever the chunk count; a capacity that is too small is reported with the size needed and the
    Python wrapper's second attempt succeeds; per-pair references too"""
    align = al[0]
    rng = np.random.default_rng(100 + int(chunks))
    ref = orc.synth_dna(0xC4, 3000).tobytes()
    reads = []
    for i in range(20_003):
        p = int(rng.integers(0, 3000 - 150))
        r = _mutate(rng, ref[p:p + int(rng.integers(1, 151))])[:152]
        if i % 997 == 0:
            r = b"" if i % 2 else r[:5] + b"N" + r[6:]
        if i % 1499 == 0:
            r = b"-" * 30                      # scores nothing against NUC_4: an empty alignment
        reads.append(r)
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    A, offA = _pack(reads)
    B, _ = _pack([ref])
    monkeypatch.setenv("POLYHIP_SW_HOST_CHUNKS", chunks)
    slots = align.sw_align_packed(sc, A, offA, B, None)
    packed = align.sw_align_strings_packed(sc, A, offA, B, None)
    for g, w in zip(packed[:4], slots[:4]):
        assert (g == w).all()
    assert packed[4] == slots[4] and packed[5] == slots[5]
    tight = align.sw_align_strings_packed(sc, A, offA, B, None, capacity=1000)   # far too small: the retry path
    assert tight[4] == slots[4] and tight[5] == slots[5]
    # reads against reads (per-pair references: the single-shot path)
    n = 300
    pa, oa = _pack(reads[:n])
    pb, ob = _pack(reads[n:2 * n])
    s2 = align.sw_align_packed(sc, pa, oa, pb, ob)
    p2 = align.sw_align_strings_packed(sc, pa, oa, pb, ob)
    for g, w in zip(p2[:4], s2[:4]):
        assert (g == w).all()
    assert p2[4] == s2[4] and p2[5] == s2[5]


@pytest.mark.parametrize("maxlen,reflen", [(64, 300), (152, 1500), (256, 2100), (40, 3), (10, 1)])
def test_ragged(al, maxlen, reflen):
    rng = np.random.default_rng(maxlen * 7 + reflen)
    ref = orc.synth_dna(1234 + reflen, reflen).tobytes()
    reads = [orc.synth_dna(int(rng.integers(1, 1 << 30)), int(rng.integers(0, maxlen + 1))).tobytes() for _ in range(200)]
    reads[0] = orc.synth_dna(5, maxlen).tobytes()
    for i in range(1, 80):
        L = int(rng.integers(1, min(maxlen, reflen) + 1))
        p = int(rng.integers(0, reflen - L + 1))
        reads[i] = _mutate(rng, ref[p:p + L], 0.03, 0.03)[:maxlen]
    pm = [[0, 0, 0, 0, 0], [0, 2, -1, -1, -1], [0, -1, 2, -1, -1], [0, -1, -1, 2, -1], [0, -1, -1, -1, 2]]
    _check(al, _scoring(al, "-ACGT", pm, -1), orc.SubstitutionMatrix("-ACGT", "-ACGT", pm), -1, reads, ref=ref)


@pytest.mark.parametrize("maxA,maxB", [(150, 150), (64, 90), (152, 40), (100, 600)])
def test_every_pair_its_own_reference_on_packed_halves(al, monkeypatch, tb_cell, maxA, maxB):
    """reads against reads (offB given): the half-float kernel whose profile is built per lane (path 6; the 32-bit fixture and
    POLYHIP_TB_PAIR16=0: the table kernel, path 2) -- 30k pairs of ragged lengths (B of 1 .. maxB symbols, some shorter than
    a block of four; empty reads; related and unrelated pairs; a pair of tandem repeats: ties), every pair equal to the table
    kernel, a sample equal to the oracle"""
    import torch
    align = al[0]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(maxA * 1000 + maxB)
    n = 30_000
    la = rng.integers(0, maxA + 1, n)
    lb = rng.integers(1, maxB + 1, n)
    la[:50] = maxA
    lb[:50] = maxB
    lb[50:60] = rng.integers(1, 4, 10)
    src = orc.synth_dna(77, 4 * (maxA + maxB) + 64)
    As, Bs = [], []
    for p in range(n):
        o = int(rng.integers(0, len(src) - max(la[p], lb[p]) - 1))
        b = src[o:o + lb[p]].copy()
        if p % 3 == 0:      # unrelated
            a = src[(o * 7 + 13) % (len(src) - maxA - 1):][:la[p]].copy()
        else:               # a (mutated) piece of b, or b of it
            a = np.resize(b, la[p]).copy() if la[p] else b[:0].copy()
            hit = rng.random(len(a)) < 0.08
            a[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        As.append(a.tobytes())
        Bs.append(b.tobytes())
    As[60], Bs[60] = (b"ACGT" * 40)[:maxA], (b"ACGT" * 200)[:maxB]
    A, offA = _pack(As)
    Bf, offB = _pack(Bs)
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    At, oAt = torch.from_numpy(A).to(dev), torch.from_numpy(offA.astype(np.int64)).to(dev)
    Bt, oBt = torch.from_numpy(Bf).to(dev), torch.from_numpy(offB.astype(np.int64)).to(dev)
    score = torch.zeros(n, dtype=torch.int64, device=dev)
    ea, eb, er = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    work = torch.empty(align.sw_workspace_bytes(sc, n, maxA, maxB, False), dtype=torch.uint8, device=dev)
    align.sw_batch_dev(sc, At, oAt, maxA, Bt, oBt, maxB, score, ea, eb, er, work)
    stride = align.sw_traceback_stride(sc, maxA, maxB)
    tbw = torch.empty(align.sw_traceback_workspace_bytes(sc, n, maxA, maxB), dtype=torch.uint8, device=dev)
    outs = []
    for mode in ("default", "table"):
        if mode == "table":
            monkeypatch.setenv("POLYHIP_TB_PAIR16", "0")
        a = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        b = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        ln = torch.zeros(n, dtype=torch.int32, device=dev)
        align.sw_traceback_dev(sc, At, oAt, maxA, Bt, oBt, maxB, ea, eb, er, a, b, ln, tbw, score_t=score)
        torch.cuda.synchronize()
        outs.append((a, b, ln, align.sw_traceback_last_path()))
        monkeypatch.delenv("POLYHIP_TB_PAIR16", raising=False)
    assert (outs[0][3], outs[1][3]) == ((6, 2) if tb_cell == "half" else (2, 2))
    live = torch.arange(stride, device=dev)[None, :] >= (stride - outs[0][2].long())[:, None]
    assert torch.equal(outs[0][2], outs[1][2])
    assert bool(((outs[0][0] == outs[1][0]) | ~live).all()) and bool(((outs[0][1] == outs[1][1]) | ~live).all())
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    a_h, b_h, l_h, s_h = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy(), outs[0][2].cpu().numpy(), score.cpu().numpy()
    for p in list(range(0, 70)) + [int(x) for x in rng.integers(0, n, 200)]:
        ws, wa, wb, _, _ = orc.smith_waterman(As[p], Bs[p], om, -2)
        wa = wa if isinstance(wa, bytes) else wa.encode()
        wb = wb if isinstance(wb, bytes) else wb.encode()
        assert int(s_h[p]) == ws and a_h[p, stride - l_h[p]:].tobytes() == wa and b_h[p, stride - l_h[p]:].tobytes() == wb, p


def test_positive_gap_score_with_a_matrix_that_has_no_positive_entry(al):
    """found by scripts/fuzz_k3.py in round 4: align.Scoring takes any integer as GapPenalty (align.go:73-95); with a positive
    one every gap move GAINS, so cells are positive although no substitution score is -- the string slots used to be sized
    for "every H is 0" (one byte).  One reference and every pair its own."""
    mat = [[0, -8], [-1, -3]]
    sc = _scoring(al, "AC", mat, 1)
    om = orc.SubstitutionMatrix("AC", "AC", mat)
    rng = np.random.default_rng(484)
    reads = [bytes(rng.choice(list(b"AC"), int(rng.integers(0, 60))).astype(np.uint8)) for _ in range(60)]
    refs = [bytes(rng.choice(list(b"AC"), int(rng.integers(1, 130))).astype(np.uint8)) for _ in range(60)]
    _check(al, sc, om, 1, reads, ref=refs[0])
    _check(al, sc, om, 1, reads, refs=refs)


def test_ties_and_repeats(al):
    ref = (b"ACGT" * 300)[:1100]
    reads = [b"ACGT" * k for k in range(1, 30)] + [b"CGTA" * 5, b"TTTT", b"GTAC" * 30, b"A", b"ACGTTGCA" * 8]
    sc = _scoring(al, "-ACGT", MAT3, -2)
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", MAT3)
    _check(al, sc, om, -2, reads, ref=ref)
    _check(al, sc, om, -2, reads, refs=[ref] * len(reads))


def test_chunks_overlapped_on_two_streams_equal_one_after_the_other(al, monkeypatch):
    """A batch that needs several chunks of the direction workspace: the byte-profile kernels take them through the two
    halves of the workspace on two streams; POLYHIP_TB_OVERLAP=0 runs one chunk after the other. 150k config-4-like reads
    through a workspace that holds 60k pairs: seven outputs equal, a sample against the oracle; the call is followed by
    work on the caller's stream that reads the results (ordering across the two streams)."""
    import torch
    from poly_amd import workloads
    align = al[0]
    dev = torch.device("cuda:0")
    n, LA, LB = 150_000, 150, 5000
    B, A2 = workloads.config4_reads(n, LA, LB, first=123_000, device=dev)
    A = A2.reshape(-1).contiguous()
    offA = torch.arange(0, (n + 1) * LA, LA, dtype=torch.int64, device=dev)
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    score = torch.zeros(n, dtype=torch.int64, device=dev)
    ea, eb, er = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    work = torch.empty(align.sw_workspace_bytes(sc, n, LA, LB, True), dtype=torch.uint8, device=dev)
    align.sw_batch_dev(sc, A, offA, LA, B, None, LB, score, ea, eb, er, work)
    stride = align.sw_traceback_stride(sc, LA, LB)
    tbw = torch.empty(align.sw_traceback_workspace_bytes(sc, 60_000, LA, LB), dtype=torch.uint8, device=dev)
    outs = []
    for mode in ("1", "0"):
        monkeypatch.setenv("POLYHIP_TB_OVERLAP", mode)
        alnA = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        alnB = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        ln = torch.full((n,), -5, dtype=torch.int32, device=dev)
        align.sw_traceback_dev(sc, A, offA, LA, B, None, LB, ea, eb, er, alnA, alnB, ln, tbw, score_t=score)
        total = ln.long().sum()  # on the caller's stream, right behind the call
        torch.cuda.synchronize()
        outs.append((alnA, alnB, ln, int(total)))
    monkeypatch.delenv("POLYHIP_TB_OVERLAP", raising=False)
    assert outs[0][3] == outs[1][3] and torch.equal(outs[0][2], outs[1][2])
    cols = torch.arange(stride, device=dev)[None, :]
    live = cols >= (stride - outs[0][2].long())[:, None]
    assert bool(((outs[0][0] == outs[1][0]) | ~live).all()) and bool(((outs[0][1] == outs[1][1]) | ~live).all())
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    refb = B.cpu().numpy().tobytes()
    a_h, b_h, l_h, rd = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy(), outs[0][2].cpu().numpy(), A2.cpu().numpy()
    for p_ in range(0, n, 1499):
        ws, wa, wb, _, _ = orc.smith_waterman(rd[p_].tobytes(), refb, om, -2)
        wa = wa if isinstance(wa, bytes) else wa.encode("latin-1")
        wb = wb if isinstance(wb, bytes) else wb.encode("latin-1")
        L = int(l_h[p_])
        assert (int(score[p_]), a_h[p_, stride - L:].tobytes(), b_h[p_, stride - L:].tobytes()) == (ws, wa, wb), p_


def test_generic_paths(al):
    """A longer than the register tile, per-pair B, and scoring without a window bound (gap >= 0)"""
    rng = np.random.default_rng(77)
    sc = _scoring(al, "-ACGT", MAT3, -2)
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", MAT3)
    ref = orc.synth_dna(31, 700).tobytes()
    reads = [orc.synth_dna(100 + i, int(rng.integers(257, 400))).tobytes() for i in range(12)]
    reads[0] = _mutate(rng, ref[100:450])
    _check(al, sc, om, -2, reads, ref=ref)
    refs = [orc.synth_dna(500 + i, int(rng.integers(0, 300))).tobytes() for i in range(64)]
    reads = [orc.synth_dna(900 + i, int(rng.integers(0, 200))).tobytes() for i in range(64)]
    for i in range(0, 64, 3):
        reads[i] = _mutate(rng, refs[i][:150], 0.05, 0.03)
    _check(al, sc, om, -2, reads, refs=refs)
    asym = [[0, 0, 0, 0, 0], [0, 30, -7, 2, -1], [0, -10, 25, 0, 3], [0, 5, -3, 40, -9], [0, 1, 2, -30, 20]]
    for gap in (1, 0):
        _check(al, _scoring(al, "-ACGT", asym, gap), orc.SubstitutionMatrix("-ACGT", "-ACGT", asym), gap, reads[:16],
               ref=ref[:120])


def test_default_matrix(al):
    rng = np.random.default_rng(26)
    letters = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZ", np.uint8)
    ref = rng.choice(letters, 900).tobytes()
    reads = [rng.choice(letters, int(rng.integers(0, 150))).tobytes() for _ in range(100)]
    for i in range(40):
        p = int(rng.integers(0, 800))
        reads[i] = ref[p:p + int(rng.integers(5, 100))]
    _check(al, al[0].NewScoring(None, -1), orc.DEFAULT_MATRIX, -1, reads, ref=ref)


def test_device_resident_chunked_workspace(al):
    """a workspace smaller than the batch needs makes the call loop over chunks: same strings"""
    import torch
    align = al[0]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2)
    ref = orc.synth_dna(0xC4, 5000)
    refb = ref.tobytes()
    n, L = 1500, 150
    reads = [(_mutate(rng, refb[s:s + L]) + b"A" * L)[:L] for s in rng.integers(0, 5000 - L, n)]
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    A = torch.from_numpy(np.frombuffer(b"".join(reads), np.uint8).copy()).to(dev)
    offA = torch.arange(0, (n + 1) * L, L, dtype=torch.int64, device=dev)
    B = torch.from_numpy(ref.copy()).to(dev)
    score = torch.zeros(n, dtype=torch.int64, device=dev)
    ea, eb, er, ln = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4))
    work = torch.empty(align.sw_workspace_bytes(sc, n, L, 5000), dtype=torch.uint8, device=dev)
    align.sw_batch_dev(sc, A, offA, L, B, None, 5000, score, ea, eb, er, work)
    stride = align.sw_traceback_stride(sc, L, 5000)
    assert stride == 150 + 5 * 150 // 2
    full = align.sw_traceback_workspace_bytes(sc, n, L, 5000)
    small = torch.empty(full // 5, dtype=torch.uint8, device=dev)  # forces >= 5 chunks
    alnA = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    alnB = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    align.sw_traceback_dev(sc, A, offA, L, B, None, 5000, ea, eb, er, alnA, alnB, ln, small, score_t=score)
    torch.cuda.synchronize()
    a_h, b_h, l_h = alnA.cpu().numpy(), alnB.cpu().numpy(), ln.cpu().numpy()
    for p in range(0, n, 11):
        s, sa, sb, _, _ = orc.smith_waterman(reads[p], refb, om, -2)
        sa = sa if isinstance(sa, bytes) else sa.encode()
        sb = sb if isinstance(sb, bytes) else sb.encode()
        assert a_h[p, stride - l_h[p]:].tobytes() == sa and b_h[p, stride - l_h[p]:].tobytes() == sb
        assert int(score[p]) == s


@pytest.mark.parametrize("gap,LB,L", [(-2, 5000, 150), (-7, 5000, 150), (-2, 15000, 150), (-2, 5000, 250), (-7, 5000, 250)])
def test_three_kernels_and_both_window_bounds_agree(al, monkeypatch, tb_cell, gap, LB, L):
    """(gap -2: even unrelated reads score > 300, the linear phase of local alignment; gap -7: scores fall
    to the noise floor, so the per-pair windows range from the tightest to the batch-wide bound.)  200k reads at 0..90 % substitutions + 0..12 % indels (scores from 750 down to the noise floor)
    against one 5 kb reference.  The byte-profile kernel (score given), the table kernel (no score: the
    batch-wide window) and the byte-profile kernel with the conservative per-pair window
    (POLYHIP_TB_WIDE=1) must write identical alignments; a sample is checked against the oracle.
    L = 250: the 256-row instantiations (one workgroup per CU, H rows partly in AGPRs)."""
    import torch
    align = al[0]
    dev = torch.device("cuda:0")
    n = (200_000 if LB == 5000 else 60_000) * 150 // L  # 15 kb: the profile takes 120 KB of LDS
    ref = orc.synth_dna(0xC4, LB)
    B = torch.from_numpy(ref.copy()).to(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    starts = torch.randint(0, LB - L, (n,), device=dev, generator=gen)
    A = B[starts[:, None] + torch.arange(L, device=dev)[None, :]]
    rate = torch.linspace(0.0, 0.9, n, device=dev)[:, None]
    hit = torch.rand(A.shape, device=dev, generator=gen) < rate
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    A[hit] = lut[torch.randint(0, 4, (int(hit.sum()),), device=dev, generator=gen)]
    # indels: rotate a random suffix by one base (deletion + insertion at the end keeps the length)
    cut = torch.randint(1, L, (n,), device=dev, generator=gen)
    shift = (torch.rand(n, device=dev, generator=gen) < rate[:, 0] / 7.5)
    idx = torch.arange(L, device=dev)[None, :].expand(n, L)
    src = torch.where(shift[:, None] & (idx >= cut[:, None]), (idx + 1).clamp(max=L - 1), idx)
    A = torch.gather(A, 1, src).reshape(-1).contiguous()
    offA = torch.arange(0, (n + 1) * L, L, dtype=torch.int64, device=dev)
    sc = _scoring(al, "-ACGT", al[2].NUC_4, gap)
    score = torch.zeros(n, dtype=torch.int64, device=dev)
    ea, eb, er = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    work = torch.empty(align.sw_workspace_bytes(sc, n, L, LB), dtype=torch.uint8, device=dev)
    align.sw_batch_dev(sc, A, offA, L, B, None, LB, score, ea, eb, er, work)
    stride = align.sw_traceback_stride(sc, L, LB)
    tbw = torch.empty(min(align.sw_traceback_workspace_bytes(sc, n, L, LB), 3 << 30), dtype=torch.uint8, device=dev)

    def run(score_t, wide):
        if wide:
            monkeypatch.setenv("POLYHIP_TB_WIDE", "1")
        else:
            monkeypatch.delenv("POLYHIP_TB_WIDE", raising=False)
        a = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        b = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        ln = torch.zeros(n, dtype=torch.int32, device=dev)
        align.sw_traceback_dev(sc, A, offA, L, B, None, LB, ea, eb, er, a, b, ln, tbw, score_t=score_t)
        torch.cuda.synchronize()
        return a, b, ln, align.sw_traceback_last_path()

    a1, b1, l1, path1 = run(score, False)
    a2, b2, l2, path2 = run(None, False)
    a3, b3, l3, path3 = run(score, True)
    # 153..256 rows: two lanes per pair on packed halves (5); the 32-bit form of the fixture: one wave per pair (4)
    assert (path1, path2, path3) == ((1, 2, 1) if L <= 152 else (5, 2, 5) if tb_cell == "half" else (4, 2, 4))
    if L > 152 and tb_cell == "half":  # ... and the one-wave-per-pair kernel on the same input, every pair
        monkeypatch.setenv("POLYHIP_TB_HALF2", "0")
        a4, b4, l4, path4 = run(score, False)
        monkeypatch.delenv("POLYHIP_TB_HALF2", raising=False)
        assert path4 == 4 and torch.equal(l1, l4) and torch.equal(a1, a4) and torch.equal(b1, b4)
    assert int(score.min()) < (100 if gap == -7 else 400) * L // 150 and int(score.max()) == 5 * L
    for a, b, ln in ((a2, b2, l2), (a3, b3, l3)):
        assert torch.equal(l1, ln) and torch.equal(a1, a) and torch.equal(b1, b)
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    A_h, a_h, b_h, l_h, s_h = A.cpu().numpy().reshape(n, L), a1.cpu().numpy(), b1.cpu().numpy(), l1.cpu().numpy(), score.cpu().numpy()
    refb = ref.tobytes()
    for p in range(0, n, 997):
        s, sa, sb, _, _ = orc.smith_waterman(A_h[p].tobytes(), refb, om, gap)
        sa = sa if isinstance(sa, bytes) else sa.encode()
        sb = sb if isinstance(sb, bytes) else sb.encode()
        assert int(s_h[p]) == s
        assert a_h[p, stride - l_h[p]:].tobytes() == sa and b_h[p, stride - l_h[p]:].tobytes() == sb, p


@pytest.mark.parametrize("maxA,LB,shared", [(300, 900, True), (700, 1500, True), (512, 600, False), (1024, 1100, False), (1200, 1300, False),
                                            (2600, 700, True), (4096, 300, False)])
def test_long_reads_wave_kernels(al, monkeypatch, maxA, LB, shared):
    """reads longer than the 256 rows a lane holds (257..4096): the one-wave-per-pair score kernel (path 6) and
    traceback kernel (path 4) against the generic kernels (POLYHIP_SW_WAVE=0 / POLYHIP_TB_WAVE=0) AND the oracle on every
    pair; shared and per-pair B, ragged lengths."""
    align = al[0]
    rng = np.random.default_rng(maxA)
    n = 48
    ref = orc.synth_dna(0xC4, LB).tobytes()
    reads, refs = [], []
    for p in range(n):
        L = int(rng.integers(maxA // 2, maxA + 1)) if p else maxA
        if shared:
            src = (ref * (L // LB + 2))
            at = int(rng.integers(0, LB))
            reads.append(_mutate(rng, src[at:at + L], sub=0.08, indel=0.02)[:maxA])
            refs.append(ref)
        else:
            b = bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, LB + 1))).astype(np.uint8))
            reads.append(_mutate(rng, (b * (L // len(b) + 2))[:L], sub=0.1, indel=0.03)[:maxA])
            refs.append(b)
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    A, offA = _pack(reads)
    if shared:
        B, offB = _pack([ref])[0], None
    else:
        B, offB = _pack(refs)
    got = align.sw_align_packed(sc, A, offA, B, offB)
    # (up to 1024 rows the traceback kernel sweeps on a byte profile of the pair in LDS: path 7; POLYHIP_TB_WAVE8=0: its
    # table form, path 4 -- every pair equal)
    assert (align.last_path(), align.sw_traceback_last_path()) == (6, 7 if maxA <= 1024 else 4)
    if maxA <= 1024:
        monkeypatch.setenv("POLYHIP_TB_WAVE8", "0")
        tab = align.sw_align_packed(sc, A, offA, B, offB)
        monkeypatch.delenv("POLYHIP_TB_WAVE8", raising=False)
        assert (align.last_path(), align.sw_traceback_last_path()) == (6, 4)
        for g, w in zip(got[:4], tab[:4]):
            assert (np.asarray(g) == np.asarray(w)).all()
        assert got[4] == tab[4] and got[5] == tab[5]
    monkeypatch.setenv("POLYHIP_SW_WAVE", "0")
    monkeypatch.setenv("POLYHIP_TB_WAVE", "0")
    base = align.sw_align_packed(sc, A, offA, B, offB)
    assert (align.last_path(), align.sw_traceback_last_path()) == (2, 3)
    for g, w in zip(got[:4], base[:4]):
        assert (np.asarray(g) == np.asarray(w)).all()
    assert got[4] == base[4] and got[5] == base[5]
    # EVERY pair against the oracle (round-5 verdict: 6 of 48 were), on all host cores
    for p, (s, sa, sb, ea, eb) in enumerate(_oracle_sw_threaded(list(zip(reads, refs)), om, -2)):
        assert (int(got[0][p]), int(got[1][p]), int(got[2][p])) == (s, ea, eb) and got[4][p] == sa and got[5][p] == sb, p


@pytest.mark.parametrize("hi,lo,gap,path", [(118, -100, -9, 7), (119, -100, -9, 4), (40, -137, -9, 7), (40, -138, -9, 4), (9, -9, -118, 7), (9, -9, -119, 4)])
def test_long_reads_byte_profile_limits(al, monkeypatch, hi, lo, gap, path):
    """the byte-profile sweep of the one-wave-per-pair traceback (path 7) keeps score - gap in a byte: matrices at both ends
    of that range take it, one step beyond they take the table form (path 4); every pair equal to the generic kernel, a
    sample equal to the oracle.  Six symbols, ragged lengths around 16 rows per lane, shared and per-pair B in one go."""
    align = al[0]
    rng = np.random.default_rng(hi * 1000 - lo)
    syms = "ACGTNU"
    mat = rng.integers(lo, hi + 1, (6, 6))
    mat[0, 0], mat[1, 2] = hi, lo
    mat[np.arange(6), np.arange(6)] = np.maximum(mat[np.arange(6), np.arange(6)], 1)
    scores = [[int(v) for v in row] for row in mat]
    sc = _scoring(al, syms, scores, gap)
    om = orc.SubstitutionMatrix(syms, syms, scores)
    n, maxA = 40, 600
    symb = np.frombuffer(syms.encode(), np.uint8)
    refs = [symb[rng.integers(0, 6, int(rng.integers(200, 900)))].tobytes() for _ in range(n)]
    reads = []
    for p in range(n):
        L = int(rng.integers(257, maxA + 1)) if p else maxA
        src = refs[p] * (L // len(refs[p]) + 2)
        at = int(rng.integers(0, len(refs[p])))
        r = bytearray(src[at:at + L])
        for q in rng.integers(0, L, L // 12):
            r[q] = int(symb[rng.integers(0, 6)])
        reads.append(bytes(r))
    A, offA = _pack(reads)
    for shared in (True, False):
        B, offB = (_pack([refs[0]])[0], None) if shared else _pack(refs)
        got = align.sw_align_packed(sc, A, offA, B, offB)
        assert align.sw_traceback_last_path() == path
        monkeypatch.setenv("POLYHIP_SW_WAVE", "0")
        monkeypatch.setenv("POLYHIP_TB_WAVE", "0")
        base = align.sw_align_packed(sc, A, offA, B, offB)
        assert align.sw_traceback_last_path() == 3
        monkeypatch.delenv("POLYHIP_SW_WAVE", raising=False)
        monkeypatch.delenv("POLYHIP_TB_WAVE", raising=False)
        for g, w in zip(got[:4], base[:4]):
            assert (np.asarray(g) == np.asarray(w)).all()
        assert got[4] == base[4] and got[5] == base[5]
        want = _oracle_sw_threaded([(reads[p], refs[0] if shared else refs[p]) for p in range(n)], om, gap)
        for p, (s_, sa, sb, ea, eb) in enumerate(want):  # every pair
            assert (int(got[0][p]), int(got[1][p]), int(got[2][p])) == (s_, ea, eb) and got[4][p] == sa and got[5][p] == sb, p


def test_long_reads_host_flavour_one_call(al, monkeypatch):
    """polyhip_sw_align_batch / _packed (host pointers: what cgo calls) on a batch of long reads that takes the packed multi-lane
    score pass (7) and the byte-profile one-wave-per-pair traceback (7) with the end cells left to it: every output equal to
    POLYHIP_SW_FUSE=0 (locate in the score pass), both string layouts equal, a sample equal to the oracle"""
    align = al[0]
    rng = np.random.default_rng(77)
    LB, n = 3000, 16_000
    ref = orc.synth_dna(0xC4, LB).tobytes()
    reads = []
    for p in range(n):
        L = int(rng.integers(300, 601)) if p else 600
        at = int(rng.integers(0, LB - L + 1))
        r = bytearray(ref[at:at + L])
        for q in rng.integers(0, L, L // 15):
            r[q] = b"ACGT"[int(rng.integers(0, 4))]
        if p % 7 == 3:
            del r[int(rng.integers(1, L - 1))]
        reads.append(bytes(r))
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    A, offA = _pack(reads)
    B = np.frombuffer(ref, np.uint8).copy()
    got = align.sw_align_packed(sc, A, offA, B, None)
    assert (align.last_path(), align.sw_traceback_last_path()) == (7, 7)
    packed = align.sw_align_strings_packed(sc, A, offA, B, None)
    monkeypatch.setenv("POLYHIP_SW_FUSE", "0")
    two = align.sw_align_packed(sc, A, offA, B, None)
    monkeypatch.delenv("POLYHIP_SW_FUSE", raising=False)
    assert (align.last_path(), align.sw_traceback_last_path()) == (7, 7)
    for other in (packed, two):
        for g, w in zip(got[:4], other[:4]):
            assert (np.asarray(g) == np.asarray(w)).all()
        assert got[4] == other[4] and got[5] == other[5]
    assert int(got[0].min()) > 0 and int(got[0].max()) <= 5 * 600 and int((got[3] != 0).sum()) == 0
    sample = list(range(0, n, 20))  # 800 of the 16,000 (round-5 verdict: 20 were)
    for p, (s_, sa, sb, ea, eb) in zip(sample, _oracle_sw_threaded([(reads[p], ref) for p in sample], om, -2)):
        assert (int(got[0][p]), int(got[1][p]), int(got[2][p])) == (s_, ea, eb) and got[4][p] == sa and got[5][p] == sb, p


def test_long_reads_chunked_workspace(al):
    """the one-wave-per-pair traceback with a workspace that holds a third of the batch: the entry point loops over
    chunks of pairs; same strings as with the full workspace, a sample equal to the oracle"""
    import torch
    align = al[0]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(4)
    LB, n = 1500, 700
    ref = orc.synth_dna(0xC4, LB).tobytes()
    reads = []
    for _ in range(n):
        L = int(rng.integers(300, 701))
        at = int(rng.integers(0, LB - L))
        reads.append(_mutate(rng, ref[at:at + L], sub=0.06, indel=0.02)[:700])
    maxA = max(len(r) for r in reads)
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    A_h, offA_h = _pack(reads)
    A = torch.from_numpy(A_h).to(dev)
    offA = torch.from_numpy(offA_h.view(np.int64)).to(dev)
    B = torch.from_numpy(np.frombuffer(ref, np.uint8).copy()).to(dev)
    score = torch.zeros(n, dtype=torch.int64, device=dev)
    ea, eb, er = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    work = torch.empty(align.sw_workspace_bytes(sc, n, maxA, LB), dtype=torch.uint8, device=dev)
    align.sw_batch_dev(sc, A, offA, maxA, B, None, LB, score, ea, eb, er, work)
    stride = align.sw_traceback_stride(sc, maxA, LB)
    full = align.sw_traceback_workspace_bytes(sc, n, maxA, LB)
    outs = []
    for nbytes in (full, full // 3 + 4096):
        tbw = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        a = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        b = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        ln = torch.zeros(n, dtype=torch.int32, device=dev)
        align.sw_traceback_dev(sc, A, offA, maxA, B, None, LB, ea, eb, er, a, b, ln, tbw, score_t=score)
        torch.cuda.synchronize()
        assert align.sw_traceback_last_path() == 7
        outs.append((a, b, ln))
    for x, y in zip(outs[0], outs[1]):
        assert torch.equal(x, y)
    a_h, b_h, l_h = (t.cpu().numpy() for t in outs[1])
    s_h = score.cpu().numpy()
    for p, (s, sa, sb, _, _) in enumerate(_oracle_sw_threaded([(r, ref) for r in reads], om, -2)):  # every pair
        assert int(s_h[p]) == s and a_h[p, stride - l_h[p]:].tobytes() == sa and b_h[p, stride - l_h[p]:].tobytes() == sb, p


def test_config4_full_size_mutated_batch(al, monkeypatch, tb_cell):
    """BASELINE configs[3] on the contract's input: all 1,000,000 reads of poly_amd.workloads.config4_reads (windows
    of the 5 kb reference with 5 % substitutions AND 1 % indels, SURVEY 8d C4 -- the input bench.py times), device
    resident.  (a) the generator is the same function on the GPU as on the CPU; (b) 20,000 sampled pairs (incl. the first and the last) equal the
    oracle in score, endA, endB and both aligned strings; (c) the packed two-pairs-per-lane pass equals the exact
    32-bit kernel (POLYHIP_SW_PACKED=0) on every pair; (d) size-independent properties on all pairs: an aligned
    pair of strings has equal length, re-scores to the reported score, and stripping the gaps gives substrings of
    the read and of the reference that end at (endA, endB)."""
    import torch
    from poly_amd import workloads
    align = al[0]
    dev = torch.device("cuda:0")
    n, LA, LB = 1_000_000, 150, 5000
    B, A2 = workloads.config4_reads(n, LA, LB, device=dev)
    ref_h, reads_h = workloads.config4_reads(3000)
    assert (A2[:3000].cpu().numpy() == reads_h).all() and (B.cpu().numpy() == ref_h).all()
    assert (workloads.config4_reads(64, first=777_000)[1] == A2[777_000:777_064].cpu().numpy()).all()
    A = A2.reshape(-1).contiguous()
    offA = torch.arange(0, (n + 1) * LA, LA, dtype=torch.int64, device=dev)
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    outs = {}
    for packed in (True, False):
        if packed:
            monkeypatch.delenv("POLYHIP_SW_PACKED", raising=False)
        else:
            monkeypatch.setenv("POLYHIP_SW_PACKED", "0")
        score = torch.zeros(n, dtype=torch.int64, device=dev)
        ea, eb, er = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
        work = torch.empty(align.sw_workspace_bytes(sc, n, LA, LB, True), dtype=torch.uint8, device=dev)
        align.sw_batch_dev(sc, A, offA, LA, B, None, LB, score, ea, eb, er, work)
        torch.cuda.synchronize()
        assert align.last_path() == (3 if packed else 1)
        outs[packed] = (score, ea, eb, er)
    monkeypatch.delenv("POLYHIP_SW_PACKED", raising=False)
    for x, y in zip(outs[True], outs[False]):
        assert torch.equal(x, y)
    score, ea, eb, er = outs[True]
    assert int(er.abs().sum()) == 0
    stride = align.sw_traceback_stride(sc, LA, LB)
    tbw = torch.empty(align.sw_traceback_workspace_bytes(sc, n, LA, LB), dtype=torch.uint8, device=dev)
    alnA = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    alnB = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    ln = torch.zeros(n, dtype=torch.int32, device=dev)
    align.sw_traceback_dev(sc, A, offA, LA, B, None, LB, ea, eb, er, alnA, alnB, ln, tbw, score_t=score)
    torch.cuda.synchronize()
    assert align.sw_traceback_last_path() == 1 and align.sw_traceback_last_half() == (tb_cell == "half")
    # (a') the one-call device path, where the score pass leaves the end cell to the traceback kernel: same seven outputs
    f_score = torch.zeros(n, dtype=torch.int64, device=dev)
    f_ea, f_eb, f_er, f_ln = (torch.full((n,), 7, dtype=torch.int32, device=dev) for _ in range(4))
    f_alnA, f_alnB = torch.zeros_like(alnA), torch.zeros_like(alnB)
    work = torch.empty(align.sw_workspace_bytes(sc, n, LA, LB, True), dtype=torch.uint8, device=dev)
    align.sw_align_dev(sc, A, offA, LA, B, None, LB, f_score, f_ea, f_eb, f_er, f_alnA, f_alnB, f_ln, work, tbw)
    torch.cuda.synchronize()
    for x, y in ((f_score, score), (f_ea, ea), (f_eb, eb), (f_er, er), (f_ln, ln)):
        assert torch.equal(x, y)
    cols0 = torch.arange(stride, device=dev)[None, :]
    live0 = cols0 >= (stride - ln.long())[:, None]
    assert bool(((f_alnA == alnA) | ~live0).all()) and bool(((f_alnB == alnB) | ~live0).all())
    del f_alnA, f_alnB, live0, work
    # (b) the oracle on a sample spread over the whole batch
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    rng = np.random.default_rng(4)
    import concurrent.futures as cf
    import os
    ncpu = max(1, min(os.cpu_count() or 1, 64))
    nsample = 20_000 if ncpu >= 8 else 2_500   # 2.7 ms of oracle per pair: ~4 s on 16 cores (round-4 verdict: 2,500 was thin)
    sample = np.sort(np.concatenate([rng.choice(n - 2, nsample - 2, replace=False) + 1, [0, n - 1]]))
    idx = torch.from_numpy(sample).to(dev)
    h = {k: v[idx].cpu().numpy() for k, v in dict(score=score, ea=ea, eb=eb, ln=ln, A=A2, alnA=alnA, alnB=alnB).items()}
    refb = ref_h.tobytes()

    def one(j):
        ws, wa, wb, wea, web = orc.smith_waterman(h["A"][j].tobytes(), refb, om, -2)
        wa = wa if isinstance(wa, bytes) else wa.encode("latin-1")
        wb = wb if isinstance(wb, bytes) else wb.encode("latin-1")
        L = int(h["ln"][j])
        got = (int(h["score"][j]), int(h["ea"][j]), int(h["eb"][j]), h["alnA"][j, stride - L:].tobytes(), h["alnB"][j, stride - L:].tobytes())
        return None if got == (ws, wea, web, wa, wb) else f"pair {sample[j]}: got {got} want {(ws, wea, web, wa, wb)}"
    with cf.ThreadPoolExecutor(ncpu) as ex:
        bad = [b for b in ex.map(one, range(len(sample)), chunksize=64) if b]
    assert not bad, bad[0]
    # (d) on every pair, on the device: re-score the aligned strings
    cols = torch.arange(stride, device=dev)[None, :]
    live = cols >= (stride - ln.long())[:, None]
    gapA, gapB = (alnA == ord("-")) & live, (alnB == ord("-")) & live
    assert not bool((gapA & gapB).any())
    match = (alnA == alnB) & live & ~gapA
    mism = live & ~gapA & ~gapB & (alnA != alnB)
    rescored = 5 * match.sum(1) - 4 * mism.sum(1) - 2 * (gapA.sum(1) + gapB.sum(1))
    assert torch.equal(rescored, score)
    # the ungapped strings are the read's and the reference's bytes ending at (endA, endB)
    nA, nB = (live & ~gapA).sum(1), (live & ~gapB).sum(1)
    assert bool((nA <= ea).all()) and bool((nB <= eb).all())
    chk = idx  # byte-exact on the sample (a full gather of ragged substrings is not worth a kernel here)
    for j, p in enumerate(sample[:200]):
        L = int(h["ln"][j])
        sa = h["alnA"][j, stride - L:].tobytes().replace(b"-", b"")
        sb = h["alnB"][j, stride - L:].tobytes().replace(b"-", b"")
        e_a, e_b = int(h["ea"][j]), int(h["eb"][j])
        assert h["A"][j].tobytes()[e_a - len(sa):e_a] == sa and refb[e_b - len(sb):e_b] == sb
    del chk


@pytest.mark.parametrize("L", [150, 250, 600, 1000])
@pytest.mark.parametrize("kind", ["random", "repeats", "ragged_bad"])
def test_fused_align_equals_two_passes(al, monkeypatch, tb_cell, kind, L):
    """polyhip_sw_align_batch_dev (deferred end cell, found by the traceback kernel in its last block) against
    POLYHIP_SW_FUSE=0 (locate in the score pass, then the traceback) on 100k reads at 0..60 % mutations: a tandem-repeat
    reference (maxima in several blocks: the tie list), ragged lengths incl. empty reads, bad symbols; a sample vs the oracle"""
    import torch
    align = al[0]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng({"random": 1, "repeats": 2, "ragged_bad": 3}[kind])
    # L = 250: two lanes per pair in both passes (tb path 5; 32-bit fixture: 4); L = 600, 1000: the packed multi-lane pass (7)
    # and the one-wave-per-pair traceback on a byte profile of the pair (7), which finds the deferred end cell in its sweep
    LB, n = 4000, {150: 100_000, 250: 60_000, 600: 16_000, 1000: 9_000}[L]
    if L > 256 and tb_cell != "half":
        pytest.skip("the long-read paths do not depend on the fixture")
    ref = orc.synth_dna(0xC4, LB).copy()
    if kind == "repeats":
        ref = np.tile(ref[:250], 16)
        ref[rng.integers(0, LB, 10)] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 10)]
    lens = np.full(n, L) if kind != "ragged_bad" else rng.integers(0, L + 1, n)
    starts = rng.integers(0, LB - L, n)
    reads = ref[(starts[:, None] + np.arange(L)[None, :])]
    hit = rng.random((n, L)) < np.linspace(0, 0.6, n)[:, None]
    reads[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    if kind == "ragged_bad":
        bad = rng.choice(n, 300, replace=False)
        reads[bad, rng.integers(0, L, 300)] = ord("X")
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    flat = np.concatenate([reads[i, :lens[i]] for i in range(n)]) if kind == "ragged_bad" else reads.reshape(-1)
    A = torch.from_numpy(flat.copy()).to(dev)
    offA = torch.from_numpy(offs).to(dev)
    B = torch.from_numpy(ref.copy()).to(dev)
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    stride = align.sw_traceback_stride(sc, L, LB)
    outs = {}
    for fuse in (True, False):
        if fuse:
            monkeypatch.delenv("POLYHIP_SW_FUSE", raising=False)
        else:
            monkeypatch.setenv("POLYHIP_SW_FUSE", "0")
        score = torch.zeros(n, dtype=torch.int64, device=dev)
        ea, eb, er, ln = (torch.full((n,), 9, dtype=torch.int32, device=dev) for _ in range(4))
        alnA = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        alnB = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        work = torch.empty(align.sw_workspace_bytes(sc, n, L, LB, True), dtype=torch.uint8, device=dev)
        tbw = torch.empty(min(align.sw_traceback_workspace_bytes(sc, n, L, LB), 3 << 30), dtype=torch.uint8, device=dev)
        align.sw_align_dev(sc, A, offA, L, B, None, LB, score, ea, eb, er, alnA, alnB, ln, work, tbw)
        torch.cuda.synchronize()
        if L > 256:
            assert (align.last_path(), align.sw_traceback_last_path()) == (7, 7)
        else:
            assert align.last_path() == 3 and align.sw_traceback_last_path() == (1 if L == 150 else 5 if tb_cell == "half" else 4)
        outs[fuse] = (score, ea, eb, er, ln, alnA, alnB)
    monkeypatch.delenv("POLYHIP_SW_FUSE", raising=False)
    for x, y in zip(outs[True][:5], outs[False][:5]):
        assert torch.equal(x, y)
    ln = outs[True][4]
    live = torch.arange(stride, device=dev)[None, :] >= (stride - ln.long())[:, None]
    assert bool(((outs[True][5] == outs[False][5]) | ~live).all()) and bool(((outs[True][6] == outs[False][6]) | ~live).all())
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    refb = ref.tobytes()
    score, ea, eb, er, ln, alnA, alnB = (t.cpu().numpy() for t in outs[True])
    for p in rng.choice(n, 300 if L <= 256 else 60, replace=False):
        a = flat[offs[p]:offs[p + 1]].tobytes()
        try:
            ws, wa, wb, wea, web = orc.smith_waterman(a, refb, om, -2)
        except orc.AlphabetError:
            assert er[p] != 0 and ln[p] == 0
            continue
        Lp = int(ln[p])
        got = (int(score[p]), int(ea[p]), int(eb[p]), alnA[p, stride - Lp:].tobytes().decode(), alnB[p, stride - Lp:].tobytes().decode())
        assert got == (ws, wea, web, wa, wb), (p, got, (ws, wea, web, wa, wb))


@pytest.mark.parametrize("maxA,maxB", [(64, None), (152, None), (256, None), (64, 90), (152, 90)])
def test_read_batch_at_an_unaligned_address(al, tb_cell, maxA, maxB):
    """A at byte offset 1, 2 and 3 of a device tensor: the row-code fetch of the half-float kernels reads aligned dwords and
    funnels them by the batch's misalignment.  300 pairs (the second workgroup partly filled) of ragged lengths 0 .. maxA,
    the last read one symbol long (the funnelled loads of the last pairs run past the batch's end), against one 600-symbol
    reference (paths 1 and 5; the 32-bit fixture: 1 and 4) or every pair its own B of up to 90 symbols (path 6; 2): all
    outputs equal to the same call on the aligned copy, a sample equal to the oracle."""
    import torch
    align = al[0]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(maxA * 100 + (maxB or 0))
    n, LB = 300, 600
    ref = orc.synth_dna(0xA1, LB)
    la = rng.integers(0, maxA + 1, n)
    la[:8] = maxA
    la[-1] = 1
    As, Bs = [], []
    for p in range(n):
        lb = int(rng.integers(1, maxB + 1)) if maxB else LB
        o = int(rng.integers(0, LB - max(lb if maxB else 0, int(la[p])) + 1))
        b = ref[o:o + lb] if maxB else ref
        a = np.resize(ref[o:o + max(1, min(lb, int(la[p])))], int(la[p])).copy()
        hit = rng.random(len(a)) < (0.5 if p % 4 == 0 else 0.06)
        a[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        As.append(a.tobytes())
        Bs.append(b.tobytes())
    A, offA = _pack(As)
    sc = _scoring(al, "-ACGT", al[2].NUC_4, -2)
    oAt = torch.from_numpy(offA.astype(np.int64)).to(dev)
    if maxB:
        Bf, offB = _pack(Bs)
        Bt, oBt, lenB = torch.from_numpy(Bf).to(dev), torch.from_numpy(offB.astype(np.int64)).to(dev), maxB
    else:
        Bt, oBt, lenB = torch.from_numpy(ref.copy()).to(dev), None, LB
    stride = align.sw_traceback_stride(sc, maxA, lenB)
    work = torch.empty(align.sw_workspace_bytes(sc, n, maxA, lenB, maxB is None), dtype=torch.uint8, device=dev)
    tbw = torch.empty(align.sw_traceback_workspace_bytes(sc, n, maxA, lenB), dtype=torch.uint8, device=dev)
    want_path = (6 if tb_cell == "half" else 2) if maxB else 1 if maxA <= 152 else 5 if tb_cell == "half" else 4
    outs = []
    for mis in range(4):
        base = torch.zeros(len(A) + 8, dtype=torch.uint8, device=dev)
        At = base[mis:mis + len(A)]
        At.copy_(torch.from_numpy(A))
        assert At.data_ptr() % 4 == mis
        score = torch.zeros(n, dtype=torch.int64, device=dev)
        ea, eb, er, ln = (torch.full((n,), 9, dtype=torch.int32, device=dev) for _ in range(4))
        alnA = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        alnB = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
        align.sw_align_dev(sc, At, oAt, maxA, Bt, oBt, lenB, score, ea, eb, er, alnA, alnB, ln, work, tbw)
        torch.cuda.synchronize()
        assert align.sw_traceback_last_path() == want_path
        if want_path == 1:
            assert align.sw_traceback_last_half() == (tb_cell == "half")
        outs.append((score, ea, eb, er, ln, alnA, alnB))
    live = torch.arange(stride, device=dev)[None, :] >= (stride - outs[0][4].long())[:, None]
    for mis in (1, 2, 3):
        for x, y in zip(outs[0][:5], outs[mis][:5]):
            assert torch.equal(x, y), mis
        assert bool(((outs[0][5] == outs[mis][5]) | ~live).all()) and bool(((outs[0][6] == outs[mis][6]) | ~live).all()), mis
    om = orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)
    score, ea, eb, er, ln, alnA, alnB = (t.cpu().numpy() for t in outs[1])
    assert not er.any()
    for p in [0, 255, 256, n - 2, n - 1] + [int(x) for x in rng.choice(n - 2, 15, replace=False)]:
        ws, wa, wb, wea, web = orc.smith_waterman(As[p], Bs[p], om, -2)
        wa = wa if isinstance(wa, bytes) else wa.encode()
        wb = wb if isinstance(wb, bytes) else wb.encode()
        Lp = int(ln[p])
        got = (int(score[p]), int(ea[p]), int(eb[p]), alnA[p, stride - Lp:].tobytes(), alnB[p, stride - Lp:].tobytes())
        assert got == (ws, wea, web, wa, wb), (p, got, (ws, wea, web, wa, wb))
