"""polyhip_demux_reads and polyhip_demux_pairs without a GPU: the oracle (tests/demux_oracle.py) against answers written out by
hand for each rule of the definition, what the hand-built inputs (tests/demux_inputs.py) hold, the declarations, the argument
errors in their documented order (they are all decided before any device call), and the guarantee the definition gives for
barcodes that are far enough apart."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import demux_inputs as di  # noqa: E402
import demux_oracle as do  # noqa: E402

NONE = do.NONE
NO = (NONE, NONE, NONE, do.F_NO_BARCODE)
AMB = (NONE, NONE, NONE, do.F_AMBIGUOUS)


# ---------------------------------------------------------------- 1. the oracle against answers worked out by hand
def test_oracle_distance_by_hand():
    assert do.distance(b"ACGTAC", b"ACGT", 0) == (0, 0)
    assert do.distance(b"TACGT", b"ACGT", 0) == (4, 0) and do.distance(b"TACGT", b"ACGT", 1) == (0, 1)
    # no start fits: the read is shorter than the barcode, whatever the shift; exactly p fits at 0 only
    assert do.distance(b"ACG", b"ACGT", 3) is None and do.distance(b"", b"ACGT", 0) is None
    assert do.distance(b"ACGA", b"ACGT", 63) == (1, 0)
    # s + p <= m bounds the starts: GGACGT holds ACGT at 2, and a max_shift beyond the read changes nothing
    assert do.distance(b"GGACGT", b"ACGT", 1) == (4, 0) and do.distance(b"GGACGT", b"ACGT", 2) == (0, 2)
    assert do.distance(b"GGACGT", b"ACGT", 63) == (0, 2)
    # lower case matches; N, n and every other byte are mismatches
    assert do.distance(b"acgt", b"ACGT", 0) == (0, 0) and do.distance(b"acgn", b"ACGT", 0) == (1, 0)
    assert do.distance(b"NNNN", b"ACGT", 0) == (4, 0) and do.distance(b"AC-\xff", b"ACGT", 0) == (2, 0)
    # equal counts: the smallest start.  ACAC sits in ACACAC at 0 and 2; in TCACAC it has one mismatch at 0 and none at 2
    assert do.distance(b"ACACAC", b"ACAC", 2) == (0, 0) and do.distance(b"TCACAC", b"ACAC", 2) == (0, 2)
    assert do.distance(b"TCACTC", b"ACAC", 2) == (1, 0)                # 1 at 0, 4 at 1, 1 at 2


def test_oracle_choice_by_hand():
    s = di.ties()
    X, Y, Z = s.barcodes
    r = s.reads
    pick = lambda read, mm, g, bc=(X, Y, Z): do.choose(read, list(bc), 0, mm, g)      # noqa: E731
    # AAAACCCG: one mismatch to X (its last byte) and one to Y (byte 6), seven to Z
    assert pick(r[0], 2, 0) == (0, 0, 1, 0) and pick(r[0], 2, 1) == AMB and pick(r[0], 0, 0) == NO and pick(r[0], 0, 5) == NO
    # the tie goes to the lowest index, whichever barcode that is
    assert pick(r[0], 2, 0, (Y, X, Z)) == (0, 0, 1, 0) and pick(r[3], 2, 0, (Y, X, Z)) == (0, 0, 0, 0)
    # AAAACCCC: 0 to X, 2 to Y -- d2 exactly min_margin above the best is enough, one more is not
    assert pick(r[2], 2, 2) == (0, 0, 0, 0) and pick(r[2], 2, 3) == AMB and pick(r[2], 0, 2) == (0, 0, 0, 0)
    # AAAACCGG: 2 to X, 0 to Y: the later barcode wins on distance
    assert pick(r[3], 2, 2) == (1, 0, 0, 0) and pick(r[3], 2, 3) == AMB
    # AAAACCTT: 2 and 2;  TAAACCCC: 1 and 3;  TTTTGGGG: 8, 6 and 0
    assert pick(r[4], 2, 0) == (0, 0, 2, 0) and pick(r[4], 2, 1) == AMB and pick(r[4], 1, 0) == NO
    assert pick(r[5], 2, 2) == (0, 0, 1, 0) and pick(r[5], 2, 3) == AMB
    assert pick(r[6], 0, 6) == (2, 0, 0, 0) and pick(r[6], 0, 7) == AMB
    # one barcode: d2 is none, no margin makes it ambiguous; a second barcode that does not fit is none as well
    assert do.choose(b"GATTACAG", [b"GATTACAG"], 0, 0, 64) == (0, 0, 0, 0)
    assert do.choose(b"GATTACAT", [b"GATTACAG"], 0, 0, 64) == NO and do.choose(b"GATTACAT", [b"GATTACAG"], 0, 64, 64) == (0, 0, 1, 0)
    assert do.choose(b"ACGTA", [b"ACGT", b"ACGTAC"], 0, 0, 5) == (0, 0, 0, 0) and do.choose(b"ACG", [b"ACGT", b"ACGTAC"], 3, 64, 0) == NO
    # the start is the chosen barcode's own: TGCA at 1, although ACGT is no worse than 3 at 0
    assert do.choose(b"ATGCAGG", [b"ACGT", b"TGCA"], 1, 0, 1) == (1, 1, 0, 0)
    # max_mismatches 64: whatever fits is a hit
    assert do.choose(b"T" * 64, [b"A" * 64], 0, 64, 1) == (0, 0, 64, 0) and do.choose(b"T" * 64, [b"A" * 64], 0, 63, 1) == NO


def test_oracle_reads_by_hand():
    bc = [b"ACGTACGT", b"TTGGCCAA"]
    reads = [b"TTGGCCAA" + b"GATTAC", b"NNNNNNNNNNNN", b"ACGTACGT" + b"CC", b"GGTTGGCCAATCA", b"ACGTACGA" + b"GGG", b"acgtacgt"]
    quals = [b"I" * len(x) for x in reads]
    quals[4] = b"I" * 5                                                  # another length: err 1, whatever the read holds
    r = do.demux_reads(reads, bc, quals, max_shift=2, max_mismatches=1, min_margin=1, clip=1, clip_extra=3)
    assert r.barcode.tolist() == [1, NONE, 0, 1, NONE, 0] and r.bstart.tolist() == [0, NONE, 0, 2, NONE, 0]
    assert r.mism.tolist() == [0, NONE, 0, 0, NONE, 0] and r.flags.tolist() == [0, 1, 0, 0, 0, 0] and r.err.tolist() == [0, 0, 0, 0, 1, 0]
    assert r.sample.tolist() == r.barcode.tolist()
    # groups 1, 2, 0, 1, 2, 0: stable, the unassigned last
    assert r.order.tolist() == [2, 5, 0, 3, 1, 4] and r.sample_start.tolist() == [0, 2, 4, 6]
    # clip: 8 + 3 bytes; read 2 has only 10 (clip_extra beyond its end), read 3 loses 2 + 8 + 3 = all 13, the bad read is empty
    assert r.seqs.tobytes() == b"" + b"" + b"TAC" + b"" + b"NNNNNNNNNNNN" + b"" and r.offsets.tolist() == [0, 0, 0, 3, 3, 15, 15]
    assert r.quals.tobytes() == b"I" * 15
    assert r.info == dict(reads=6, assigned=4, exact=4, no_barcode=1, ambiguous=0, not_in_sheet=0, bad=1, bytes_in=68, bytes_out=15)
    # clip = 0: the batch permuted, but for the bad read
    r = do.demux_reads(reads, bc, quals, max_shift=2, clip=0, clip_extra=3)
    assert r.seqs.tobytes() == reads[2] + reads[5] + reads[0] + reads[3] + reads[1] and r.offsets.tolist() == [0, 10, 18, 32, 45, 57, 57]
    r = do.demux_reads(reads, bc, None, max_shift=0, max_mismatches=1, clip_extra=1)
    assert r.barcode.tolist() == [1, NONE, 0, NONE, 0, 0] and r.mism[4] == 1 and r.quals is None and r.info["exact"] == 3
    assert r.seqs.tobytes() == b"C" + b"GG" + b"" + b"ATTAC" + reads[1] + reads[3]


def test_oracle_pairs_by_hand():
    b1, b2 = [b"ACGTACGT", b"TTGGCCAA"], [b"GATC", b"CTAG", b"AAAA"]
    table = [0, NONE, 2,
             1, 3, NONE]
    reads1 = [b"ACGTACGT" + b"CC", b"TTGGCCAA" + b"GG", b"ACGTACGT" + b"TT", b"CCCCCCCCCC", b"TTGGCCAA" + b"AC", b"TTGGCCAA" + b"GT"]
    reads2 = [b"AAAA" + b"TGT", b"GATC" + b"TGT", b"CTAG" + b"TGT", b"GATC" + b"TGT", b"TTTT" + b"TGT", b"CTAG" + b"TGT"]
    q1, q2 = [b"F" * len(x) for x in reads1], [b"F" * len(x) for x in reads2]
    q2[5] = b"F"
    r = do.demux_pairs(reads1, reads2, b1, b2, table, 4, q1, q2, max_mismatches=0)
    assert r.sample.tolist() == [2, 1, NONE, NONE, NONE, NONE]
    assert r.barcode.tolist() == [0, 2, 1, 0, 0, 1, NONE, 0, 1, NONE, 1, NONE]
    assert r.flags.tolist() == [0, 0, 0, 0, 4, 4, 1, 0, 0, 1, 0, 0] and r.err.tolist() == [0] * 11 + [1]
    assert r.order.tolist() == [1, 0, 2, 3, 4, 5] and r.sample_start.tolist() == [0, 0, 1, 2, 2, 6]
    # only the assigned pairs are clipped: a hole, a mate without a barcode and a bad mate leave both mates whole (the bad one empty)
    assert r.seqs[0].tobytes() == b"GG" + b"CC" + reads1[2] + reads1[3] + reads1[4] + reads1[5]
    assert r.seqs[1].tobytes() == b"TGT" + b"TGT" + reads2[2] + reads2[3] + reads2[4] + b""
    assert r.quals[1].tobytes() == b"F" * (3 + 3 + 7 + 7 + 7)
    assert r.info == dict(reads=12, assigned=4, exact=9, no_barcode=2, ambiguous=0, not_in_sheet=2, bad=1, bytes_in=102, bytes_out=71)
    # nbarcodes2 == 0: mate 1 alone decides, mate 2 is not judged and not clipped
    r = do.demux_pairs(reads1, reads2, b1, (), None, None, q1, q2, max_mismatches=0)
    assert r.sample.tolist() == [0, 1, 0, NONE, 1, NONE] and r.barcode[1::2].tolist() == [NONE] * 6 and r.flags[1::2].tolist() == [0] * 6
    assert r.order.tolist() == [0, 2, 1, 4, 3, 5] and r.sample_start.tolist() == [0, 2, 4, 6] and r.nsamples == 2
    assert r.seqs[0].tobytes() == b"CC" + b"TT" + b"GG" + b"AC" + reads1[3] + reads1[5]
    assert r.seqs[1].tobytes() == reads2[0] + reads2[2] + reads2[1] + reads2[4] + reads2[3]


# ---------------------------------------------------------------- 2. what the hand-built inputs hold
def _run(s, mode):
    if hasattr(s, "reads1"):
        return do.demux_pairs(s.reads1, s.reads2, s.barcodes1, s.barcodes2, s.pair_sample, s.nsamples, s.quals1, s.quals2, **mode)
    return do.demux_reads(s.reads, s.barcodes, s.quals, **mode)


def _groups(r):
    return np.diff(r.sample_start.astype(np.int64)).tolist()


def test_inputs_hold_what_they_promise():
    names = [s.name for s in di.single_sets() + di.pair_sets()] + ["random_many"]
    assert len(names) == len(set(names))
    s = di.lengths()
    assert [len(x) for x in s.reads[:5]] == [0, 3, 7, 8, 8] and len(s.reads[8]) == 8 + 3
    r = _run(s, s.modes[0])
    assert r.bstart.tolist() == [NONE, NONE, NONE, 0, 0, 1, 2, 2, 3, 3, 0, NONE] and r.flags[:3].tolist() == [1, 1, 1]
    assert _run(s, s.modes[1]).bstart.tolist() == [NONE] * 3 + [0, 0] + [NONE] * 5 + [0, NONE]
    assert _run(s, s.modes[3]).bstart[11] == 4
    s = di.long_at_63()
    assert [len(b) for b in s.barcodes] == [64, 64] and len(s.reads[0]) == 127
    r = _run(s, s.modes[0])
    assert r.bstart.tolist() == [63, 63, 62, NONE, 63, 0, 63, NONE] and r.mism.tolist() == [0, 0, 0, NONE, 2, 0, 1, NONE]
    assert _run(s, s.modes[3]).bstart.tolist() == [NONE, NONE, 62, NONE, NONE, 0, NONE, NONE]
    assert _run(s, s.modes[2]).info["no_barcode"] == 0                                   # 64 mismatches allowed: whatever fits
    s = di.four_byte()
    assert {len(b) for b in s.barcodes} == {4}
    r = _run(s, s.modes[0])
    assert r.barcode.tolist() == [0, 1, 2, 3, 1, NONE, 0, NONE, NONE] and r.bstart[4] == 1
    assert _run(s, s.modes[1]).mism[7] == 1 and _run(s, s.modes[2]).info["ambiguous"] == 1
    s = di.mixed_lengths()
    assert tuple(len(b) for b in s.barcodes) == di.MIXED
    r = _run(s, s.modes[0])
    assert r.barcode.tolist() == [x for t in range(6) for x in (t, t, NONE) * 3] and r.bstart[:9].tolist() == [0, 0, NONE, 1, 1, NONE, 2, 2, NONE]
    s = di.case_and_n()
    assert [_run(s, m).info["assigned"] for m in s.modes] == [3, 7, 9]
    r = _run(s, s.modes[1])
    assert r.mism.tolist() == [0, 0, 1, 1, NONE, 1, 0, NONE, 1, NONE] and _run(s, s.modes[2]).bstart[7] == 1
    s = di.two_starts()
    r = _run(s, s.modes[0])
    # read 0: 0, 2 and 4 are equally good; read 1: one mismatch at 0, none at 2; read 2: one mismatch at 0, 2 and 4 alike
    assert r.bstart.tolist() == [0, 2, 0, 3, 1] and r.mism.tolist() == [0, 0, 1, 0, 0]
    assert _run(s, s.modes[2]).mism.tolist() == [0, 1, 1, NONE, 0]
    s = di.ties()
    got = [_run(s, m) for m in s.modes]
    assert [g.info["ambiguous"] for g in got] == [0, 3, 3, 6, 0] and got[0].barcode.tolist() == [0, 0, 0, 1, 0, 0, 2]
    assert got[2].barcode.tolist() == [NONE, NONE, 0, 1, NONE, 0, 2] and got[3].barcode.tolist() == [NONE] * 6 + [2]
    assert do.demux_reads(s.reads, s.swapped.barcodes, s.quals, **s.modes[0]).barcode.tolist() == [0, 0, 1, 0, 0, 1, 2]
    s = di.single_barcode()
    assert len(s.barcodes) == 1 and [_groups(_run(s, m)) for m in s.modes] == [[3, 2], [4, 1]]
    s = di.one_sample()
    assert _groups(_run(s, s.modes[0])) == [0, 0, 70, 0, 0, 0]
    s = di.all_unassigned()
    r = _run(s, s.modes[0])
    assert _groups(r) == [0, 0, 0, 71] and r.order.tolist() == list(range(71)) and r.info["no_barcode"] == 71
    s = di.empty_samples()
    assert _groups(_run(s, s.modes[0])) == [0, 12, 16, 0, 0, 12, 0, 0, 1]
    s = di.clip_edges()
    a, b, c, d = (_run(s, m) for m in s.modes)
    assert s.lead > 0 and np.diff(a.offsets.astype(np.int64))[:4].tolist() == [0, 1, 5, 0]         # sample 0: reads 0, 4, 8 of 8, 12, 16 bytes lose 11
    assert b.info["bytes_out"] == d.info["bytes_out"] == len(s.reads[13]) and c.info["bytes_out"] == c.info["bytes_in"]
    s = di.no_qual()
    assert s.quals is None and _run(s, s.modes[0]).quals is None and s.lead > 0
    s = di.errs()
    r = _run(s, s.modes[0])
    assert np.flatnonzero(r.err).tolist() == s.bad and r.info["bad"] == 4 and r.order.tolist()[-4:] == s.bad
    assert all(r.barcode[i] == NONE and r.flags[i] == 0 for i in s.bad) and _run(s, s.modes[1]).info["bytes_out"] == 120
    for nb in di.COUNTS:
        s = di.count(nb)
        assert len(s.barcodes) == nb == len(set(s.barcodes))
        r = _run(s, s.modes[0])
        assert {0, nb - 1} <= set(r.barcode.tolist()), nb
    s = di.pairs_one_set()
    r = _run(s, s.modes[0])
    assert s.barcodes2 == [] and r.barcode[1::2].tolist() == [NONE] * 16 and r.sample.tolist() == [0, 1, 2, 3, 4] * 2 + [0, 1, 2, 3, NONE, 0]
    assert _run(s, s.modes[2]).sample[15] == NONE
    s = di.pairs_holes()
    r = _run(s, s.modes[0])
    assert r.sample[:12].tolist() == s.pair_sample and r.info["not_in_sheet"] == 8 and r.info["bad"] == 1
    assert r.flags[24:].tolist() == [1, 0, 0, 1, 1, 0, 0, 1, 0, 0] and r.err[33] == 1 and r.sample[12:].tolist() == [NONE] * 5
    s = di.pairs_no_qual()
    assert s.quals1 is None and _run(s, s.modes[0]).sample.tolist() == [1, 0, 0, NONE, 1, 0, 0, NONE, 1]
    for k in di.TABLE_SAMPLES:
        s = di.pairs_table(k)
        r = _run(s, s.modes[0])
        assert s.nsamples == k and len(r.sample_start) == k + 2 and r.sample_start[k + 1] == 300
        assert r.sample[0] == {1: 0, 256: 271 % 256, 257: 271 % 257, 65536: 65535}[k]
        assert r.info["not_in_sheet"] == (0 if k == 65536 else 2 * int((r.sample == NONE).sum()))


def test_random_many_holds_what_it_promises():
    s = di.random_many()
    r = _run(s, s.modes[0])
    assert len(s.reads) == 20_000 and min(_groups(r)) > 1000 and r.info["ambiguous"] > 0 and r.info["no_barcode"] > 2000
    assert 0 < r.info["bytes_out"] < r.info["bytes_in"] and sorted(r.order.tolist()) == list(range(20_000))


# ---------------------------------------------------------------- 3. the declarations and the errors that need no device
def test_declarations():
    from poly_amd import _lib, demux
    assert len(_lib.SIGNATURES["polyhip_demux_reads"][1]) == 20 and len(_lib.SIGNATURES["polyhip_demux_pairs"][1]) == 31
    assert "polyhip_demux_last_info" in _lib.SIGNATURES
    assert C.sizeof(demux._CParams) == 24 and C.sizeof(demux._CInfo) == 72
    assert tuple(n for n, _ in demux._CInfo._fields_) == do.INFO_FIELDS
    assert tuple(n for n, _ in demux._CParams._fields_) == tuple(do.DEFAULTS) + ("nsamples",)
    header = open(os.path.join(ROOT, "include", "polyhip.h")).read()
    assert "uint64_t reads, assigned, exact, no_barcode, ambiguous, not_in_sheet, bad, bytes_in, bytes_out;" in header
    assert "#define POLYHIP_ABI_VERSION 1\n" in header
    for n in ("polyhip_demux_reads", "polyhip_demux_pairs", "polyhip_demux_last_info"):
        assert f"int {n}(" in header and "polyhip_stream_t" not in header.split(f"int {n}(")[1].split(";")[0]
        assert not n.endswith("_dev") and hasattr(_lib.lib(), n)
    assert (demux.FLAG_NO_BARCODE, demux.FLAG_AMBIGUOUS, demux.FLAG_NOT_IN_SHEET, demux.NONE) == \
        (do.F_NO_BARCODE, do.F_AMBIGUOUS, do.F_NOT_IN_SHEET, do.NONE)
    for f in (demux.demux_packed, demux.demux_pairs_packed, demux.demux_fastq, demux.last_info, demux.Demuxed.sample_batch,
              demux.Demuxed.unassigned):
        assert callable(f)
    p = demux.DemuxParams()
    assert {k: getattr(p, k) for k in do.DEFAULTS} == do.DEFAULTS


def test_argument_errors_without_gpu():
    """everything the header lists is decided before any device call, in the documented order: each case holds every later
    fault as well"""
    from poly_amd import _lib, demux
    L = _lib.lib()
    P = demux._CParams
    a32, out8 = np.zeros(4, np.uint32), np.zeros(64, np.uint8)
    up, down, o64 = np.array([0, 4, 8], np.uint64), np.array([0, 8, 4], np.uint64), np.zeros(8, np.uint64)
    huge = np.array([0, 1 << 24, (1 << 24) + 1], np.uint64)
    rd = np.frombuffer(b"ACGTACGT", np.uint8).copy()
    bc = np.frombuffer(b"ACGTACGTAcGTAC" + b"C" * 70, np.uint8).copy()
    good, short, long_, lower, two = (np.array(x, np.uint32) for x in ([0, 8], [0, 3], [14, 79], [8, 14], [0, 4, 8]))
    p = lambda x: None if x is None else x.ctypes.data      # noqa: E731
    X = (1 << 24) - 1
    ok = P(0, 1, 1, 1, 0, 1)

    def call(params, barcodes=bc, bcoff=good, nbc=1, reads=rd, off=up, qual=None, qoff=None, n=2, barcode=a32, out=out8, oq=None, ooff=o64,
             starts=o64):
        rc = L.polyhip_demux_reads(None if params is None else C.byref(params), p(barcodes), p(bcoff), nbc, p(reads), p(off), p(qual),
                                   p(qoff), n, p(barcode), a32.ctypes.data, a32.ctypes.data, a32.ctypes.data, a32.ctypes.data,
                                   a32.ctypes.data, a32.ctypes.data, p(starts), p(out), p(oq), p(ooff))
        return rc, L.polyhip_last_error()

    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    worst = dict(nbc=4097, bcoff=short, qoff=down, oq=out8, barcode=None, off=huge)       # every later fault at once
    cases = (
        (None, worst, INV, b"null params"),
        (P(64, 65, 0, 2, 1 << 24, 0), worst, INV, b"max_shift = 64"),
        (P(63, 65, 0, 2, 1 << 24, 0), worst, INV, b"max_mismatches = 65"),
        (P(63, 64, 0, 2, 1 << 24, 0), worst, INV, b"clip = 2"),
        (P(63, 64, 0, 1, 1 << 24, 0), worst, INV, b"clip_extra = 16777216"),
        (P(63, 64, 0, 1, X, 0), worst, INV, b"nsamples = 0"),
        (P(63, 64, 0, 1, X, 65537), worst, INV, b"nsamples = 65537"),
        (P(63, 64, 0, 1, X, 65536), worst, INV, b"4097 barcodes"),
        (P(63, 64, 0, 1, X, 5), dict(worst, nbc=0), INV, b"0 barcodes"),
        (P(63, 64, 0, 1, X, 5), dict(worst, nbc=1, barcodes=None), INV, b"null barcodes"),
        (P(63, 64, 0, 1, X, 5), dict(worst, nbc=1, bcoff=None), INV, b"null barcodes"),
        (P(63, 64, 0, 1, X, 5), dict(worst, nbc=1), INV, b"barcode 0 of set 1 has 3 bytes"),
        (P(63, 64, 0, 1, X, 5), dict(worst, nbc=1, bcoff=long_), INV, b"barcode 0 of set 1 has 65 bytes"),
        (P(63, 64, 0, 1, X, 5), dict(worst, nbc=1, bcoff=lower), INV, b"barcode 0 of set 1 has byte 0x63 at 1"),
        (P(63, 64, 0, 1, X, 5), dict(worst, nbc=2, bcoff=np.array([0, 8, 14], np.uint32)), INV, b"barcode 1 of set 1 has byte 0x63 at 1"),
        (P(63, 64, 0, 1, X, 5), dict(worst, nbc=1, bcoff=good), INV, b"nsamples = 5"),
        (P(63, 64, 0, 1, X, 1), dict(worst, nbc=2, bcoff=two), INV, b"nsamples = 1"),
        (ok, dict(worst, nbc=1, bcoff=good), INV, b"come together"),
        (ok, dict(worst, bcoff=good, nbc=1, qual=rd, qoff=None), INV, b"come together"),
        (ok, dict(worst, bcoff=good, nbc=1, qual=rd, oq=None), INV, b"come together"),
        (ok, dict(worst, bcoff=good, nbc=1, qoff=None), INV, b"come together"),
        (ok, dict(worst, bcoff=good, nbc=1, qoff=None, oq=None), INV, b"null argument"),
        (ok, dict(starts=None, off=huge), INV, b"null argument"),
        (ok, dict(out=None, off=huge), INV, b"null argument"),
        (ok, dict(ooff=None, off=huge), INV, b"null argument"),
        (ok, dict(reads=None, off=huge), INV, b"null argument"),
        (ok, dict(off=None), INV, b"null argument"),
        (ok, dict(n=0, out=None, reads=None, off=None), INV, b"null argument"),
        (ok, dict(off=down), INV, b"not ascending"),
        (ok, dict(qual=rd, qoff=down, oq=out8, off=huge), INV, b"not ascending"),
        (ok, dict(off=huge), UNS, b"read 0 has 16777216 bytes"),
    )
    for params, kw, status, word in cases:
        rc, msg = call(params, **kw)
        assert rc == status and word in msg and b"polyhip_demux_reads" in msg, (kw, rc, msg)
    # the empty batch needs no device and no inputs: out_off[0] = 0, every sample_start 0, the info that of an empty call
    o64[:] = 7
    assert call(ok, n=0, reads=None, off=None)[0] == _lib.OK and o64.tolist() == [0, 0, 0, 7, 7, 7, 7, 7]
    assert demux.last_info() == dict.fromkeys(do.INFO_FIELDS, 0)
    assert L.polyhip_demux_last_info(None) == INV
    r = demux.demux_packed(np.zeros(0, np.uint8), [0], ["ACGT", "TTTT"])
    assert len(r.seqs) == 0 and r.offsets.tolist() == [0] and r.quals is None and len(r.sample) == 0 and r.sample_start.tolist() == [0] * 4
    assert [len(x[1]) for x in (r.sample_batch(0), r.sample_batch(1), r.unassigned())] == [1, 1, 1]
    with pytest.raises(IndexError):
        r.sample_batch(2)

    # the pairs call shares the checks; what it adds: the second set, the table, qualities of one mate only, its own name
    tab = np.array([0, 1, 9, NONE], np.uint32)

    def pairs(params, nb1=2, nb2=2, bcoff2=two, table=tab, q1=None, qo1=None, q2=None, qo2=None, oq1=None, oq2=None, off2=up, n=2):
        rc = L.polyhip_demux_pairs(C.byref(params), p(bc), p(two), nb1, p(bc), p(bcoff2), nb2, p(table), p(rd), p(up), p(q1), p(qo1),
                                   p(rd), p(off2), p(q2), p(qo2), n, p(a32), p(a32), p(a32), p(a32), p(a32), p(a32), p(a32), p(o64),
                                   p(out8), p(oq1), p(o64), p(out8), p(oq2), p(o64))
        return rc, L.polyhip_last_error()

    ten = P(0, 1, 1, 1, 0, 10)
    for params, kw, status, word in (
            (ten, dict(nb2=4097, bcoff2=short, table=None, off2=huge), INV, b"4097 barcodes in set 2"),
            (ten, dict(nb2=1, bcoff2=short, table=None, off2=huge), INV, b"barcode 0 of set 2 has 3 bytes"),
            (ten, dict(nb2=0, off2=huge), INV, b"nsamples = 10"),
            (ten, dict(table=None, off2=huge), INV, b"null pair_sample"),
            (P(0, 1, 1, 1, 0, 9), dict(off2=huge, q1=rd), INV, b"pair_sample[2] = 9"),
            (ten, dict(q1=rd, qo1=up, oq1=out8, off2=huge), INV, b"qualities of one mate only"),
            (ten, dict(q1=rd, qo1=up, q2=rd, qo2=up, oq1=out8, off2=huge), INV, b"come together"),
            (ten, dict(off2=down), INV, b"not ascending"),
            (ten, dict(off2=huge), UNS, b"2^24")):
        rc, msg = pairs(params, **kw)
        assert rc == status and word in msg and b"polyhip_demux_pairs" in msg, (kw, rc, msg)
    o64[:] = 7
    assert pairs(P(0, 1, 1, 1, 0, 2), nb2=0, n=0)[0] == _lib.OK and o64.tolist() == [0, 0, 0, 0, 7, 7, 7, 7]
    with pytest.raises(_lib.PolyhipError) as ei:
        demux.demux_packed(rd, up, ["ACGN"])
    assert ei.value.status == INV and "barcode 0" in ei.value.message
    with pytest.raises(ValueError):
        demux.demux_packed(rd, up, ["ACGT"], quals=rd)
    with pytest.raises(ValueError):
        demux.demux_pairs_packed(rd, up, rd, [0, 8], ["ACGT"])
    with pytest.raises(ValueError):
        demux.demux_pairs_packed(rd, up, rd, up, ["ACGT"], ["ACGT"])


def test_kernels_use_no_scratch(tmp_path):
    """what the compiler made of demux.hip: its five kernels, none of which spills to scratch, none below 8 waves per SIMD; and
    it compiles without a warning"""
    import re
    import subprocess
    from poly_amd import build
    asm = str(tmp_path / "demux.s")
    flags = [f for f in build.CXXFLAGS if f != "-fPIC"]
    res = subprocess.run([build._hipcc()] + flags + ["--cuda-device-only", "-S", os.path.join(build.CSRC, "demux.hip"), "-o", asm],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "demux.hip" not in res.stderr and "read_batch.h" not in res.stderr, res.stderr[-2000:]
    seen = {}
    for block in re.split(r"\n\s+- \.", open(asm).read().split("amdhsa.kernels:", 1)[1]):
        name = re.search(r"\.name:\s+\S*?\d+(match|assign|starts|place|gather)_kernelE", block)
        if name:
            seen[name.group(1)] = {key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1)) for key in ("vgpr_count", "private_segment_fixed_size")}
    assert sorted(seen) == ["assign", "gather", "match", "place", "starts"], seen
    for kernel, m in seen.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_count"] <= 64, (kernel, m)


# ---------------------------------------------------------------- 4. what the definition guarantees
def test_separated_barcodes_always_reach_their_sample():
    """With max_shift = 0, barcodes pairwise at Hamming distance >= 3, max_mismatches = 1 and min_margin = 1, a read whose barcode
    has at most one substitution is at distance <= 1 from its own barcode and, by the triangle inequality, at >= 2 from every
    other: it is a hit, the margin is >= 1, and it goes to its own sample -- all of them, by construction.  Asserted on the
    pooled constructs of the end-to-end test (tests/demux_inputs.py::pooled)."""
    d = di.pooled()
    bc = d["barcodes"]
    assert di.POOL_PARAMS == dict(max_shift=0, max_mismatches=1, min_margin=1, clip=1, clip_extra=0)
    assert min(di.hamming(a, b) for i, a in enumerate(bc) for b in bc[:i]) >= 3 and len(d["reads"]) == 3 * di.POOL_PER_SAMPLE
    r = do.demux_reads(d["reads"], bc, None, **di.POOL_PARAMS)
    tagged = [i for i, k in enumerate(d["truth"]) if k != NONE]
    assert len(tagged) > 0.9 * len(d["reads"]) and sum(d["subst"]) > 40 and len(tagged) < len(d["reads"])
    assert all(r.sample[i] == d["truth"][i] and r.mism[i] == d["subst"][i] for i in tagged)
    # and none of the reads without a barcode slipped in: each sample holds exactly its own reads, in input order
    for k in range(3):
        lo, hi = int(r.sample_start[k]), int(r.sample_start[k + 1])
        assert r.order[lo:hi].tolist() == [i for i in tagged if d["truth"][i] == k]
