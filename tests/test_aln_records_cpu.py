"""polyhip_aln_records without a GPU: the oracle (tests/aln_records_oracle.py) against answers written out by hand, the round
trip q + CIGAR + MD -> text on every input and on the mapper oracles' datasets, what the hand-built inputs hold, sam.write's
lines on oracle records, and the declarations."""
import io
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import aln_records_inputs as ari  # noqa: E402
import aln_records_oracle as aro  # noqa: E402


def _cigar(values):
    return "".join(f"{v >> 4}{aro.OP_CHARS[v & 15]}" for v in values)


def _one(A, B, rs=0, re_=None, rl=None, eqx=False, score=100, second=40, mapped=True):
    used = sum(1 for x in A if x != 45)
    re_ = rs + used if re_ is None else re_
    return aro.one(mapped, len(A), A, B, rs, re_, re_ if rl is None else rl, score, second, eqx)


# ---------------------------------------------------------------- 1. the oracle against answers worked out by hand
WORKED = [
    # alnA (read), alnB (text), read_start, read_len, CIGAR, CIGAR with eqx, MD, NM
    (b"ACGT", b"ACGT", 0, 4, "4M", "4=", "4", 0),
    (b"ACGT", b"AGGT", 0, 4, "4M", "1=1X2=", "1G2", 1),
    (b"AACCA", b"AGTCA", 0, 5, "5M", "1=2X2=", "1G0T2", 2),                   # adjacent mismatches
    (b"AC--GT", b"ACTTGT", 0, 4, "2M2D2M", "2=2D2=", "2^TT2", 2),
    (b"ACGGT", b"AC--T", 0, 5, "2M2I1M", "2=2I1=", "3", 2),                    # an insertion leaves no trace in the MD
    (b"AC-GT", b"ACTCT", 0, 4, "2M1D2M", "2=1D1X1=", "2^T0C1", 2),            # a deletion, at once a mismatch
    (b"A-C-G", b"AT-TG", 0, 3, "1M1D1I1D1M", "1=1D1I1D1=", "1^T0^T1", 3),     # D I D: two deletions
    (b"ACG", b"ACG", 2, 9, "2S3M4S", "2S3=4S", "3", 0),
    (b"GAC-", b"-ACT", 0, 3, "1I2M1D", "1I2=1D", "2^T0", 2),                   # I first, D last
    (b"AAA", b"CCC", 0, 3, "3M", "3X", "0C0C0C0", 3),
    (b"-AC", b"TAC", 1, 3, "1S1D2M", "1S1D2=", "0^T2", 1),                     # D first, after a clip
    (b"AAAAAAAAAAC", b"AAAAAAAAAAG", 0, 11, "11M", "10=1X", "10G0", 1),        # two digits
    (b"acg", b"aCg", 0, 3, "3M", "1=1X1=", "1C1", 1),                          # raw bytes: no case folding
    (b"AC", b"A-", 0, 2, "1M1I", "1=1I", "1", 1),                              # I last
]


@pytest.mark.parametrize("k", range(len(WORKED)))
def test_oracle_worked_examples(k):
    A, B, rs, rl, cigar, cigar_eqx, md, nm = WORKED[k]
    for eqx, want in ((False, cigar), (True, cigar_eqx)):
        e = _one(A, B, rs, rl=rl, eqx=eqx)
        assert (e.err, e.live, _cigar(e.cigar), e.md, e.nm) == (0, True, want, md.encode(), nm)


def test_oracle_err_mapq_and_flags_by_hand():
    assert _one(b"AC-G", b"AC-G").err == 1
    assert _one(b"ACG", b"ACG", rs=3, re_=2, rl=9).err == 2 and _one(b"ACG", b"ACG", rs=0, re_=3, rl=2).err == 2
    assert _one(b"ACG", b"ACG", rs=0, re_=4, rl=9).err == 2 and _one(b"", b"", rs=2, re_=3, rl=9).err == 2
    assert _one(b"", b"", rs=2, re_=2, rl=9).err == 3
    assert _one(b"A-", b"A-", rs=0, re_=5, rl=9).err == 1                        # 1 comes before 2
    assert _one(b"A-", b"A-", mapped=False).err == 0 and not _one(b"A", b"A", mapped=False).live
    dead = _one(b"AC-G", b"AC-G")
    assert (dead.live, dead.cigar, dead.md, dead.nm, dead.mapq) == (False, [], b"", 0, 0)
    # more than 2^28 - 1 columns: only the offsets say so, the strings are not there to be read
    big = aro.records([1, 1], [50, 50], [0, 0], [0, 0], [4, 4], [4, 4], b"ACGT", b"ACGT", [0, 4, 4 + (1 << 28)])
    assert list(big.err) == [0, 4] and big.info["bad"] == 1 and big.info["mapped"] == 1 and list(big.cigar_off) == [0, 1, 1]
    assert aro.records([1], [50], [0], [0], [4], [4], b"", b"", [0, (1 << 28) - 1]).err[0] != 4
    for s, t, q in ((100, 40, 36), (90, 0, 60), (90, -5, 60), (90, 90, 0), (90, 120, 0), (1, 0, 60), (120, 119, 0), (120, 60, 30),
                    (0, 0, 0), (-3, -9, 0)):
        assert aro.mapq_of(s, t) == q
    # mates: (live forward proper, live reverse proper), (live, unmapped), (unmapped, live reverse)
    flags, live = [1 | 4, 1 | 2 | 4, 1 | 4, 0, 0, 1 | 2], [True, True, True, False, False, True]
    assert aro.sam_flags(flags, live, True) == [0x1 | 0x2 | 0x20 | 0x40, 0x1 | 0x2 | 0x10 | 0x80, 0x1 | 0x8 | 0x40, 0x1 | 0x4 | 0x80,
                                                0x1 | 0x4 | 0x20 | 0x40, 0x1 | 0x8 | 0x10 | 0x80]
    assert aro.sam_flags(flags, live, False) == [0, 0x10, 0, 0x4, 0x4, 0x10]


# ---------------------------------------------------------------- 2. the round trip, which knows nothing of column classes
def _round_trip(A, B, rs, re_, rl, text=None):
    """q, the CIGAR and the MD of a live entry give back the text's bytes, and the CIGAR consumes the whole read"""
    q = b"\x00" * rs + bytes(x for x in A if x != 45) + b"\x00" * (rl - re_)
    want = bytes(x for x in B if x != 45) if text is None else text
    for eqx in (False, True):
        e = aro.one(True, len(A), A, B, rs, re_, rl, 100, 40, eqx)
        assert e.live
        got, used = aro.rebuild_text(q, e.cigar, e.md)
        assert got == want and used == rl
        assert sum(v >> 4 for v in e.cigar if v & 15 in (2, 7, 8, 0)) == len(want)       # reference bases the CIGAR spans


def test_round_trip_on_every_input():
    n = 0
    for c in ari.cases() + ari.paired_batch() + ari.batch(257):
        if aro.one(bool(c.flags & 1), len(c.A), c.A, c.B, c.read_start, c.read_end, c.read_len, c.score, c.second, False).live:
            _round_trip(c.A, c.B, c.read_start, c.read_end, c.read_len)
            n += 1
    assert n > 250


def _mapper_hits():
    """the mapper oracles' answers on their datasets: (text, hit, read length) per entry"""
    import map_affine_inputs as mai
    import map_pairs_inputs as mpi
    d = mai.dataset()
    out = [(d["T"], h, len(r)) for h, r in zip(mai.expected(*mai.GAPS[0])[0], d["reads"])]
    p = mpi.dataset()
    hits, _ = mpi.flat(mpi.expected(*mpi.GAPS[0])[0])
    reads = [r for pair in zip(p["reads1"], p["reads2"]) for r in pair]
    return out + [(p["T"], h, len(r)) for h, r in zip(hits, reads)]


def test_round_trip_on_the_mapper_datasets():
    seen = dict(ins=0, dele=0, reverse=0, clipped=0)
    for T, h, m in _mapper_hits():
        if not h.flags & 1:
            continue
        _round_trip(h.alignA, h.alignB, h.read_start, h.read_end, m, T[h.ref_start:h.ref_end])
        seen["ins"] += b"-" in h.alignB
        seen["dele"] += b"-" in h.alignA
        seen["reverse"] += bool(h.flags & 2)
        seen["clipped"] += h.read_start > 0 or h.read_end < m
    assert all(v > 0 for v in seen.values()), seen


# ---------------------------------------------------------------- 3. what the hand-built inputs hold
def _class_runs(c):
    """[(class, first column, one past the last)] of the maximal runs, '=' and X apart"""
    out = []
    for j, (a, b) in enumerate(zip(c.A, c.B)):
        k = aro.column_class(a, b)
        if out and out[-1][0] == k:
            out[-1][2] = j + 1
        else:
            out.append([k, j, j + 1])
    return out


def test_inputs_hold_every_condition():
    cs = ari.cases()
    by = {c.name: c for c in cs}
    E = {c.name: aro.one(True, len(c.A), c.A, c.B, c.read_start, c.read_end, c.read_len, c.score, c.second, False) for c in cs}
    live = [c for c in cs if E[c.name].live]
    for c in cs:      # the class string is what the strings hold
        assert "".join(aro.column_class(a, b) for a, b in zip(c.A, c.B)) == c.classes and len(c.A) == len(c.B)
    assert {len(c.A) for c in live} >= set(ari.COLUMN_COUNTS) | {11264} and ari.LONGEST == 11264
    runs = {c.name: _class_runs(c) for c in live}
    for cl in "XID=":
        ends = {e for c in live for k, s, e in runs[c.name] if k == cl and e < len(c.A)}
        assert {63, 64, 65} <= ends, (cl, "a run ending one before, at and one after the 64-column boundary")
        assert any(k == cl and s // 64 + 2 <= (e - 1) // 64 for c in live for k, s, e in runs[c.name]), (cl, "a run over three steps")
    # MD counters of one, two, three and four digits, at both ends of each
    counters = {int(x) for c in live for x in re.findall(rb"\d+", E[c.name].md)}
    assert counters >= set(ari.MATCH_RUNS)
    mds = {c.name: E[c.name].md for c in live}
    assert re.search(rb"[A-Z]0[A-Z]", mds["adjacent_mismatches"]) and re.search(rb"\^[A-Z]+0[A-Z]\d", mds["d_then_x"])
    assert re.search(rb"\^[A-Z]0\^[A-Z]", mds["d_i_d"]) and by["d_i_d"].classes.count("DID") == 1
    first = {c.classes[0] for c in live}
    last = {c.classes[-1] for c in live}
    assert {"I", "D"} <= first and {"I", "D"} <= last
    assert any(set(c.classes) == {"X"} and len(c.A) > 64 for c in live)
    clips = {(c.read_start > 0, c.read_len > c.read_end) for c in live}
    assert clips == {(False, False), (True, False), (False, True), (True, True)}
    assert any(c.second == 0 for c in live) and any(c.second < 0 for c in live) and any(c.second == c.score for c in live)
    assert any(c.second > c.score for c in live) and any(c.score == 1 for c in live) and any(c.flags & 2 for c in live)
    assert {E[c.name].mapq for c in live} >= {0, 30, 36, 60}
    assert {E[c.name].err for c in cs} == {0, 1, 2, 3}
    assert by["err1_second_step"].classes.index("?") >= 64 and E["err1_before_err2"].err == 1 and E["err2_before_err3"].err == 2
    e2 = [c for c in cs if E[c.name].err == 2]
    assert any(c.read_start > c.read_end for c in e2) and any(c.read_end > c.read_len for c in e2)
    assert any(c.read_start <= c.read_end <= c.read_len and len(c.A) for c in e2)
    # batches: the sizes, unmapped entries between the others (zeros for the scans), some of them with columns never read
    assert ari.BATCH_SIZES == (1, 255, 256, 257)
    for n in ari.BATCH_SIZES:
        b = ari.batch(n)
        assert len(b) == n
        if n > 1:
            dead = [i for i, c in enumerate(b) if not c.flags & 1]
            assert len(dead) >= n // 4 and any(len(b[i].A) for i in dead) and 0 not in dead
            assert any(len(c.A) == ari.LONGEST for c in b) and {1, 2, 3} <= {E[c.name].err for c in b if c.name in E}
    # pairs: every combination of live / unmapped / err, strand and proper bit, per mate
    p = ari.paired_batch()
    state = lambda c: ("unmapped" if not c.flags & 1 else "err" if "?" in c.classes else "live", c.flags & 2, c.flags & 4)  # noqa: E731
    assert len({(state(p[i]), state(p[i + 1])) for i in range(0, len(p), 2)}) == 144 == len(p) // 2


# ---------------------------------------------------------------- 4. sam.write on oracle records
def _write(names, reads, quals, ref_start, score, tlen, rec, paired):
    from types import SimpleNamespace

    from poly_amd import sam
    fh = io.StringIO()
    result = SimpleNamespace(ref_start=np.array(ref_start, np.uint32), score=np.array(score, np.int64), tlen=np.array(tlen, np.int64))
    got = SimpleNamespace(sam_flag=rec.sam_flag, mapq=rec.mapq, nm=rec.nm, cigar_string=rec.cigar_string, md_string=rec.md_string)
    sam.write(fh, "chr", 5000, names, reads, quals, result, got, paired=paired)
    return fh.getvalue().split("\n")


def test_sam_write_lines():
    # pair 0: mate 1 forward at 100, mate 2 reverse at 300 (proper, tlen 350); pair 1: mate 1 unmapped, mate 2 live reverse with
    # a byte the complement table lacks; pair 2: both at 700 (a tie: mate 1 takes the plus sign); pair 3: neither mapped
    A = [b"ACGTA", b"TT-GC", b"", b"AC.TG", b"AAAA", b"CCCC", b"", b""]
    B = [b"ACCTA", b"TTAGC", b"", b"AC.TG", b"AAAA", b"CCCC", b"", b""]
    flags = [1 | 4, 1 | 2 | 4, 0, 1 | 2, 1, 1, 0, 0]
    rs, re_ = [1, 0, 0, 0, 0, 0, 0, 0], [6, 4, 0, 5, 4, 4, 0, 0]
    rl = [6, 6, 5, 5, 4, 4, 3, 3]
    off = np.concatenate([[0], np.cumsum([len(a) for a in A])])
    score, second = [21, 15, 0, 25, 20, 20, 0, 0], [0] * 8
    rec = aro.records(flags, score, second, rs, re_, rl, b"".join(A), b"".join(B), off, eqx=False, paired=True)
    assert [e.live for e in rec.entries] == [True, True, False, True, True, True, False, False]
    ref_start, tlen = [100, 300, 0, 500, 700, 700, 0, 0], [350, 0, -7, 0]
    names = ["p0", "p0", "p1", "p1", "p2", "p2", "p3", "p3"]
    reads = [b"GACGTA", b"GCAAGG", b"ACGTN", b"CA.GT", b"AAAA", b"GGGG", b"ACG", b"TTT"]       # as sequenced: mates 2 of pairs 0, 1 reverse
    quals = ["abcdef", "ghijkl", "mnopq", "rstuv", "wxyz", "0123", "456", "789"]
    lines = _write(names, reads, quals, ref_start, score, tlen, rec, True)
    assert lines[:2] == ["@HD\tVN:1.6\tSO:unsorted", "@SQ\tSN:chr\tLN:5000"] and lines[-1] == "" and len(lines) == 2 + 8 + 1
    assert lines[:-1] == aro.sam_lines("chr", 5000, names, reads, quals, ref_start, score, tlen, rec, True)
    f = [ln.split("\t") for ln in lines[2:-1]]
    assert [len(x) for x in f] == [14, 14, 11, 14, 14, 14, 11, 11]
    assert f[0] == ["p0", str(0x1 | 0x2 | 0x20 | 0x40), "chr", "101", "60", "1S5M", "=", "301", "350", "GACGTA", "abcdef", "NM:i:1",
                    "MD:Z:2C2", "AS:i:21"]
    assert f[1] == ["p0", str(0x1 | 0x2 | 0x10 | 0x80), "chr", "301", "60", "2M1D2M2S", "=", "101", "-350", "CCTTGC", "lkjihg", "NM:i:1",
                    "MD:Z:2^A2", "AS:i:15"]
    assert f[2] == ["p1", str(0x1 | 0x4 | 0x20 | 0x40), "chr", "501", "0", "*", "=", "501", "0", "ACGTN", "mnopq"]     # takes the mate's place
    assert f[3][:11] == ["p1", str(0x1 | 0x8 | 0x10 | 0x80), "chr", "501", "60", "5M", "*", "0", "0", "ACNTG", "vutsr"]
    assert (f[4][3], f[4][8], f[5][3], f[5][8]) == ("701", "-7", "701", "7")                  # tlen's own sign is kept: plus means +tlen
    assert f[6] == ["p3", str(0x1 | 0x4 | 0x8 | 0x40), "*", "0", "0", "*", "*", "0", "0", "ACG", "456"]
    # single-end, no qualities: no mate fields, '*' for QUAL
    rec1 = aro.records(flags[:4], score[:4], second[:4], rs[:4], re_[:4], rl[:4], b"".join(A[:4]), b"".join(B[:4]), off[:5])
    lines = _write(names[:4], reads[:4], None, ref_start[:4], score[:4], [], rec1, False)
    assert lines[:-1] == aro.sam_lines("chr", 5000, names[:4], reads[:4], None, ref_start[:4], score[:4], [], rec1, False)
    f = [ln.split("\t") for ln in lines[2:-1]]
    assert f[1][:11] == ["p0", "16", "chr", "301", "60", "2M1D2M2S", "*", "0", "0", "CCTTGC", "*"] and f[2][1:6] == ["4", "*", "0", "0", "*"]


# ---------------------------------------------------------------- 5. declarations
def test_declarations():
    from poly_amd import _lib, sam
    header = open(os.path.join(ROOT, "include", "polyhip.h")).read()
    for name in ("polyhip_aln_records", "polyhip_aln_records_last_info"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["polyhip_aln_records"][1]) == 21
    assert re.search(r"#define POLYHIP_ABI_VERSION\s+1\b", header)
    assert header.index("polyhip_map_pairs_last_info(polyhip_map_pairs_info") < header.index("polyhip_aln_records_params {")
    assert "not a calibrated quality" in header and "not a calibrated quality" in sam.__doc__
    go = open(os.path.join(ROOT, "go", "polyhip", "alnrecords.go")).read()
    assert "C.polyhip_aln_records(" in go and "func AlnRecords(" in go
    assert [n for n, _ in sam._CInfo._fields_] == ["entries", "mapped", "columns", "cigar_ops", "md_bytes", "bad"]
    from poly_amd import mapper
    assert "poly_amd.sam" in mapper.__doc__
