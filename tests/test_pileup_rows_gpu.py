"""polyhip_pileup_rows on the GPU against its CPU oracle (tests/pileup_rows_oracle.py): text, row_off, err, *ntext and the info
counters are compared exactly on the inputs of tests/pileup_rows_inputs.py (what they hold is asserted in
tests/test_pileup_rows_cpu.py), then the C call's own contract (argument errors in their order, the capacity rule, empty
calls, order that is no permutation, the same bytes twice), and end to end from a FASTQ image through the mapper, the
records, the duplicate marks and the coordinate order, on one text and on one contig of three."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_affine_inputs as mai  # noqa: E402
import pileup_inputs as pi  # noqa: E402
import pileup_qual_inputs as qi  # noqa: E402
import pileup_rows_inputs as ri  # noqa: E402
import pileup_rows_oracle as ro  # noqa: E402
from map_check import _params, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ARGS = ("flags", "mapq", "ref_start", "ref_end", "read_start", "alnA", "alnB", "aln_off", "qual", "qual_off")
SET_NAMES = ("shapes", "edges", "regions", "contention", "random", "bytes", "errs", "thresholds", "batch1", "batch255", "batch256", "batch257",
             "quality_errs", "crossing", "run_lengths", "digits", "depths", "tokens")
SETS = {s.name: s for s in ri.all_sets()}


@functools.lru_cache(maxsize=None)
def _want(name, k, with_qual):
    s = SETS[name]
    st = s.settings[k]
    p, kw = ri.arguments(s, st, with_qual)
    return ro.pileup_rows(*[p[f] for f in ARGS], s.qs.ref, st["name"], order=p["order"], **kw)


def _call(p, ref, name, **kw):
    from poly_amd import pileup
    return pileup.rows_packed(p["flags"], p["ref_start"], p["ref_end"], p["alnA"], p["alnB"], p["aln_off"], ref, name, p["mapq"], p["read_start"],
                              p["qual"], p["qual_off"], p.get("order"), **kw)


def _assert_same(got, want, what=""):
    from poly_amd import pileup
    assert got.status == 0 and got.ntext == len(want.text), (what, got.ntext, len(want.text))
    have = got.text.tobytes()
    if have != want.text:
        at = next(k for k in range(min(len(have), len(want.text))) if have[k] != want.text[k])
        row = have.rfind(b"\n", 0, at) + 1
        raise AssertionError(f"{what}: the text differs at byte {at}: got {have[row:at + 40]!r}, want {want.text[row:at + 40]!r}")
    assert got.row_off.dtype == np.uint64 and got.row_off.tolist() == want.row_off.tolist(), what
    assert got.err.dtype == np.uint32 and got.err.tolist() == want.err.tolist(), what
    assert pileup.last_rows_info() == want.info and got.nrows == want.info["rows"], (what, pileup.last_rows_info(), want.info)


# ---------------------------------------------------------------- 1. every set, every setting, with and without qualities
def test_set_names():
    assert tuple(s.name for s in ri.all_sets()) == SET_NAMES


@pytest.mark.parametrize("name", SET_NAMES)
def test_all_sets(name):
    s = SETS[name]
    for k, st in enumerate(s.settings):
        for with_qual in (True, False):
            p, kw = ri.arguments(s, st, with_qual)
            got = _call(p, s.qs.ref, st["name"], **kw)
            _assert_same(got, _want(name, k, with_qual), (name, k, with_qual))
            want = _want(name, k, with_qual)
            for pos in list(want.rows)[:50]:
                assert got.row(pos) == want.rows[pos]


def test_the_same_call_twice_gives_the_same_bytes():
    for name in ("depths", "random"):
        s = SETS[name]
        p, kw = ri.arguments(s, s.settings[1], True)
        one, two = _call(p, s.qs.ref, b"seq1", **kw), _call(p, s.qs.ref, b"seq1", **kw)
        assert one.text.tobytes() == two.text.tobytes() and (one.row_off == two.row_off).all() and one.ntext > 1000


# ---------------------------------------------------------------- 2. the C call itself
def _raw(s, st=None, n=None, text=None, cap=0, null=(), params=True, ref_len=None, p=None, n_claimed=None, name=b"seq1", name_len=None, order=None,
         with_qual=True, **fields):
    """polyhip_pileup_rows on a QualSet -> (status, message, outputs); `null`: arguments passed as NULL.  The outputs start out as
    0xAB bytes, so what the call leaves alone shows"""
    from poly_amd import _lib, pileup
    p = qi.pack(s) if p is None else p
    n = len(s.entries) if n is None else n
    st = dict(ri.DEFAULTS, **(st or {}))
    lo, hi = st["region"] or (0, len(s.ref))
    L = max(hi - lo, 0)
    out = dict(row_off=np.full(L + 1, 0xABABABABABABABAB, np.uint64), err=np.full(n, 0xABABABAB, np.uint32))
    nt = C.c_uint64(0xAB)
    ref, nm = np.frombuffer(s.ref, np.uint8), np.frombuffer(name, np.uint8)
    ptr = lambda k, a: None if k in null or a is None else a.ctypes.data    # noqa: E731
    q = with_qual
    cp = pileup._CRowsParams(lo, hi, st["pos_origin"], st["min_mapq"], st["qual_offset"], st["all_positions"], 0)
    for f, v in fields.items():
        setattr(cp, f, v)
    rc = _lib.lib().polyhip_pileup_rows(C.byref(cp) if params else None, n if n_claimed is None else n_claimed, ptr("flags", p["flags"]),
                                        ptr("mapq", p["mapq"]), ptr("ref_start", p["ref_start"]), ptr("ref_end", p["ref_end"]),
                                        ptr("read_start", p["read_start"] if q else None), ptr("alnA", p["alnA"]), ptr("alnB", p["alnB"]),
                                        ptr("aln_off", p["aln_off"]), ptr("qual", p["qual"] if q else None),
                                        ptr("qual_off", p["qual_off"] if q else None), ptr("ref", ref), len(s.ref) if ref_len is None else ref_len,
                                        ptr("order", order), ptr("name", nm), len(name) if name_len is None else name_len,
                                        None if "ntext" in null else C.byref(nt), ptr("text", text), cap, ptr("row_off", out["row_off"]),
                                        ptr("err", out["err"]))
    out["ntext"] = int(nt.value)
    return rc, _lib.lib().polyhip_last_error().decode(), out


def test_capacity_size_only_short_and_exact():
    from poly_amd import _lib, pileup
    s, want = SETS["shapes"].qs, _want("shapes", 0, True)
    nt = len(want.text)
    assert nt > 10000
    rc, msg, out = _raw(s)                                                        # NULL and no capacity: the size
    assert rc == _lib.ERR_INVALID and f"the text needs {nt} bytes" in msg and "holds 0" in msg and "polyhip_pileup_rows" in msg
    assert out["ntext"] == nt and out["row_off"].tolist() == want.row_off.tolist() and out["err"].tolist() == want.err.tolist()
    assert pileup.last_rows_info() == want.info
    text = np.full(nt + 8, 0xAB, np.uint8)
    rc, msg, out = _raw(s, text=text, cap=nt - 1)                                 # short by one byte: nothing is written
    assert rc == _lib.ERR_INVALID and f"the text needs {nt} bytes" in msg and f"holds {nt - 1}" in msg
    assert (text == 0xAB).all() and out["ntext"] == nt and out["row_off"].tolist() == want.row_off.tolist() and out["err"].tolist() == want.err.tolist()
    rc, _, out = _raw(s, text=text, cap=nt)                                       # exactly what was asked for, and not a byte beyond
    assert rc == _lib.OK and text[:nt].tobytes() == want.text and (text[nt:] == 0xAB).all() and out["ntext"] == nt
    rc, _, out = _raw(s, text=text, cap=nt, null=("row_off",))                    # row_off is optional
    assert rc == _lib.OK and text[:nt].tobytes() == want.text
    p, kw = ri.arguments(SETS["shapes"], SETS["shapes"].settings[0], True)
    short = _call(p, s.ref, b"seq1", text_capacity=nt - 1, **kw)                  # the wrapper with a capacity the caller fixed
    assert short.status == _lib.ERR_INVALID and short.text is None and short.ntext == nt and short.row_off.tolist() == want.row_off.tolist()
    _assert_same(_call(p, s.ref, b"seq1", text_capacity=nt, **kw), want)


def test_the_wrappers_guess_runs_again():
    """many short reads under a long name: the text outgrows the guess and the call is made a second time with the exact size"""
    s = SETS["depths"]
    k = len(s.settings) - 1
    p, kw = ri.arguments(s, s.settings[k], True)
    name = b"n" * 200
    p2, _ = ri.arguments(s, s.settings[k], True)
    want = ro.pileup_rows(*[p2[f] for f in ARGS], s.qs.ref, name, order=p2["order"], **kw)
    nbytes = int(p["aln_off"][-1])
    assert len(want.text) > 2 * nbytes + len(s.qs.ref) * (len(name) + 16) + 1024
    _assert_same(_call(p, s.qs.ref, name, **kw), want)


def test_empty_batch_empty_region_and_no_tokens():
    from poly_amd import _lib, pileup
    s = SETS["edges"].qs
    none = qi.pack(qi.QualSet("none", (), (), (), s.ref, ()))
    zero = dict(entries=0, used=0, skipped_mapq=0, bad=0, columns=0, tokens=0, rows=0, text_bytes=0, dropped_events=0, max_row_bytes=0)
    rc, _, out = _raw(s, n=0, p=none, null=ARGS + ("err",))                       # n == 0: no row without all_positions
    assert rc == _lib.OK and out["ntext"] == 0 and (out["row_off"] == 0).all() and pileup.last_rows_info() == zero
    got = _call(dict(none, order=None), s.ref, b"seq1", all_positions=True)       # ... and one per position with it
    want = ro.pileup_rows(*[none[f] for f in ARGS], s.ref, b"seq1", all_positions=1)
    _assert_same(got, want)
    assert got.nrows == len(s.ref) and got.text.tobytes().count(b"\t0\t*\t*\n") == len(s.ref)
    e = SETS["quality_errs"].qs
    p = qi.pack(e)
    want = ro.pileup_rows(*[p[f] for f in ARGS], e.ref, b"seq1", region=(7, 7))
    rc, _, out = _raw(e, dict(region=(7, 7)))                                     # L == 0: err, one offset and *ntext = 0
    assert rc == _lib.OK and out["ntext"] == 0 and out["row_off"].tolist() == [0] and out["err"].tolist() == want.err.tolist()
    assert pileup.last_rows_info() == want.info and want.info["used"] > 0 and want.info["tokens"] == 0
    want = ro.pileup_rows(*[p[f] for f in ARGS], e.ref, b"seq1", region=(0, 5))   # entries, a region, and no token in it
    assert want.info["tokens"] == 0 and want.info["used"] > 0
    rc, _, out = _raw(e, dict(region=(0, 5)))
    assert rc == _lib.OK and out["ntext"] == 0 and (out["row_off"] == 0).all() and pileup.last_rows_info() == want.info
    # entries without a column or a quality byte: alnA, alnB may be NULL
    two = (pi.Entry("err3", "", b"", b"", 9, 9), pi.Entry("unmapped", "", b"", b"", 0, 0, flags=0))
    rc, _, out = _raw(qi.QualSet("no_columns", two, (0, 0), (b"", b""), e.ref, ()), null=("alnA", "alnB"), with_qual=False)
    assert rc == _lib.OK and list(out["err"]) == [3, 0] and out["ntext"] == 0


def test_order_that_is_no_permutation():
    from poly_amd import _lib
    s = SETS["regions"].qs
    n = len(s.entries)
    text = np.full(4096, 0xAB, np.uint8)
    for bad in ([0, 1, 1, 3], [0, 1, n, 3], [0, 1, 0xFFFFFFFF, 3]):
        rc, msg, out = _raw(s, text=text, cap=len(text), order=np.array(bad, np.uint32))
        assert rc == _lib.ERR_INVALID and "order is not a permutation" in msg and "polyhip_pileup_rows" in msg, msg
        assert out["ntext"] == 0xAB and (out["err"] == 0xABABABAB).all() and (out["row_off"] == 0xABABABABABABABAB).all() and (text == 0xAB).all()
    rc, _, out = _raw(s, text=text, cap=len(text), order=np.array([3, 1, 0, 2], np.uint32))
    want = ro.pileup_rows(*[qi.pack(s)[f] for f in ARGS], s.ref, b"seq1", order=[3, 1, 0, 2])
    assert rc == _lib.OK and text[:out["ntext"]].tobytes() == want.text


def test_argument_errors_in_order():
    from poly_amd import _lib
    s = SETS["regions"].qs
    p = qi.pack(s)
    every = ARGS + ("ref", "ntext", "err", "name")
    down = dict(p, aln_off=p["aln_off"][::-1].copy(), qual_off=p["qual_off"][::-1].copy())
    qdown = dict(p, qual_off=p["qual_off"][::-1].copy())
    L = len(s.ref)
    notperm = np.array([0, 0, 0, 0], np.uint32)
    worst = dict(null=every, n_claimed=1 << 32, all_positions=2, qual_offset=163, name_len=0, order=notperm)
    text = np.full(16, 0xAB, np.uint8)
    steps = [                                                   # each call also has everything wrong that a later check looks for
        (dict(worst, params=False, st=dict(min_mapq=1, region=(3, 2), pos_origin=9)), _lib.ERR_INVALID, "null params"),
        (dict(worst, st=dict(min_mapq=1, region=(3, 2), pos_origin=9)), _lib.ERR_INVALID, "region_lo"),
        (dict(worst, st=dict(min_mapq=1, region=(3, L + 1), pos_origin=9)), _lib.ERR_INVALID, "region_hi"),
        (dict(worst, st=dict(min_mapq=1, region=(3, 9), pos_origin=4)), _lib.ERR_INVALID, "pos_origin = 4"),
        (dict(worst, st=dict(min_mapq=1, region=(3, 9), pos_origin=3)), _lib.ERR_INVALID, "all_positions = 2"),
        (dict(worst, st=dict(min_mapq=1), all_positions=1), _lib.ERR_INVALID, "qual_offset = 163"),
        (dict(worst, st=dict(min_mapq=1), all_positions=1, qual_offset=162, name_len=4), _lib.ERR_INVALID, "the name is null or empty"),
        (dict(worst, st=dict(min_mapq=1), all_positions=1, qual_offset=162, null=ARGS + ("ref", "ntext", "err")), _lib.ERR_INVALID,
         "the name is null or empty"),
        (dict(worst, st=dict(min_mapq=1), all_positions=1, qual_offset=162, null=ARGS + ("ref", "ntext", "err"), name_len=None, name=b"a b"),
         _lib.ERR_INVALID, "byte 1 of the name is 0x20"),
        (dict(worst, st=dict(min_mapq=1), all_positions=1, qual_offset=162, null=ARGS + ("ref", "ntext", "err"), name_len=None, name=b"ab\x7f"),
         _lib.ERR_INVALID, "byte 2 of the name is 0x7f"),
        (dict(worst, st=dict(min_mapq=1), all_positions=1, qual_offset=162, null=ARGS + ("ref", "ntext", "err"), name_len=None, name=b"~!"),
         _lib.ERR_UNSUPPORTED, f"{1 << 32} entries"),
        (dict(st=dict(min_mapq=1), null=ARGS + ("ref", "ntext", "err"), order=notperm), _lib.ERR_INVALID, "min_mapq = 1 needs mapq"),
        (dict(null=("ref",), p=down, order=notperm), _lib.ERR_INVALID, "null argument"),
        (dict(null=("ntext",), p=down, order=notperm), _lib.ERR_INVALID, "null argument"),
        (dict(cap=5, p=down, order=notperm), _lib.ERR_INVALID, "null argument"),
        (dict(null=("flags",), p=down, order=notperm), _lib.ERR_INVALID, "null argument"),
        (dict(null=("ref_end",), p=down, order=notperm), _lib.ERR_INVALID, "null argument"),
        (dict(null=("read_start",), p=down, order=notperm), _lib.ERR_INVALID, "null argument"),
        (dict(null=("alnB",), p=down, order=notperm), _lib.ERR_INVALID, "null argument"),
        (dict(null=("qual_off",), p=down, order=notperm), _lib.ERR_INVALID, "null argument"),
        (dict(null=("err",), p=down, order=notperm), _lib.ERR_INVALID, "null argument"),
        (dict(p=down, order=notperm), _lib.ERR_INVALID, "not ascending"),
        (dict(p=qdown, order=notperm), _lib.ERR_INVALID, "not ascending"),
        (dict(order=notperm), _lib.ERR_INVALID, "order is not a permutation"),
    ]
    for kw, status, what in steps:
        kw = dict(kw)
        st = kw.pop("st", None)
        kw.setdefault("text", text)
        kw.setdefault("cap", len(text))
        if "cap" in kw and kw["cap"] == 5:
            kw["text"] = None                                   # a capacity without a buffer
        rc, msg, out = _raw(s, st, **kw)
        assert rc == status and what in msg and "polyhip_pileup_rows" in msg, (what, msg)
        assert out["ntext"] == 0xAB and (out["err"] == 0xABABABAB).all() and (out["row_off"] == 0xABABABABABABABAB).all() and (text == 0xAB).all()
    # what may be NULL: mapq without min_mapq, the qualities with read_start and qual_off, order, row_off; a reversed qual_off is then not read
    rc, msg, _ = _raw(s, null=("mapq", "row_off"), p=qdown, with_qual=False)
    assert rc == _lib.ERR_INVALID and "the text needs" in msg                   # nothing wrong but the capacity
    rc, msg, out = _raw(s, qual_offset=162)                                     # the largest offset is taken: every byte is below it
    assert rc == _lib.OK and out["ntext"] == 0 and (out["err"] == 7).all()


# ---------------------------------------------------------------- 3. end to end: FASTQ image -> mapper -> records -> duplicates, order -> rows
def _fastq(reads, rng):
    quals = [bytes(rng.integers(qi.Q_LO, qi.Q_HI + 1, len(r), dtype=np.uint8)) for r in reads]
    return b"".join(b"@r%d\n" % k + r + b"\n+\n" + q + b"\n" for k, (r, q) in enumerate(zip(reads, quals)))


def test_end_to_end_from_a_fastq_image(nuc4_scoring):
    from poly_amd import bwt, dedup, fastq, mapper, pileup, pileup_text, sam
    d = pi.planted()
    T = d["T"]
    rng = np.random.default_rng(ri.SEED + 50)
    reads = list(d["reads"]) + [d["reads"][k] for k in range(0, 200, 10)]         # 200 reads and 20 copies
    seqs, offs, quals, qoffs, rec_start, err, mismatch = fastq.pack_qual(_fastq(reads, rng), with_mismatch=True)
    assert err is None and len(offs) == 221 and mismatch == 0
    result = mapper.map_reads_affine_packed(bwt.New(T), nuc4_scoring, *mai.GAPS[0], seqs, offs, _params(mai.PARAMS))
    rec = sam.records(result, 100)
    m = dedup.mark(result, 100, quals=quals, qual_offsets=qoffs)
    order = dedup.coord_order(rec, result)
    assert int(m.dup.sum()) == 20 and sorted(order.tolist()) == list(range(220)) and order.tolist() != list(range(220))
    got = pileup.rows(result, T, "T", quals, qoffs, records=rec, order=order, dup=m.dup, read_offsets=offs)
    a, b = b"".join(result.alignA), b"".join(result.alignB)
    flags = np.where(m.dup != 0, result.flags & ~np.uint32(1), result.flags).astype(np.uint32)
    want = ro.pileup_rows(flags, rec.mapq, result.ref_start, result.ref_end, result.read_start, a, b, result.aln_off, quals, qoffs, T, b"T",
                          order=order)
    _assert_same(got, want)
    assert not got.err.any() and pileup.last_rows_info()["used"] == 200 and got.last_info()["max_row_bytes"] < pileup_text.MAX_LINE_SIZE
    rows = got.parse()
    depth = pileup.pileup(result, T, records=rec, dup=m.dup).depth()
    assert len(rows) == int((depth > 0).sum()) and [x.position - 1 for x in rows] == np.nonzero(depth)[0].tolist()
    for x in rows:
        assert x.sequence == "T" and x.read_count == depth[x.position - 1] and len(x.quality) == x.read_count
        assert x.reference_base == chr(T[x.position - 1])
    at = {x.position - 1: x for x in rows}
    assert any(r.upper() == "-3CGT" for r in at[pi.PLANTED_DEL].read_results) and any(r[0] == "*" for r in at[pi.PLANTED_DEL + 1].read_results)
    assert any(r.upper() == "+2GG" for r in at[pi.PLANTED_INS].read_results)
    snv = chr(d["snv"])
    said = [r[2] if r[0] == "^" else r[0] for r in at[pi.PLANTED_SNV].read_results if r[0] not in "+-"]
    assert len(said) == depth[pi.PLANTED_SNV] and sum(x in (snv, snv.lower()) for x in said) * 10 >= 9 * len(said)
    # the reads of a row stand in coordinate order: a read that starts here ('^') never precedes one that started earlier
    for x in rows:
        starts = [r[0] == "^" for r in x.read_results if r[0] not in "+-"]
        assert starts == sorted(starts)
    with pytest.raises(ValueError, match="not as long as its read"):
        longer = qoffs.copy()
        longer[7:] += 1
        pileup.rows(result, T, "T", np.append(quals, quals[:1]), longer, read_offsets=offs)
    plain = pileup.rows(result, T, "T", all_positions=True)                       # no qualities, no records: '~' for both
    assert plain.nrows == len(T) and set(x.quality for x in plain.parse() if x.read_count) and all(
        set(x.quality) == {"~"} for x in plain.parse() if x.read_count)


def test_end_to_end_one_contig_of_three(nuc4_scoring):
    import map_refs_inputs as mri
    from map_check import _pack
    from poly_amd import dedup, mapper, pileup, refs, sam
    T = pi.planted()["T"]
    contigs = (T[:700], T[700:1300], T[1300:2000])
    rng = np.random.default_rng(ri.SEED + 51)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    reads = []
    for c, text in enumerate(contigs):
        for k in range(40):
            at = k * (len(text) - 80) // 39
            r = bytearray(text[at:at + 80])
            r[40] = b"CGTA"[b"ACGT".index(r[40])]                                  # one substitution a read
            reads.append(bytes(r).translate(comp)[::-1] if (k + c) % 2 else bytes(r))
    reads = [reads[int(k)] for k in rng.permutation(len(reads))]
    rs = refs.New(["a", "b", "c"], list(contigs))
    buf, offs = _pack(reads)
    quals = rng.integers(qi.Q_LO, qi.Q_HI + 1, int(offs[-1]), dtype=np.uint8)
    got = mapper.map_reads_refs_packed(rs, nuc4_scoring, mri.GO, mri.GE, buf, offs, _params(mri.P))
    rec = sam.records(got, 80)
    order = dedup.coord_order(rec, got)
    assert sorted(set(got.rid.tolist())) == [0, 1, 2] and (got.flags & 1).all()
    for c, region in ((1, None), (2, (95, 105)), (0, (0, 12))):
        rows = pileup.rows_refs(got, rs, c, b"ctg", quals, offs, records=rec, region=region, order=order, read_offsets=offs)
        keep = [int(i) for i in order if got.rid[i] == c]                          # the contig's entries alone, in coordinate order
        a, b = b"".join(got.alignA[i] for i in keep), b"".join(got.alignB[i] for i in keep)
        off = np.concatenate([[0], np.cumsum([len(got.alignA[i]) for i in keep])]).astype(np.uint64)
        q = b"".join(quals[int(offs[i]):int(offs[i + 1])].tobytes() for i in keep)
        qoff = np.concatenate([[0], np.cumsum([len(reads[i]) for i in keep])]).astype(np.uint64)
        want = ro.pileup_rows(got.flags[keep], rec.mapq[keep], got.ref_start[keep], got.ref_end[keep], got.read_start[keep], a, b, off, q, qoff,
                              contigs[c], b"ctg", region=region)
        assert rows.text.tobytes() == want.text and rows.row_off.tolist() == want.row_off.tolist() and not rows.err.any()
        lo, hi = region or (0, len(contigs[c]))
        assert rows.region_lo == lo and rows.last_info()["used"] == 40
        depth = pileup.pileup_refs(got, rs, c, records=rec, region=region).depth()
        parsed = rows.parse()
        assert [x.position for x in parsed] == [lo + j + 1 for j in np.nonzero(depth)[0]]      # local positions, 1-based
        assert [x.read_count for x in parsed] == depth[depth > 0].tolist()
        assert rows.row(lo + int(np.nonzero(depth)[0][0])) == want.rows[lo + int(np.nonzero(depth)[0][0])]
    with pytest.raises(ValueError, match="contig 3 of 3"):
        pileup.rows_refs(got, rs, 3, b"ctg")
