"""polyhip_pileup_qual on the GPU against its CPU oracle (tests/pileup_qual_oracle.py): counts, qsum, consensus, sites, err and
the info counters are compared exactly on the inputs of tests/pileup_qual_inputs.py (what they hold is asserted in
tests/test_pileup_qual_cpu.py), against polyhip_pileup itself at min_base_qual = 0, and end to end from a FASTQ image with
a low-quality decoy."""
import ctypes as C
import functools
import io
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
import pileup_qual_oracle as qo  # noqa: E402
from map_check import _pack, _params, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ARGS = ("flags", "mapq", "ref_start", "ref_end", "read_start", "alnA", "alnB", "aln_off", "qual", "qual_off")
SET_NAMES = ("shapes", "edges", "regions", "contention", "random", "bytes", "errs", "thresholds", "batch1", "batch255", "batch256", "batch257",
             "quality_errs", "crossing")
FIELDS = ("counts", "qsum", "consensus", "sites", "err")


@functools.lru_cache(maxsize=None)
def _set(name):
    return {s.name: s for s in qi.all_sets()}[name]


@functools.lru_cache(maxsize=None)
def _want(name, k, min_base_qual):
    s = _set(name)
    p = qi.pack(s)
    return qo.pileup_qual(*[p[f] for f in ARGS], s.ref, **s.settings[k], min_base_qual=min_base_qual)


def _call(p, ref, **kw):
    from poly_amd import pileup
    return pileup.pileup_qual_packed(p["flags"], p["ref_start"], p["ref_end"], p["read_start"], p["alnA"], p["alnB"], p["aln_off"], p["qual"],
                                     p["qual_off"], ref, p["mapq"], **kw)


def _assert_same(got, want, info=True):
    from poly_amd import pileup
    assert got.sites.dtype == want.sites.dtype == pileup.SITE_DTYPE
    for f in FIELDS:
        have, need = getattr(got, f), getattr(want, f)
        assert have.dtype == need.dtype and have.shape == need.shape, (f, have.dtype, have.shape, need.shape)
        bad = np.argwhere(have != need)
        assert bad.size == 0, f"{f}: {len(bad)} items differ, first at {bad[0]}: got {have[tuple(bad[0])]}, want {need[tuple(bad[0])]}"
    assert got.nsites == len(want.sites)
    if info:
        assert pileup.last_qual_info() == want.info


# ---------------------------------------------------------------- 1. every set, every setting, three thresholds; batches of 1, 255, 256, 257
def test_set_names():
    assert tuple(s.name for s in qi.all_sets()) == SET_NAMES and qi.MIN_BASE_QUALS == (0, 20, 42)


@pytest.mark.parametrize("name", SET_NAMES)
def test_all_sets(name):
    from poly_amd import pileup
    s = _set(name)
    p = qi.pack(s)
    for k, st in enumerate(s.settings):
        for t in qi.MIN_BASE_QUALS:
            got = _call(p, s.ref, **st, min_base_qual=t)
            assert got.status == 0
            _assert_same(got, _want(name, k, t))
            assert type(got).last_info() == _want(name, k, t).info
        # the identity: at threshold 0 everything polyhip_pileup gives, it gives (the two sets with err 6 / 7 aside)
        got = _call(p, s.ref, **st)
        base = pileup.pileup_packed(p["flags"], p["ref_start"], p["ref_end"], p["alnA"], p["alnB"], p["aln_off"], s.ref, p["mapq"], **st)
        shared = pileup.last_info()
        if name != "quality_errs":
            for f in ("counts", "consensus", "sites", "err"):
                assert (getattr(got, f) == getattr(base, f)).all(), f
            assert {f: _want(name, k, 0).info[f] for f in shared} == shared
        # the sum of the qualities of the counted bases never exceeds 41 (93 in quality_errs) a base
        top = 93 if name == "quality_errs" else 41
        both = got.counts.reshape(2, 8, -1)[:, :4].reshape(8, -1)
        assert (got.qsum <= top * both).all()


def test_another_qual_offset():
    for name in ("shapes", "quality_errs", "crossing"):
        s = _set(name)
        for t in (0, 20):
            got = _call(qi.pack(s, rebase=31), s.ref, **s.settings[0], min_base_qual=t, qual_offset=64)
            _assert_same(got, _want(name, 0, t))
    s = _set("crossing")                                       # read at the wrong offset every byte is 31 too high: Q up to 72, still in range
    got = _call(qi.pack(s, rebase=31), s.ref, min_base_qual=42)
    assert int(got.err.sum()) == 0 and type(got).last_info()["filtered_bases"] < _want("crossing", 0, 42).info["filtered_bases"]


# ---------------------------------------------------------------- 2. the C call itself
def _raw(s, setting=None, n=None, sites=None, cap=0, null=(), params=True, ref_len=None, p=None, n_claimed=None, min_base_qual=0, qual_offset=33):
    """polyhip_pileup_qual on a QualSet -> (status, message, outputs); `null`: arguments passed as NULL.  The outputs start out as
    0xAB bytes, so what the call leaves alone shows"""
    from poly_amd import _lib, pileup
    p = qi.pack(s) if p is None else p
    n = len(s.entries) if n is None else n
    st = dict(pi.DEFAULTS, **(setting or {}))
    lo, hi = st["region"] or (0, len(s.ref))
    L = max(hi - lo, 0)
    out = dict(counts=np.full((16, L), 0xABABABAB, np.uint32), qsum=np.full((8, L), 0xABABABAB, np.uint32), consensus=np.full(L, 0xAB, np.uint8),
               err=np.full(n, 0xABABABAB, np.uint32))
    ns = C.c_uint64(0xAB)
    ref = np.frombuffer(s.ref, np.uint8)
    ptr = lambda k, a: None if k in null or a is None else a.ctypes.data    # noqa: E731
    cp = pileup._CQualParams(pileup._CParams(lo, hi, st["min_mapq"], st["min_depth"], st["min_alt_count"], st["min_alt_permille"]),
                             min_base_qual, qual_offset)
    rc = _lib.lib().polyhip_pileup_qual(C.byref(cp) if params else None, n if n_claimed is None else n_claimed, ptr("flags", p["flags"]),
                                        ptr("mapq", p["mapq"]), ptr("ref_start", p["ref_start"]), ptr("ref_end", p["ref_end"]),
                                        ptr("read_start", p["read_start"]), ptr("alnA", p["alnA"]), ptr("alnB", p["alnB"]),
                                        ptr("aln_off", p["aln_off"]), ptr("qual", p["qual"]), ptr("qual_off", p["qual_off"]), ptr("ref", ref),
                                        len(s.ref) if ref_len is None else ref_len, ptr("counts", out["counts"]), ptr("qsum", out["qsum"]),
                                        ptr("consensus", out["consensus"]), None if "nsites" in null else C.byref(ns), ptr("sites", sites), cap,
                                        ptr("err", out["err"]))
    out["nsites"] = int(ns.value)
    return rc, _lib.lib().polyhip_last_error().decode(), out


def test_short_capacity_and_size_only():
    from poly_amd import _lib, pileup
    s, want = _set("shapes"), _want("shapes", 0, 20)
    ns = len(want.sites)
    assert ns > 1000
    for cap in (ns - 1, 0):
        sites = np.full(20 * ns, 0xAB, np.uint8).view(pileup.SITE_DTYPE)
        rc, msg, out = _raw(s, sites=sites, cap=cap, min_base_qual=20)
        assert rc == _lib.ERR_INVALID and f"the sites need {ns} entries" in msg and f"holds {cap}" in msg and "polyhip_pileup_qual" in msg
        assert (sites.view(np.uint8) == 0xAB).all()
        assert out["nsites"] == ns and (out["counts"] == want.counts).all() and (out["qsum"] == want.qsum).all()
        assert (out["consensus"] == want.consensus).all() and (out["err"] == want.err).all() and pileup.last_qual_info() == want.info
    rc, msg, out = _raw(s, min_base_qual=20)                                     # NULL and no capacity: the size
    assert rc == _lib.ERR_INVALID and out["nsites"] == ns and (out["qsum"] == want.qsum).all()
    sites = np.full(20 * (ns + 3), 0xAB, np.uint8).view(pileup.SITE_DTYPE)
    rc, _, out = _raw(s, sites=sites, cap=ns, min_base_qual=20)                  # exactly what was asked for, and not a byte beyond
    assert rc == _lib.OK and (sites[:ns] == want.sites).all() and (sites[ns:].view(np.uint8) == 0xAB).all()
    p = qi.pack(s)
    short = _call(p, s.ref, site_capacity=ns - 1, min_base_qual=20)              # the wrapper with a capacity the caller fixed
    assert short.status == _lib.ERR_INVALID and short.sites is None and short.nsites == ns and (short.qsum == want.qsum).all()
    assert ns > len(s.ref) // 64 + 1024                                          # the wrapper's guess is short: it runs again
    _assert_same(_call(p, s.ref, min_base_qual=20), want)


def test_empty_batch_and_empty_region():
    from poly_amd import _lib, pileup
    s = _set("edges")
    none = qi.pack(qi.QualSet("none", (), (), (), s.ref, ()))
    rc, _, out = _raw(s, n=0, p=none, null=ARGS + ("err",))
    assert rc == _lib.OK and out["nsites"] == 0 and (out["counts"] == 0).all() and (out["qsum"] == 0).all()
    assert out["consensus"].tobytes() == b"N" * len(s.ref)
    assert pileup.last_qual_info() == dict(entries=0, used=0, skipped_mapq=0, bad=0, columns=0, edge_events=0, sites=0, filtered_bases=0)
    got = _call(none, s.ref)
    assert got.status == 0 and got.counts.shape == (16, len(s.ref)) and got.qsum.shape == (8, len(s.ref)) and len(got.sites) == 0
    e = _set("quality_errs")
    p = qi.pack(e)
    want = qo.pileup_qual(*[p[f] for f in ARGS], e.ref, region=(7, 7), min_base_qual=20)
    rc, _, out = _raw(e, dict(region=(7, 7)), null=("counts", "qsum", "consensus"), min_base_qual=20)   # L == 0: err and *nsites only
    assert rc == _lib.OK and out["nsites"] == 0 and (out["err"] == want.err).all() and pileup.last_qual_info() == want.info
    assert want.info["filtered_bases"] > 0                                     # counted whatever the region
    # entries without a column or a quality byte: alnA, alnB and qual may be NULL
    two = (pi.Entry("err3", "", b"", b"", 9, 9), pi.Entry("unmapped", "", b"", b"", 0, 0, flags=0))
    rc, _, out = _raw(qi.QualSet("no_columns", two, (0, 0), (b"", b""), e.ref, ()), null=("alnA", "alnB", "qual"))
    assert rc == _lib.OK and list(out["err"]) == [3, 0] and (out["counts"] == 0).all() and (out["qsum"] == 0).all()


def test_argument_errors_in_order():
    from poly_amd import _lib
    s = _set("regions")
    p = qi.pack(s)
    every = ARGS + ("ref", "counts", "qsum", "consensus", "nsites", "err")
    down = dict(p, aln_off=p["aln_off"][::-1].copy(), qual_off=p["qual_off"][::-1].copy())
    qdown = dict(p, qual_off=p["qual_off"][::-1].copy())
    L = len(s.ref)
    bad = dict(min_alt_permille=1001, min_mapq=1)
    big = (1 << 32) // 93 + 1                                   # the smallest n with n * 93 >= 2^32
    assert (big - 1) * 93 < 1 << 32 <= big * 93
    worst = dict(null=every, n_claimed=big, min_base_qual=94, qual_offset=163)
    steps = [                                                   # each call also has everything wrong that a later check looks for
        (dict(worst, params=False, setting=dict(bad, region=(3, 2))), _lib.ERR_INVALID, "null params"),
        (dict(worst, setting=dict(bad, region=(3, 2))), _lib.ERR_INVALID, "region_lo"),
        (dict(worst, setting=dict(bad, region=(3, L + 1))), _lib.ERR_INVALID, "region_hi"),
        (dict(worst, setting=dict(bad)), _lib.ERR_INVALID, "min_alt_permille = 1001"),
        (dict(worst, setting=dict(min_mapq=1)), _lib.ERR_INVALID, "min_base_qual = 94"),
        (dict(worst, setting=dict(min_mapq=1), min_base_qual=93), _lib.ERR_INVALID, "qual_offset = 163"),
        (dict(worst, setting=dict(min_mapq=1), min_base_qual=93, qual_offset=162), _lib.ERR_UNSUPPORTED, f"{big} entries"),
        (dict(setting=dict(min_mapq=1), null=every), _lib.ERR_INVALID, "min_mapq = 1 needs mapq"),
        (dict(null=("ref",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("nsites",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("counts",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("qsum",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("consensus",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(cap=5, p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("flags",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("read_start",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("alnB",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("qual",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("qual_off",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("err",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(p=down), _lib.ERR_INVALID, "not ascending"),
        (dict(p=qdown), _lib.ERR_INVALID, "not ascending"),
    ]
    for kw, status, text in steps:
        rc, msg, out = _raw(s, **kw)
        assert rc == status and text in msg and "polyhip_pileup_qual" in msg, (text, msg)
        assert out["nsites"] == 0xAB and (out["err"] == 0xABABABAB).all() and (out["counts"] == 0xABABABAB).all()
        assert (out["qsum"] == 0xABABABAB).all() and (out["consensus"] == 0xAB).all()
    rc, msg, _ = _raw(s, null=("mapq",))                                        # mapq is not needed without min_mapq
    assert rc == _lib.ERR_INVALID and "the sites need" in msg                   # nothing wrong but the capacity
    rc, msg, out = _raw(s, min_base_qual=93, qual_offset=162)                   # the largest settings are taken: every byte is below 162
    assert rc == _lib.OK and out["nsites"] == 0 and (out["err"] == 7).all() and (out["counts"] == 0).all() and (out["qsum"] == 0).all()


# ---------------------------------------------------------------- 3. end to end: FASTQ image -> mapper -> records -> pileup
DECOY = 1200


@functools.lru_cache(maxsize=None)
def _planted_fastq():
    """pileup_inputs.planted()'s 200 reads as a FASTQ image, quality 'I' everywhere; a third of the reads that cover DECOY carry a
    wrong base of quality '#' there"""
    d = pi.planted()
    T, sample = d["T"], d["sample"]
    at_sample = DECOY - 3                                     # 3 bases are deleted in front of it (the insertion lies behind)
    assert sample[at_sample - 5:at_sample + 6] == T[DECOY - 5:DECOY + 6]
    wrong = b"CGTA"[b"ACGT".index(T[DECOY])]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    recs, covering, changed = [], 0, 0
    for k, r in enumerate(d["reads"]):
        start = k * (len(sample) - 100) // 199
        read, qual = bytearray(r), bytearray(b"I" * len(r))
        if start <= at_sample < start + 100:
            covering += 1
            if covering % 3 == 0:
                x = at_sample - start
                y = 99 - x if k % 2 else x                   # every second read is the reverse complement
                read[y] = bytes([wrong]).translate(comp)[0] if k % 2 else wrong
                qual[y] = ord("#")
                changed += 1
        recs.append(b"@r%d\n" % k + bytes(read) + b"\n+\n" + bytes(qual) + b"\n")
    assert changed >= 3 and changed * 1000 >= 200 * covering
    return b"".join(recs), wrong, changed


def test_end_to_end_from_a_fastq_image(nuc4_scoring):
    from poly_amd import bwt, fastq, mapper, pileup, sam
    d = pi.planted()
    T = d["T"]
    image, wrong, changed = _planted_fastq()
    seqs, offs, quals, qoffs, rec_start, err, mismatch = fastq.pack_qual(image, with_mismatch=True)
    assert err is None and len(offs) == 201 and mismatch == 0 and (offs == qoffs).all()
    result = mapper.map_reads_affine_packed(bwt.New(T), nuc4_scoring, *mai.GAPS[0], seqs, offs, _params(mai.PARAMS))
    rec = sam.records(result, 100)
    a, b = b"".join(result.alignA), b"".join(result.alignB)
    found = {}
    for t in (0, 20):
        got = pileup.pileup_qual(result, T, quals, qoffs, records=rec, min_alt_permille=200, min_base_qual=t, read_offsets=offs)
        want = qo.pileup_qual(result.flags, rec.mapq, result.ref_start, result.ref_end, result.read_start, a, b, result.aln_off, quals, qoffs, T,
                              min_alt_permille=200, min_base_qual=t)
        _assert_same(got, want)
        assert int(got.err.sum()) == 0 and pileup.last_qual_info()["used"] == 200
        found[t] = [(int(x["pos"]), int(x["kind"])) for x in got.sites]
        snv = got.sites[0]
        assert snv["pos"] == pi.PLANTED_SNV and snv["alt"] == d["snv"]
        k = b"ACGT".index(d["snv"])
        assert int(got.qsum[k, pi.PLANTED_SNV]) + int(got.qsum[4 + k, pi.PLANTED_SNV]) == 40 * int(snv["count"])
    planted = list(pi.PLANTED_SITES)
    assert found[0] == sorted(planted + [(DECOY, 1)]) and found[20] == planted      # the decoy is a site only while '#' bases count
    assert pileup.last_qual_info()["filtered_bases"] == changed
    # a quality one byte longer than its read raises no err in the library; the wrapper refuses it when it knows the reads' offsets
    longer = qoffs.copy()
    longer[7:] += 1
    with pytest.raises(ValueError, match="not as long as its read"):
        pileup.pileup_qual(result, T, np.append(quals, quals[:1]), longer, read_offsets=offs)
    # the SAM text carries each record's QUAL as the file has it, reversed on the reverse strand
    names = [b"r%d" % k for k in range(200)]
    reads = [seqs[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(200)]
    qs = [quals[int(qoffs[i]):int(qoffs[i + 1])].tobytes() for i in range(200)]
    fh = io.StringIO()
    sam.write(fh, "T", len(T), names, reads, qs, result, rec)
    rows = [ln.split("\t") for ln in fh.getvalue().splitlines() if not ln.startswith("@")]
    assert len(rows) == 200
    nrev = 0
    for i, row in enumerate(rows):
        reverse = bool(int(row[1]) & 16)
        nrev += reverse
        assert row[10] == (qs[i][::-1] if reverse else qs[i]).decode(), i
    assert nrev > 50 and any("#" in row[10] for row in rows)


# ---------------------------------------------------------------- 4. one contig of a reference of several
def test_pileup_qual_refs(nuc4_scoring):
    """pileup.pileup_qual_refs on tests/map_refs_inputs.many(): per contig against the oracle on that contig's entries alone, at
    threshold 0 against pileup.pileup_refs, and a region inside a contig"""
    import map_refs_inputs as ri
    from poly_amd import mapper, pileup, refs
    case = ri.many()
    rs = refs.New([f"c{i}" for i in range(len(case.contigs))], list(case.contigs))
    reads = list(case.reads)
    buf, offs = _pack(reads)
    got = mapper.map_reads_refs_packed(rs, nuc4_scoring, ri.GO, ri.GE, buf, offs, _params(ri.P))
    rng = np.random.default_rng(qi.SEED + 200)
    quals = rng.integers(qi.Q_LO, qi.Q_HI + 1, int(offs[-1]), dtype=np.uint8)
    for c in (2, ri.MANY_REPEAT[0], 299):
        keep = [i for i in range(len(reads)) if got.rid[i] == c]
        a, b = b"".join(got.alignA[i] for i in keep), b"".join(got.alignB[i] for i in keep)
        off = np.concatenate([[0], np.cumsum([len(got.alignA[i]) for i in keep])]).astype(np.uint64)
        q = b"".join(quals[int(offs[i]):int(offs[i + 1])].tobytes() for i in keep)
        qoff = np.concatenate([[0], np.cumsum([len(reads[i]) for i in keep])]).astype(np.uint64)
        for t in (0, 20):
            want = qo.pileup_qual(got.flags[keep], None, got.ref_start[keep], got.ref_end[keep], got.read_start[keep], a, b, off, q, qoff,
                                  case.contigs[c], min_depth=1, min_alt_count=1, min_base_qual=t)
            have = pileup.pileup_qual_refs(got, rs, c, quals, offs, min_base_qual=t, read_offsets=offs)
            assert (have.counts == want.counts).all() and (have.qsum == want.qsum).all() and (have.consensus == want.consensus).all()
            assert [tuple(int(x) for x in s) for s in have.sites.tolist()] == want.site_list()
            info = have.last_info()
            assert have.region_lo == 0 and not have.err.any() and (info["used"], info["filtered_bases"]) == (
                want.info["used"], want.info["filtered_bases"])
        plain = pileup.pileup_refs(got, rs, c)
        have = pileup.pileup_qual_refs(got, rs, c, quals, offs)
        assert (have.counts == plain.counts).all() and (have.sites == plain.sites).all() and want.info["filtered_bases"] > 0
    c = ri.MANY_REPEAT[0]
    part, whole = pileup.pileup_qual_refs(got, rs, c, quals, offs, region=(10, 40), min_base_qual=20), pileup.pileup_qual_refs(
        got, rs, c, quals, offs, min_base_qual=20)
    assert part.region_lo == 10 and (part.qsum == whole.qsum[:, 10:40]).all() and whole.qsum.any()
    with pytest.raises(ValueError, match="contig 300 of 300"):
        pileup.pileup_qual_refs(got, rs, 300, quals, offs)
