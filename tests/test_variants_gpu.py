"""polyhip_call_variants on the GPU against its CPU oracle (tests/variants_oracle.py): records, allele bytes, err, both sizes and
every info counter are compared exactly on the inputs of tests/variants_inputs.py (what they hold is asserted in
tests/test_variants_cpu.py), with and without qualities; against polyhip_pileup_qual itself; and end to end from a FASTQ image
through trim, the affine mapper, the records, the duplicate marks, the call and the VCF text back to the sample's sequence."""
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
import variants_inputs as vi  # noqa: E402
import variants_oracle as vo  # noqa: E402
from map_check import _params, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _set(name):
    return {s.name: s for s in vi.all_sets()}[name]


def _call(s, st, with_qual=True, p=None, **kw):
    from poly_amd import variants
    p = vi.pack(s) if p is None else p
    q = dict(read_start=p["read_start"], qual=p["qual"], qual_off=p["qual_off"]) if with_qual else {}
    return variants.call_packed(p["flags"], p["ref_start"], p["ref_end"], p["alnA"], p["alnB"], p["aln_off"], s.ref, p["mapq"], **q, **st, **kw)


def _assert_same(got, want):
    from poly_amd import variants
    assert got.status == 0 and got.records.dtype == want.records.dtype == variants.VARIANT_DTYPE
    assert got.nvariants == len(want.records) == len(got.records) and got.nallele_bytes == len(want.alleles) == len(got.alleles)
    for f in want.records.dtype.names:
        bad = np.flatnonzero(got.records[f] != want.records[f])
        assert bad.size == 0, f"{f}: {len(bad)} records differ, first {bad[0]}: got {got.records[bad[0]]}, want {want.records[bad[0]]}"
    assert got.alleles.tobytes() == want.alleles.tobytes() and (got.err == want.err).all()
    assert variants.last_info() == want.info == type(got).last_info()


# ---------------------------------------------------------------- 1. every set, every setting, with and without qualities
def test_set_names():
    assert tuple(s.name for s in vi.all_sets()) == vi.SET_NAMES


@pytest.mark.parametrize("name", vi.SET_NAMES)
def test_all_sets(name):
    s = _set(name)
    for st in s.settings:
        for with_qual in (True, False):
            if not with_qual and st["min_base_qual"]:
                continue
            want = vo.call_variants(*vi.oracle_args(s, with_qual), **st)
            got = _call(s, st, with_qual)
            _assert_same(got, want)
            again = _call(s, st, with_qual)                       # the same call gives the same bytes
            assert again.records.tobytes() == got.records.tobytes() and again.alleles.tobytes() == got.alleles.tobytes()


@pytest.mark.parametrize("name", vi.SET_NAMES)
def test_identity_with_the_pileup(name):
    """without left alignment and thresholds: the SNV records are polyhip_pileup_qual's SNV sites, and at every position with a
    record the insertion alleles' counts add up to its plane 6 and the deletion alleles' to plane 7, per strand, the runs above
    max_indel aside"""
    from poly_amd import pileup, variants
    s = _set(name)
    p = vi.pack(s)
    for st in s.settings:
        st = dict(st, left_align=0, min_alt_count=1, min_alt_permille=0, max_indel=255, min_depth=0)
        got = _call(s, st)
        info = variants.last_info()
        pst = {k: st[k] for k in ("region", "min_mapq", "min_depth", "min_alt_count", "min_alt_permille", "min_base_qual")}
        base = pileup.pileup_qual_packed(p["flags"], p["ref_start"], p["ref_end"], p["read_start"], p["alnA"], p["alnB"], p["aln_off"], p["qual"],
                                         p["qual_off"], s.ref, p["mapq"], **pst)
        shared = pileup.last_qual_info()
        assert (got.err == base.err).all() and all(info[f] == shared[f] for f in ("used", "skipped_mapq", "bad", "columns", "edge_events",
                                                                                   "filtered_bases"))
        snv, sites = got.records[got.records["kind"] == 1], base.sites[base.sites["kind"] == 1]
        assert len(snv) == len(sites) and all((snv[f] == sites[f]).all() for f in ("pos", "depth", "count", "count_fwd", "ref", "alt"))
        depth, short = base.depth(), 0
        for kind, ch in ((2, 6), (3, 7)):
            r = got.records[got.records["kind"] == kind]
            two, fwd = np.zeros(base.counts.shape[1], np.int64), np.zeros(base.counts.shape[1], np.int64)
            np.add.at(two, r["pos"].astype(np.int64) - got.region_lo, r["count"])
            np.add.at(fwd, r["pos"].astype(np.int64) - got.region_lo, r["count_fwd"])
            plane2, plane1 = base.counts[ch].astype(np.int64) + base.counts[8 + ch], base.counts[ch].astype(np.int64)
            covered = depth >= 1
            assert (two[covered] <= plane2[covered]).all() and (fwd[covered] <= plane1[covered]).all() and not two[~covered].any()
            short += int((plane2 - two)[covered].sum())
        assert short <= info["long_events"] and (name != "lengths" or st["region"] is not None or short == info["long_events"] == 3)


def test_dup_and_mapq_pass_through():
    from poly_amd import variants
    s = _set("grouping")
    p = vi.pack(s)
    dup = np.zeros(len(s.entries), np.uint8)
    dup[:40] = 1
    got = _call(s, s.settings[0], dup=dup)
    want = vo.call_variants(np.where(dup != 0, 0, p["flags"]), *vi.oracle_args(s)[1:], **s.settings[0])
    _assert_same(got, want)
    assert variants.last_info()["used"] == len(s.entries) - 40 and 73 - 40 in got.records["count"]      # 40 reads of the large allele are gone


# ---------------------------------------------------------------- 2. the C call itself
def _raw(s, st, with_qual=True, vcap=0, acap=0, records=None, alleles=None, null=(), n=None, p=None):
    """polyhip_call_variants -> (status, message, outputs); `null`: arguments passed as NULL.  err starts out as 0xAB bytes"""
    from poly_amd import _lib, variants
    from poly_amd.pileup import _CParams, _CQualParams
    p = vi.pack(s) if p is None else p
    n = len(s.entries) if n is None else n
    lo, hi = st["region"] or (0, len(s.ref))
    cp = variants._CVarParams(_CQualParams(_CParams(lo, hi, st["min_mapq"], st["min_depth"], st["min_alt_count"], st["min_alt_permille"]),
                                           st["min_base_qual"], 33), st["left_align"], st["hom_permille"], st["max_indel"], 0)
    err, nv, nb = np.full(n, 0xABABABAB, np.uint32), C.c_uint64(0xAB), C.c_uint64(0xAB)
    ref = np.frombuffer(s.ref, np.uint8)
    skip = set(null) | (set() if with_qual else {"qual", "qual_off", "read_start"})
    a = lambda k: None if k in skip else p[k].ctypes.data      # noqa: E731
    rc = _lib.lib().polyhip_call_variants(C.byref(cp), n, a("flags"), a("mapq"), a("ref_start"), a("ref_end"), a("read_start"), a("alnA"), a("alnB"),
                                          a("aln_off"), a("qual"), a("qual_off"), ref.ctypes.data, len(s.ref), C.byref(nv),
                                          None if records is None else records.ctypes.data, vcap, C.byref(nb),
                                          None if alleles is None else alleles.ctypes.data, acap, None if "err" in null else err.ctypes.data)
    return rc, _lib.lib().polyhip_last_error().decode(), dict(err=err, nvariants=int(nv.value), nallele_bytes=int(nb.value))


def test_capacities():
    from poly_amd import _lib, variants
    s = _set("lengths")
    st = s.settings[0]
    want = vo.call_variants(*vi.oracle_args(s), **st)
    nv, nb = len(want.records), len(want.alleles)
    assert nv >= 20 and nb > 500
    rec = lambda: np.full(40 * (nv + 2), 0xAB, np.uint8).view(variants.VARIANT_DTYPE)      # noqa: E731
    pool = lambda: np.full(nb + 2, 0xAB, np.uint8)                                          # noqa: E731
    rc, msg, out = _raw(s, st)                                                             # NULL and no capacity: the sizes
    assert rc == _lib.ERR_INVALID and f"the variants need {nv} entries" in msg and (out["nvariants"], out["nallele_bytes"]) == (nv, nb)
    assert (out["err"] == want.err).all() and variants.last_info() == want.info
    for vcap, acap, word in ((nv - 1, nb, f"the variants need {nv} entries, the buffer holds {nv - 1}"),
                             (nv, nb - 1, f"the alleles need {nb} bytes, the buffer holds {nb - 1}"), (nv, 0, f"the alleles need {nb} bytes"),
                             (nv - 1, nb - 1, "the variants need")):
        r, a = rec(), pool()
        rc, msg, out = _raw(s, st, vcap=vcap, acap=acap, records=r, alleles=a)
        assert rc == _lib.ERR_INVALID and word in msg and "polyhip_call_variants" in msg, msg
        assert (r.view(np.uint8) == 0xAB).all() and (a == 0xAB).all()                      # nothing is written to either
        assert (out["nvariants"], out["nallele_bytes"]) == (nv, nb) and (out["err"] == want.err).all()
    r, a = rec(), pool()
    rc, _, out = _raw(s, st, vcap=nv, acap=nb, records=r, alleles=a)                        # exactly what was asked for, not a byte beyond
    assert rc == _lib.OK and r[:nv].tobytes() == want.records.tobytes() and (r[nv:].view(np.uint8) == 0xAB).all()
    assert a[:nb].tobytes() == want.alleles.tobytes() and (a[nb:] == 0xAB).all()
    short = _call(s, st, variant_capacity=nv - 1)                                           # the wrapper with a capacity the caller fixed
    assert short.status == _lib.ERR_INVALID and short.records is None and (short.nvariants, short.nallele_bytes) == (nv, nb)
    short = _call(s, st, allele_capacity=nb - 1)
    assert short.status == _lib.ERR_INVALID and short.alleles is None and (short.nvariants, short.nallele_bytes) == (nv, nb)
    big = _set("shapes")                                                                    # the wrapper's guess is short: it runs again
    want = vo.call_variants(*vi.oracle_args(big), **big.settings[0])
    assert len(want.records) > len(big.ref) // 64 + 1024
    _assert_same(_call(big, big.settings[0]), want)


def test_calls_that_need_little():
    from poly_amd import _lib, variants
    s = _set("text_start")
    st = s.settings[0]
    every = ("flags", "mapq", "ref_start", "ref_end", "read_start", "alnA", "alnB", "aln_off", "qual", "qual_off", "err")
    rc, _, out = _raw(s, st, n=0, null=every)                                               # n == 0: no array is needed
    assert rc == _lib.OK and (out["nvariants"], out["nallele_bytes"]) == (0, 0)
    assert variants.last_info() == dict.fromkeys(vo.INFO_FIELDS, 0)
    want = vo.call_variants(*vi.oracle_args(s), **dict(st, region=(7, 7)))
    rc, _, out = _raw(s, dict(st, region=(7, 7)))                                           # L == 0: err and the counters
    assert rc == _lib.OK and (out["nvariants"], out["nallele_bytes"]) == (0, 0) and (out["err"] == want.err).all()
    assert variants.last_info() == want.info and want.info["open_events"] == 4
    rc, msg, out = _raw(s, st, null=("mapq",))                                              # mapq is not needed without min_mapq
    assert rc == _lib.ERR_INVALID and "the variants need 2 entries" in msg
    rc, msg, _ = _raw(s, dict(st, min_mapq=1), null=("mapq",))
    assert rc == _lib.ERR_INVALID and "min_mapq = 1 needs mapq" in msg
    # a non-NULL qual whose strings are all empty means qualities: every entry with a read base is err 6
    p = dict(vi.pack(s), qual=np.zeros(1, np.uint8), qual_off=np.zeros(len(s.entries) + 1, np.uint64))
    rc, _, out = _raw(s, st, p=p)
    assert rc == _lib.OK and (out["err"] == 6).all() and out["nvariants"] == 0


# ---------------------------------------------------------------- 3. 20,000 random entries
def test_random_entries_compared_whole():
    from poly_amd import variants
    s = vi.random_entries(20000, 3000, 13, max_cols=40)
    for st in s.settings:
        want = vo.call_variants(*vi.oracle_args(s), **st)
        _assert_same(_call(s, st), want)
    info = variants.last_info()
    assert info["used"] > 10000 and info["events"] > 10000 and info["alleles"] > 3000


# ---------------------------------------------------------------- 4. end to end: FASTQ image -> trim -> mapper -> records -> dedup -> call -> VCF
def _chain(index, text, nuc4_scoring, map_fn):
    from poly_amd import dedup, fastq, sam, trim
    d = vi.planted()
    seqs, offs, quals, qoffs, rec_start, err = fastq.pack_qual(d["fastq"])
    assert err is None and len(offs) == vi.PLANTED_READS + 1
    t = trim.trim_packed(seqs, offs, quals, qoffs, params=trim.TrimParams(min_qual_3p=20, min_qual_5p=20))
    assert not t.err.any() and (t.offsets == offs).all()                 # quality 'I' everywhere: nothing is cut
    result = map_fn(index, nuc4_scoring, *mai.GAPS[0], t.seqs, t.offsets, _params(mai.PARAMS))
    rec = sam.records(result, vi.PLANTED_READ)
    dup = dedup.mark(result, vi.PLANTED_READ, quals=t.quals, qual_offsets=t.offsets)
    return d, t, result, rec, dup


def _check_planted(d, v, name):
    from poly_amd import vcf
    text = vcf.write(v, d["T"], name)
    rows = vcf.parse(text)
    assert vi.called(rows) == list(d["variants"]) and all(r.gt == 2 and r.chrom == name for r in rows)
    assert vcf.apply(d["T"], rows) == d["sample"] == vcf.apply(d["T"], v)
    assert text.startswith(b"##fileformat=VCFv4.2\n") and text.count(b"\n") == 7 + len(rows)


def test_end_to_end_on_one_text(nuc4_scoring):
    from poly_amd import bwt, mapper, variants
    d = vi.planted()
    d, t, result, rec, dup = _chain(bwt.New(d["T"]), d["T"], nuc4_scoring, mapper.map_reads_affine_packed)
    a, b = b"".join(result.alignA), b"".join(result.alignB)
    for left_align in (1, 0):
        for with_qual in (True, False):
            q = dict(quals=t.quals, qual_offsets=t.offsets, read_offsets=t.offsets) if with_qual else {}
            v = variants.call(result, d["T"], records=rec, min_mapq=10, dup=dup.dup, left_align=left_align, **q, **vi.PLANTED_CALL)
            flags = np.where(dup.dup != 0, result.flags & ~np.uint32(1), result.flags)
            want = vo.call_variants(flags, rec.mapq, result.ref_start, result.ref_end, result.read_start, a, b, result.aln_off,
                                    t.quals if with_qual else None, t.offsets, d["T"],
                                    **dict(vi.DEFAULTS, **vi.PLANTED_CALL, min_mapq=10, left_align=left_align))
            _assert_same(v, want)
            assert not v.err.any() and variants.last_info()["used"] >= vi.PLANTED_READS - 20
            _check_planted(d, v, "construct")


def test_end_to_end_on_one_contig_of_three(nuc4_scoring):
    from poly_amd import mapper, refs, variants, vcf
    d = vi.planted()
    rng = np.random.default_rng(vi.SEED + 30)
    import pileup_inputs as pi
    contigs = [pi.random_text(rng, 700), d["T"], pi.random_text(rng, 450)]
    rs = refs.New(["left", "construct", "right"], contigs)
    d, t, result, rec, dup = _chain(rs, d["T"], nuc4_scoring, mapper.map_reads_refs_packed)
    assert (np.asarray(result.rid)[(result.flags & 1) != 0] == 1).all()
    v = variants.call_refs(result, rs, 1, quals=t.quals, qual_offsets=t.offsets, records=rec, dup=dup.dup, **vi.PLANTED_CALL)
    assert v.region_lo == 0 and v.ref.tobytes() == d["T"]
    keep = np.flatnonzero(np.asarray(result.rid) == 1)
    a, b = b"".join(result.alignA[i] for i in keep), b"".join(result.alignB[i] for i in keep)
    off = np.concatenate([[0], np.cumsum([len(result.alignA[i]) for i in keep])]).astype(np.uint64)
    q = b"".join(t.quals[int(t.offsets[i]):int(t.offsets[i + 1])].tobytes() for i in keep)
    qoff = np.concatenate([[0], np.cumsum([int(t.offsets[i + 1] - t.offsets[i]) for i in keep])]).astype(np.uint64)
    flags = np.where(dup.dup != 0, result.flags & ~np.uint32(1), result.flags)
    want = vo.call_variants(flags[keep], rec.mapq[keep], result.ref_start[keep], result.ref_end[keep], result.read_start[keep], a, b, off, q, qoff,
                            d["T"], **dict(vi.DEFAULTS, **vi.PLANTED_CALL))
    assert v.records.tobytes() == want.records.tobytes() and v.alleles.tobytes() == want.alleles.tobytes()
    _check_planted(d, v, "construct")
    empty = variants.call_refs(result, rs, 0, **vi.PLANTED_CALL)
    text = vcf.write_refs({0: empty, 1: v}, rs)
    assert text.count(b"##contig=") == 3 and b"##contig=<ID=right,length=450>" in text and vcf.parse(text) == vcf.rows(v, d["T"], "construct")
    part = variants.call_refs(result, rs, 1, region=(1000, 2000), **vi.PLANTED_CALL)
    assert part.region_lo == 1000 and [int(x) for x in part.records["pos"]] == [1200, 1500, 1800]
