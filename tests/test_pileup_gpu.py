"""polyhip_pileup on the GPU against its CPU oracle (tests/pileup_oracle.py): every output array and the info counters are
compared exactly on the hand-built inputs (tests/pileup_inputs.py; what they hold is asserted in tests/test_pileup_cpu.py),
on what the affine and the paired mapper return for their own test datasets, and on reads with planted variants."""
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
import map_pairs_inputs as mpi  # noqa: E402
import pileup_inputs as pi  # noqa: E402
import pileup_oracle as po  # noqa: E402
from map_check import _pack, _params, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu

INPUTS = ("flags", "mapq", "ref_start", "ref_end", "alnA", "alnB", "aln_off")
SET_NAMES = ("shapes", "edges", "regions", "contention", "random", "bytes", "errs", "thresholds", "batch1", "batch255", "batch256", "batch257")


@functools.lru_cache(maxsize=None)
def _set(name):
    return {s.name: s for s in pi.all_sets()}[name]


@functools.lru_cache(maxsize=None)
def _want(name, k):
    s = _set(name)
    p = pi.pack(s.entries)
    return po.pileup(*[p[f] for f in INPUTS], s.ref, **s.settings[k])


def _assert_same(got, want, info=True):
    from poly_amd import pileup
    assert got.sites.dtype == want.sites.dtype == pileup.SITE_DTYPE
    for f in ("counts", "consensus", "sites", "err"):
        have, need = getattr(got, f), getattr(want, f)
        assert have.dtype == need.dtype and have.shape == need.shape, (f, have.dtype, have.shape, need.shape)
        bad = np.argwhere(have != need)
        assert bad.size == 0, f"{f}: {len(bad)} items differ, first at {bad[0]}: got {have[tuple(bad[0])]}, want {need[tuple(bad[0])]}"
    assert got.nsites == len(want.sites)
    if info:
        assert pileup.last_info() == want.info


# ---------------------------------------------------------------- 1. the hand-built inputs
@pytest.mark.parametrize("name", SET_NAMES)
def test_hand_built_inputs(name):
    from poly_amd import pileup
    s = _set(name)
    p = pi.pack(s.entries)
    assert len(s.settings) >= 2
    for k, st in enumerate(s.settings):
        got = pileup.pileup_packed(p["flags"], p["ref_start"], p["ref_end"], p["alnA"], p["alnB"], p["aln_off"], s.ref, p["mapq"], **st)
        assert got.status == 0
        _assert_same(got, _want(name, k))
    want = _want(name, len(s.settings) - 1)
    assert got.depth().tolist() == (want.counts[:6].astype(np.uint64).sum(axis=0) + want.counts[8:14].astype(np.uint64).sum(axis=0)).tolist()
    assert got.consensus_string() == want.consensus.tobytes().decode("latin-1")


# ---------------------------------------------------------------- 2. the C call itself: capacity, the empty batch, errors
def _raw(s, setting=None, n=None, sites=None, cap=0, null=(), params=True, ref_len=None, p=None, n_claimed=None):
    """polyhip_pileup on an InputSet -> (status, message, outputs); `null`: arguments passed as NULL.  The outputs start out
    as 0xAB bytes, so what the call leaves alone shows"""
    from poly_amd import _lib, pileup
    p = pi.pack(s.entries) if p is None else p
    n = len(s.entries) if n is None else n
    st = dict(pi.DEFAULTS, **(setting or {}))
    lo, hi = st["region"] or (0, len(s.ref))
    L = max(hi - lo, 0)
    out = dict(counts=np.full((16, L), 0xABABABAB, np.uint32), consensus=np.full(L, 0xAB, np.uint8), err=np.full(n, 0xABABABAB, np.uint32))
    ns = C.c_uint64(0xAB)
    ref = np.frombuffer(s.ref, np.uint8)
    ptr = lambda k, a: None if k in null or a is None else a.ctypes.data    # noqa: E731
    cp = pileup._CParams(lo, hi, st["min_mapq"], st["min_depth"], st["min_alt_count"], st["min_alt_permille"])
    rc = _lib.lib().polyhip_pileup(C.byref(cp) if params else None, n if n_claimed is None else n_claimed, ptr("flags", p["flags"]),
                                   ptr("mapq", p["mapq"]), ptr("ref_start", p["ref_start"]), ptr("ref_end", p["ref_end"]),
                                   ptr("alnA", p["alnA"]), ptr("alnB", p["alnB"]), ptr("aln_off", p["aln_off"]), ptr("ref", ref),
                                   len(s.ref) if ref_len is None else ref_len, ptr("counts", out["counts"]),
                                   ptr("consensus", out["consensus"]), None if "nsites" in null else C.byref(ns), ptr("sites", sites), cap,
                                   ptr("err", out["err"]))
    out["nsites"] = int(ns.value)
    return rc, _lib.lib().polyhip_last_error().decode(), out


def test_short_capacity_and_size_only():
    from poly_amd import _lib, pileup
    s, want = _set("shapes"), _want("shapes", 0)
    p = pi.pack(s.entries)
    ns = len(want.sites)
    assert ns > 1000
    for cap in (ns - 1, 1, 0):
        sites = np.full(20 * ns, 0xAB, np.uint8).view(pileup.SITE_DTYPE)
        rc, msg, out = _raw(s, sites=sites, cap=cap)
        assert rc == _lib.ERR_INVALID and f"the sites need {ns} entries" in msg and f"holds {cap}" in msg and "polyhip_pileup" in msg
        assert (sites.view(np.uint8) == 0xAB).all()
        assert out["nsites"] == ns and (out["counts"] == want.counts).all() and (out["consensus"] == want.consensus).all()
        assert (out["err"] == want.err).all() and pileup.last_info() == want.info
    rc, msg, out = _raw(s)                                                      # NULL and no capacity: the size
    assert rc == _lib.ERR_INVALID and out["nsites"] == ns and (out["counts"] == want.counts).all()
    sites = np.full(20 * (ns + 3), 0xAB, np.uint8).view(pileup.SITE_DTYPE)
    rc, _, out = _raw(s, sites=sites, cap=ns)                                   # exactly what was asked for, and not a byte beyond
    assert rc == _lib.OK and (sites[:ns] == want.sites).all() and (sites[ns:].view(np.uint8) == 0xAB).all()
    rc, _, out = _raw(s, dict(pi.STRICT))                                       # no sites: the size-only call succeeds
    assert rc == _lib.OK and out["nsites"] == 0 and len(_want("shapes", 1).sites) == 0
    args = (p["flags"], p["ref_start"], p["ref_end"], p["alnA"], p["alnB"], p["aln_off"], s.ref, p["mapq"])
    short = pileup.pileup_packed(*args, site_capacity=ns - 1)                  # the wrapper with a capacity the caller fixed
    assert short.status == _lib.ERR_INVALID and short.sites is None and short.nsites == ns and (short.counts == want.counts).all()
    assert ns > len(s.ref) // 64 + 1024                                         # the wrapper's guess is short: it runs again
    _assert_same(pileup.pileup_packed(*args), want)
    _assert_same(pileup.pileup_packed(*args, site_capacity=ns), want)


def test_empty_batch_and_empty_region():
    from poly_amd import _lib, pileup
    s = _set("edges")
    none = pi.pack(())
    rc, _, out = _raw(s, n=0, p=none, null=INPUTS + ("err",))
    assert rc == _lib.OK and out["nsites"] == 0 and (out["counts"] == 0).all() and out["consensus"].tobytes() == b"N" * len(s.ref)
    assert pileup.last_info() == dict(entries=0, used=0, skipped_mapq=0, bad=0, columns=0, edge_events=0, sites=0)
    got = pileup.pileup_packed(none["flags"], none["ref_start"], none["ref_end"], none["alnA"], none["alnB"], none["aln_off"], s.ref)
    assert got.status == 0 and got.counts.shape == (16, len(s.ref)) and len(got.sites) == 0 and len(got.err) == 0
    e = _set("errs")
    want = po.pileup(*[pi.pack(e.entries)[f] for f in INPUTS], e.ref, region=(7, 7))
    rc, _, out = _raw(e, dict(region=(7, 7)), null=("counts", "consensus"))   # L == 0: err and *nsites are the only outputs
    assert rc == _lib.OK and out["nsites"] == 0 and (out["err"] == want.err).all() and pileup.last_info() == want.info
    # entries without a column: alnA and alnB may be NULL
    two = (pi.Entry("err3", "", b"", b"", 9, 9), pi.Entry("unmapped", "", b"", b"", 0, 0, flags=0))
    rc, _, out = _raw(pi.InputSet("no_columns", two, e.ref, ()), null=("alnA", "alnB"))
    assert rc == _lib.OK and list(out["err"]) == [3, 0] and (out["counts"] == 0).all()


def test_argument_errors_in_order():
    from poly_amd import _lib
    s = _set("regions")
    p = pi.pack(s.entries)
    every = INPUTS + ("ref", "counts", "consensus", "nsites", "err")
    down = dict(p, aln_off=p["aln_off"][::-1].copy())
    L = len(s.ref)
    bad = dict(min_alt_permille=1001, min_mapq=1)
    steps = [                                                   # each call also has everything wrong that a later check looks for
        (dict(params=False, setting=dict(bad, region=(3, 2)), null=every, n_claimed=1 << 32), _lib.ERR_INVALID, "null params"),
        (dict(setting=dict(bad, region=(3, 2)), null=every, n_claimed=1 << 32), _lib.ERR_INVALID, "region_lo"),
        (dict(setting=dict(bad, region=(3, L + 1)), null=every, n_claimed=1 << 32), _lib.ERR_INVALID, "region_hi"),
        (dict(setting=dict(bad), null=every, n_claimed=1 << 32), _lib.ERR_INVALID, "min_alt_permille = 1001"),
        (dict(setting=dict(min_mapq=1), null=every, n_claimed=1 << 32), _lib.ERR_UNSUPPORTED, "4294967296 entries"),
        (dict(setting=dict(min_mapq=1), null=every), _lib.ERR_INVALID, "min_mapq = 1 needs mapq"),
        (dict(null=("ref",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("nsites",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("counts",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("consensus",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(cap=5, p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("flags",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("ref_end",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("alnB",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(null=("err",), p=down), _lib.ERR_INVALID, "null argument"),
        (dict(p=down), _lib.ERR_INVALID, "not ascending"),
    ]
    for kw, status, text in steps:
        rc, msg, out = _raw(s, **kw)
        assert rc == status and text in msg and "polyhip_pileup" in msg, (text, msg)
        assert out["nsites"] == 0xAB and (out["err"] == 0xABABABAB).all() and (out["counts"] == 0xABABABAB).all()
    rc, msg, _ = _raw(s, null=("mapq",))                                        # mapq is not needed without min_mapq
    assert rc == _lib.ERR_INVALID and "the sites need" in msg                   # nothing wrong but the capacity


# ---------------------------------------------------------------- 3. end to end: what the mappers return
def _end_to_end(result, T, reads, paired):
    from poly_amd import pileup, sam
    rec = sam.records(result, np.array([len(r) for r in reads], np.uint32), paired=paired)
    a, b = b"".join(result.alignA), b"".join(result.alignB)
    out = []
    for kw in (dict(min_mapq=0), dict(min_mapq=20, min_depth=2, min_alt_permille=200)):
        got = pileup.pileup(result, T, records=rec, **kw)
        want = po.pileup(result.flags, rec.mapq, result.ref_start, result.ref_end, a, b, result.aln_off, T, **kw)
        _assert_same(got, want)
        assert want.info["bad"] == 0 and want.info["used"] > len(reads) // 2 and want.info["used"] + want.info["skipped_mapq"] == int(
            (result.flags & 1).sum())
        out.append(got)
    assert out[0].counts[8:].sum() > 0 and out[0].counts[[6, 7, 14, 15]].sum() > 0
    part = pileup.pileup(result, T, region=(len(T) // 3, len(T) // 2))          # without records: min_mapq 0
    assert (part.counts == out[0].counts[:, len(T) // 3:len(T) // 2]).all()
    assert part.consensus_string() == out[0].consensus_string()[len(T) // 3:len(T) // 2]
    return out


def test_end_to_end_affine(nuc4_scoring):
    from poly_amd import bwt, mapper
    d = mai.dataset()
    result = mapper.map_reads_affine_packed(bwt.New(d["T"]), nuc4_scoring, *mai.GAPS[0], *_pack(d["reads"]), _params(mai.PARAMS))
    _end_to_end(result, d["T"], d["reads"], False)
    from poly_amd import pileup
    assert pileup.last_info()["skipped_mapq"] == 0                             # the last call had no records


def test_end_to_end_pairs(nuc4_scoring):
    from poly_amd import bwt, mapper
    d = mpi.dataset()
    PP = mapper.PairParams(mpi.PAIR.min_insert, mpi.PAIR.max_insert, mpi.PAIR.rescue)
    result = mapper.map_pairs_packed(bwt.New(d["T"]), nuc4_scoring, *mpi.GAPS[0], *_pack(d["reads1"]), *_pack(d["reads2"]),
                                     _params(mpi.PARAMS), PP, max_len=mpi.MAX_LEN)
    _end_to_end(result, d["T"], [r for pair in zip(d["reads1"], d["reads2"]) for r in pair], True)


def test_planted_variants_through_the_gpu_mapper(nuc4_scoring):
    from poly_amd import bwt, mapper, pileup, sam
    d = pi.planted()
    T = d["T"]
    result = mapper.map_reads_affine_packed(bwt.New(T), nuc4_scoring, *mai.GAPS[0], *_pack(d["reads"]), _params(mai.PARAMS))
    rec = sam.records(result, 100)
    got = pileup.pileup(result, T, records=rec, min_mapq=20, min_alt_permille=500)
    want = po.pileup(result.flags, rec.mapq, result.ref_start, result.ref_end, b"".join(result.alignA), b"".join(result.alignB),
                     result.aln_off, T, min_mapq=20, min_alt_permille=500)
    _assert_same(got, want)
    assert [(int(x["pos"]), int(x["kind"])) for x in got.sites] == list(pi.PLANTED_SITES)
    assert got.sites[0]["alt"] == d["snv"] and got.sites[0]["ref"] == T[pi.PLANTED_SNV]
    assert got.consensus_string()[995:1008] == (T[995:1000] + b"***" + T[1003:1008]).decode()
    assert pileup.last_info()["used"] == 200
