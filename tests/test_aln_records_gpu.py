"""polyhip_aln_records on the GPU against its CPU oracle (tests/aln_records_oracle.py): every array of sam.records is compared
exactly on the hand-built inputs (tests/aln_records_inputs.py; what they hold is asserted in tests/test_aln_records_cpu.py) and
on what the affine and the paired mapper return for their own test datasets."""
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
import aln_records_inputs as ari  # noqa: E402
import aln_records_oracle as aro  # noqa: E402
import map_affine_inputs as mai  # noqa: E402
import map_pairs_inputs as mpi  # noqa: E402
import oracle  # noqa: E402
from map_check import _pack, _params, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ARRAYS = ("cigar_off", "cigar", "md_off", "md", "nm", "mapq", "sam_flag", "err")
INPUTS = ("flags", "score", "second", "read_start", "read_end", "read_len", "alnA", "alnB", "aln_off")


@functools.lru_cache(maxsize=None)
def _set(name):
    if name == "cases":
        cs = ari.cases()
        return cs + (ari.unmapped(1),) * (len(cs) % 2)
    return ari.paired_batch() if name == "pairs" else ari.batch(int(name))


@functools.lru_cache(maxsize=None)
def _want(name, eqx, paired):
    p = ari.pack(_set(name))
    return aro.records(*[p[k] for k in INPUTS], eqx, paired)


def _assert_same(got, want, info=True):
    from poly_amd import sam
    for f in ARRAYS:
        have, need = getattr(got, f), getattr(want, f)
        assert have.dtype == need.dtype and have.shape == need.shape, (f, have.dtype, have.shape, need.shape)
        bad = np.nonzero(have != need)[0]
        assert bad.size == 0, f"{f}: {bad.size} items differ, first {bad[0]}: got {have[bad[0]]}, want {need[bad[0]]}"
    if info:
        assert sam.last_info() == want.info


# ---------------------------------------------------------------- 1. the hand-built inputs
@pytest.mark.parametrize("eqx", [False, True], ids=["m", "eqx"])
@pytest.mark.parametrize("name", ["cases", "pairs"] + [str(n) for n in ari.BATCH_SIZES])
def test_hand_built_inputs(name, eqx):
    from poly_amd import sam
    cs = _set(name)
    p = ari.pack(cs)
    for paired in (False, True) if len(cs) % 2 == 0 else (False,):
        got = sam.records_packed(**p, eqx=eqx, paired=paired)
        assert got.status == 0
        _assert_same(got, _want(name, eqx, paired))
    want = _want(name, eqx, False)
    for i in range(0, len(cs), 7):
        assert got.cigar_string(i) == want.cigar_string(i) and got.md_string(i) == want.md_string(i)


# ---------------------------------------------------------------- 2. the C call itself: capacities, the empty batch, errors
def _raw(p, n, eqx=0, paired=0, cigar=None, ccap=0, md=None, mcap=0, null=(), params=True):
    """polyhip_aln_records on the arrays of ari.pack -> (status, message, outputs); `null`: arguments passed as NULL"""
    from poly_amd import _lib, sam
    out = dict(cigar_off=np.full(n + 1, 7, np.uint64), md_off=np.full(n + 1, 7, np.uint64), nm=np.full(n, 7, np.uint32),
               mapq=np.full(n, 7, np.uint8), sam_flag=np.full(n, 7, np.uint32), err=np.full(n, 7, np.uint32))
    ptr = lambda k, a: None if k in null or a is None else a.ctypes.data    # noqa: E731
    cp = sam._CParams(eqx, paired)
    rc = _lib.lib().polyhip_aln_records(C.byref(cp) if params else None, n, *[ptr(k, p[k]) for k in INPUTS], ptr("cigar_off", out["cigar_off"]),
                                        ptr("cigar", cigar), ccap, ptr("md_off", out["md_off"]), ptr("md", md), mcap,
                                        *[ptr(k, out[k]) for k in ("nm", "mapq", "sam_flag", "err")])
    return rc, _lib.lib().polyhip_last_error().decode(), out


def test_short_capacity_and_sizes_only():
    from poly_amd import _lib, sam
    want = _want("256", False, True)
    p, n = ari.pack(_set("256")), 256
    nc, nb = int(want.cigar_off[n]), int(want.md_off[n])
    assert nc > n and nb > n
    for ccap, mcap in ((nc - 1, nb), (nc, nb - 1), (0, 0)):
        cigar, md = np.full(nc, 0xDEADBEEF, np.uint32), np.full(nb, 0xAB, np.uint8)
        rc, msg, out = _raw(p, n, 0, 1, cigar, ccap, md, mcap)
        assert rc == _lib.ERR_INVALID and f"{nc} CIGAR entries and {nb} MD bytes" in msg and f"hold {ccap} and {mcap}" in msg
        assert (cigar == 0xDEADBEEF).all() and (md == 0xAB).all()
        for f in ("cigar_off", "md_off", "nm", "mapq", "sam_flag", "err"):
            assert (out[f] == getattr(want, f)).all(), f
        assert sam.last_info() == want.info
    rc, msg, out = _raw(p, n, 0, 1)                                          # NULL, NULL and no capacity: the sizes
    assert rc == _lib.ERR_INVALID and (out["cigar_off"] == want.cigar_off).all() and (out["md_off"] == want.md_off).all()
    assert (out["err"] == want.err).all() and (out["sam_flag"] == want.sam_flag).all()
    cigar, md = np.full(nc + 3, 0xDEADBEEF, np.uint32), np.full(nb + 3, 0xAB, np.uint8)
    rc, _, out = _raw(p, n, 0, 1, cigar, nc, md, nb)                         # exactly what was asked for, and not a byte beyond
    assert rc == _lib.OK and (cigar[:nc] == want.cigar).all() and (md[:nb] == want.md).all()
    assert (cigar[nc:] == 0xDEADBEEF).all() and (md[nb:] == 0xAB).all()
    short = sam.records_packed(**p, paired=True, cigar_capacity=nc - 1)    # the wrapper with a capacity the caller fixed
    assert short.status == _lib.ERR_INVALID and short.cigar is None and int(short.cigar_off[n]) == nc
    _assert_same(sam.records_packed(**p, paired=True, cigar_capacity=nc, md_capacity=nb), want)


def test_records_that_outgrow_the_guess_run_again():
    """sam.records_packed's default capacities are a guess per entry; entries of all-X columns need more MD than that"""
    from poly_amd import sam
    rng = np.random.default_rng(5)
    cs = tuple(ari.case(f"x{i}", "XI" * 1000, rng) for i in range(8))
    p = ari.pack(cs)
    want = aro.records(*[p[k] for k in INPUTS], True, False)
    assert int(want.md_off[8]) > 32 * 8 + 4096 and int(want.cigar_off[8]) > 8 * 8 + 1024
    _assert_same(sam.records_packed(**p, eqx=True), want)


def test_empty_batch():
    from poly_amd import _lib, sam
    p = ari.pack(())
    rc, _, out = _raw(p, 0, null=INPUTS + ("nm", "mapq", "sam_flag", "err"))
    assert rc == _lib.OK and out["cigar_off"][0] == 0 and out["md_off"][0] == 0
    assert sam.last_info() == dict(entries=0, mapped=0, columns=0, cigar_ops=0, md_bytes=0, bad=0)
    got = sam.records_packed(**p, paired=True)
    assert got.status == 0 and len(got.cigar) == 0 and len(got.md) == 0 and list(got.cigar_off) == [0]


def test_argument_errors_in_order():
    from poly_amd import _lib
    cs = ari.batch(255)[:3]
    p = ari.pack(cs)
    every = INPUTS + ("cigar_off", "md_off", "nm", "mapq", "sam_flag", "err")
    down = dict(p, aln_off=p["aln_off"][::-1].copy())
    steps = [                                                   # each call also has everything wrong that a later check looks for
        (dict(params=False, eqx=2, paired=2, null=every), "null params"),
        (dict(eqx=2, paired=2, null=every), "eqx = 2"),
        (dict(eqx=1, paired=2, null=every), "paired = 2"),
        (dict(paired=1, null=every), "paired with 3 entries"),
        (dict(null=("flags",), p=down), "null argument"),
        (dict(null=("md_off",), p=down), "null argument"),
        (dict(ccap=5, p=down), "null output"),
        (dict(p=down), "not ascending"),
    ]
    for kw, text in steps:
        rc, msg, _ = _raw(kw.pop("p", p), 3, **kw)
        assert rc == _lib.ERR_INVALID and text in msg and "polyhip_aln_records" in msg, (text, msg)
    assert _raw(p, 3)[0] == _lib.ERR_INVALID and "the records need" in _raw(p, 3)[1]      # nothing wrong but the capacity


# ---------------------------------------------------------------- 3. end to end: what the mappers return
def _end_to_end(result, T, reads, paired):
    from poly_amd import sam
    n = len(reads)
    read_len = np.array([len(r) for r in reads], np.uint32)
    a, b = b"".join(result.alignA), b"".join(result.alignB)
    seen = dict(ins=0, dele=0, reverse=0, clipped=0)
    for eqx in (False, True):
        got = sam.records(result, read_len, eqx=eqx, paired=paired)
        info = sam.last_info()
        want = aro.records(result.flags, result.score, result.second, result.read_start, result.read_end, read_len, a, b, result.aln_off,
                           eqx, paired)
        _assert_same(got, want)
        live = (got.sam_flag & 4) == 0
        assert (got.err == 0).all() and (live == ((result.flags & 1) == 1)).all() and live.sum() > n // 2
        cols = np.diff(result.aln_off.astype(np.int64))
        assert info == dict(entries=n, mapped=int(live.sum()), columns=int(cols[live].sum()), cigar_ops=len(got.cigar),
                            md_bytes=len(got.md), bad=0)
        assert info["cigar_ops"] == int(np.diff(got.cigar_off.astype(np.int64)).sum())
        for i in np.nonzero(live)[0]:
            q = oracle.reverse_complement(reads[i]) if result.flags[i] & 2 else reads[i]
            cigar = got.cigar[int(got.cigar_off[i]):int(got.cigar_off[i + 1])]
            text, used = aro.rebuild_text(q, cigar, got.md[int(got.md_off[i]):int(got.md_off[i + 1])].tobytes())
            assert text == T[int(result.ref_start[i]):int(result.ref_end[i])] and used == len(reads[i]), i
            ops = {int(x) & 15 for x in cigar}
            seen["ins"] += 1 in ops
            seen["dele"] += 2 in ops
            seen["reverse"] += bool(got.sam_flag[i] & 0x10)
            seen["clipped"] += 4 in ops
    assert all(v > 0 for v in seen.values()), seen
    fh = io.StringIO()
    names = [f"r{i >> 1 if paired else i}" for i in range(n)]
    sam.write(fh, "T", len(T), names, reads, None, result, got, paired=paired)
    tlen = result.tlen if paired else []
    assert fh.getvalue().split("\n")[:-1] == aro.sam_lines("T", len(T), names, reads, None, result.ref_start, result.score, tlen, want, paired)
    return got


def test_end_to_end_affine(nuc4_scoring):
    from poly_amd import bwt, mapper
    d = mai.dataset()
    result = mapper.map_reads_affine_packed(bwt.New(d["T"]), nuc4_scoring, *mai.GAPS[0], *_pack(d["reads"]), _params(mai.PARAMS))
    _end_to_end(result, d["T"], d["reads"], False)


def test_end_to_end_pairs(nuc4_scoring):
    from poly_amd import bwt, mapper
    d = mpi.dataset()
    PP = mapper.PairParams(mpi.PAIR.min_insert, mpi.PAIR.max_insert, mpi.PAIR.rescue)
    result = mapper.map_pairs_packed(bwt.New(d["T"]), nuc4_scoring, *mpi.GAPS[0], *_pack(d["reads1"]), *_pack(d["reads2"]),
                                     _params(mpi.PARAMS), PP, max_len=mpi.MAX_LEN)
    reads = [r for pair in zip(d["reads1"], d["reads2"]) for r in pair]
    got = _end_to_end(result, d["T"], reads, True)
    proper = (result.flags & 4) != 0
    assert ((got.sam_flag & 2) != 0).tolist() == proper.tolist() and proper.sum() > 100
    assert ((got.sam_flag & 0x40) != 0).tolist() == [i % 2 == 0 for i in range(len(reads))]
