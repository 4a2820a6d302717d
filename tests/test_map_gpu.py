"""The read mapper on the GPU against its CPU oracle (tests/map_oracle.py): every output array and both aligned strings of
every read, and the info counters, are compared exactly -- no exclusions.  Inputs: tests/map_inputs.py (their coverage of
every class of read is asserted in tests/test_map_cpu.py)."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_inputs as mi  # noqa: E402
import map_oracle as mo  # noqa: E402
import oracle  # noqa: E402
from map_check import _Dev, _assert_equal, _assert_info, _pack, _params, layout, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(HERE, "golden", "bwt", "reference_tables.json")))


def _map(index, scoring, reads, P, **kw):
    from poly_amd import mapper
    buf, offs = _pack(reads)
    return mapper.map_reads_packed(index, scoring, buf, offs, _params(P), **kw)


# ---------------------------------------------------------------- parity on the shared inputs
@pytest.mark.parametrize("which", ["a", "b"])
def test_parity(layout, which, nuc4_scoring):
    from poly_amd import bwt
    d = mi.dataset()
    hits, info = mi.expected(which)
    index = bwt.New(d["T"])
    assert index.Layout() == ("nucleotide" if layout == "auto" else "general")
    got = _map(index, nuc4_scoring, d["reads"], mi.PARAMS_A if which == "a" else mi.PARAMS_B)
    _assert_equal(got, hits)
    assert _assert_info(info)["chunks"] == 1


def test_device_flavour_and_chunks(nuc4_scoring):
    """the device flavour with the whole workspace, and with about a third of it: three chunks or more, the same outputs"""
    from poly_amd import bwt
    d = mi.dataset()
    hits, info = mi.expected("a")
    index = bwt.New(d["T"])
    whole = _Dev(index, nuc4_scoring, d["reads"], mi.PARAMS_A)
    _assert_equal(whole, hits)
    assert _assert_info(info)["chunks"] == 1
    third = _Dev(index, nuc4_scoring, d["reads"], mi.PARAMS_A, work_bytes=lambda full: int(full * 0.34))
    _assert_equal(third, hits)
    assert _assert_info(info)["chunks"] >= 3
    assert (third.aln_off == whole.aln_off).all()
    # less than one chunk of 256 reads needs: refused
    from poly_amd import _lib
    with pytest.raises(_lib.PolyhipError) as ei:
        _Dev(index, nuc4_scoring, d["reads"], mi.PARAMS_A, work_bytes=lambda full: full // 8)
    assert ei.value.status == _lib.ERR_INVALID and "workspace" in ei.value.message


def test_string_capacity(nuc4_scoring):
    from poly_amd import _lib, bwt
    d = mi.dataset()
    hits, _ = mi.expected("a")
    index = bwt.New(d["T"])
    needed = sum(len(h.alignA) for h in hits)
    for run in (lambda cap: _map(index, nuc4_scoring, d["reads"], mi.PARAMS_A, capacity=cap),
                lambda cap: _Dev(index, nuc4_scoring, d["reads"], mi.PARAMS_A, capacity=cap)):
        exact = run(needed)
        assert exact.status == 0
        _assert_equal(exact, hits)
        short = run(needed - 1)
        assert short.status == _lib.ERR_INVALID and int(short.aln_off[-1]) == needed
        _assert_equal(short, hits, strings=False)
        want_off = np.concatenate([[0], np.cumsum([len(h.alignA) for h in hits])])
        assert (np.asarray(short.aln_off).astype(np.int64) == want_off).all()
    for without in (_map(index, nuc4_scoring, d["reads"], mi.PARAMS_A, strings=False),
                    _Dev(index, nuc4_scoring, d["reads"], mi.PARAMS_A, strings=False)):
        assert without.status == 0 and without.alignA is None
        _assert_equal(without, hits, strings=False)


# ---------------------------------------------------------------- a general-alphabet text
def test_general_alphabet():
    """the reference's pangram (upper-cased: matrix.Default scores A..Z), repeated, forward only: every seed of a read has one
    occurrence per copy, so each read has a candidate in every copy and the rank decides"""
    from poly_amd import align, bwt
    T = (GOLD["pangram_base"] * GOLD["pangram_repeat"]).upper().encode()
    rng = np.random.default_rng(11)
    reads = []
    for _ in range(40):
        m = int(rng.integers(30, 61))
        at = int(rng.integers(0, len(T) - m + 1))
        r = bytearray(T[at:at + m])
        for pos in rng.integers(0, m, 3):
            r[pos] = int(rng.integers(ord("A"), ord("Z") + 1))
        reads.append(bytes(r))
    P = mo.Params(seed_len=8, seed_stride=4, max_occ=8, band=8, max_cand=4, both_strands=False, min_score=1)
    hits, info = mo.map_reads(T, reads, oracle.DEFAULT_MATRIX, -1, P)
    assert sum(h.flags & 1 for h in hits) >= 30 and any(len(h.cands) > 1 for h in hits)
    index = bwt.New(T)
    assert index.Layout() == "general"
    _assert_equal(_map(index, align.NewScoring(None, -1), reads, P), hits)
    _assert_info(info)


# ---------------------------------------------------------------- long reads: the one-wave-per-pair alignment path
def test_long_reads(nuc4_scoring):
    from poly_amd import align, bwt
    rng = np.random.default_rng(12)
    T = mi.dna(rng, 50_000)
    reads = []
    for i, m in enumerate([1000] * 20 + [4096] * 5):
        at = int(rng.integers(0, len(T) - m + 1))
        r = mi.mutate(rng, T[at:at + m])[:m]
        reads.append(oracle.reverse_complement(r) if i % 2 else r)
    P = dataclasses.replace(mi.PARAMS_A, band=64)
    hits, info = mo.map_reads(T, reads, mi.nuc4(), mi.GAP, P)
    assert all(h.flags & 1 for h in hits) and max(len(r) for r in reads) > 4000
    index = bwt.New(T)
    _assert_equal(_map(index, nuc4_scoring, reads, P), hits)
    _assert_info(info)
    assert align.last_path() == 6 and align.sw_traceback_last_path() == 4  # one wave per pair, score pass and traceback


# ---------------------------------------------------------------- edges
def test_edges(nuc4_scoring):
    from poly_amd import bwt, mapper
    d = mi.dataset()
    T, P = d["T"], mi.PARAMS_A
    index = bwt.New(T)
    mat = mi.nuc4()
    # no reads
    got = _map(index, nuc4_scoring, [], P)
    assert got.status == 0 and len(got.score) == 0 and got.alignA == [] and int(got.aln_off[0]) == 0
    assert mapper.last_info() == dict(seeds=0, seeds_over_max_occ=0, hits=0, clusters=0, pairs_aligned=0, reads_mapped=0, chunks=0)
    assert _Dev(index, nuc4_scoring, [], P).status == 0
    # every read shorter than a seed: no seeds, nothing aligned (the longest read is shorter than seed_len as well)
    short = [T[100:100 + k] for k in (1, 7, 15, 15)]
    hits, info = mo.map_reads(T, short, mat, mi.GAP, P)
    _assert_equal(_map(index, nuc4_scoring, short, P), hits)
    assert _assert_info(info)["seeds"] == 0
    _assert_equal(_Dev(index, nuc4_scoring, short, P), hits)
    # ... and among reads that have seeds
    mixed = [T[100:110], T[300:420], b"", T[700:715]]
    hits, info = mo.map_reads(T, mixed, mat, mi.GAP, P)
    assert [h.flags for h in hits] == [0, 1, 0, 0]
    _assert_equal(_map(index, nuc4_scoring, mixed, P), hits)
    _assert_info(info)
    # one read
    one = [d["reads"][d["special"]["tie_rev"]]]
    hits, info = mo.map_reads(T, one, mat, mi.GAP, P)
    _assert_equal(_map(index, nuc4_scoring, one, P), hits)
    _assert_info(info)
    # max_cand = 1: the tied reads keep one candidate, second = 0
    P1 = dataclasses.replace(P, max_cand=1)
    some = d["reads"][:40] + d["reads"][650:]
    hits, info = mo.map_reads(T, some, mat, mi.GAP, P1)
    assert hits[-4].second == 0 and hits[-4].score == 750
    _assert_equal(_map(index, nuc4_scoring, some, P1), hits)
    _assert_info(info)
    # MapReads: records, str in -> str out
    rec = mapper.MapReads(index, nuc4_scoring, [r.decode() for r in some[:3]], _params(P1))
    assert [(x.mapped, x.reverse, x.score, x.ref_start, x.alignA) for x in rec] == \
        [(bool(h.flags & 1), bool(h.flags & 2), h.score, h.ref_start, h.alignA.decode()) for h in hits[:3]]


def test_every_seed_over_max_occ(layout, nuc4_scoring):
    from poly_amd import bwt
    T = b"ACGT" * 500
    reads = [T[1:121], T[2:152], oracle.reverse_complement(T[3:103])]
    hits, info = mo.map_reads(T, reads, mi.nuc4(), mi.GAP, mi.PARAMS_A)
    assert info["seeds"] == info["seeds_over_max_occ"] > 0 and info["hits"] == 0
    _assert_equal(_map(bwt.New(T), nuc4_scoring, reads, mi.PARAMS_A), hits)
    _assert_info(info)
