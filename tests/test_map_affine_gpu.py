"""polyhip_map_reads_affine on the GPU against its CPU oracle (tests/map_affine_oracle.py): all nine arrays, both aligned
strings of every read and the six counters the call shares with polyhip_map_reads are compared exactly.  Inputs:
tests/map_affine_inputs.py (what they hold is asserted in tests/test_map_affine_cpu.py)."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_affine_inputs as mai  # noqa: E402
import map_inputs as mi  # noqa: E402
import sw_affine_oracle as ao  # noqa: E402
from map_check import COUNTERS, _assert_equal, _pack, _params, layout, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def _map(index, scoring, reads, P, go, ge, packed=None, **kw):
    from poly_amd import mapper
    buf, offs = _pack(reads) if packed is None else packed
    return mapper.map_reads_affine_packed(index, scoring, go, ge, buf, offs, _params(P), **kw)


def _assert_info(info):
    """the six shared counters equal the oracle's, and every mapped read was traced, no other"""
    from poly_amd import mapper
    got = mapper.last_affine_info()
    assert {k: got[k] for k in COUNTERS} == {k: info[k] for k in COUNTERS}
    assert got["pairs_traced"] == got["reads_mapped"]
    return got


def _chunk_bytes(index, scoring, reads, P, go, ge):
    """what one chunk of min(nreads, 256) reads needs, as the error of a limit that is too small states it"""
    from poly_amd import _lib
    with pytest.raises(_lib.PolyhipError) as ei:
        _map(index, scoring, reads, P, go, ge, work_limit=1)
    assert ei.value.status == _lib.ERR_INVALID
    m = re.search(r"a chunk of (\d+) reads \((\d+) bytes\)", ei.value.message)
    assert m and int(m.group(1)) == min(len(reads), 256)
    return int(m.group(2))


@pytest.fixture(scope="module")
def index():
    from poly_amd import bwt
    return bwt.New(mai.dataset()["T"])


# ---------------------------------------------------------------- 1. parity with the oracle
@pytest.mark.parametrize("gaps", mai.GAPS, ids=lambda g: f"{g[0]}_{g[1]}")
def test_parity(layout, gaps, nuc4_scoring):
    from poly_amd import bwt
    d = mai.dataset()
    hits, info = mai.expected(*gaps)
    idx = bwt.New(d["T"])
    assert idx.Layout() == ("nucleotide" if layout == "auto" else "general")
    got = _map(idx, nuc4_scoring, d["reads"], mai.PARAMS, *gaps)
    _assert_equal(got, hits)
    got_info = _assert_info(info)
    assert got_info["chunks"] == 1 and got_info["tb_chunks"] == 1 and got_info["tb_cells"] > 0


def test_threshold_between_the_linear_and_the_affine_score(index, nuc4_scoring):
    """Z is mapped by polyhip_map_reads (gap -2) and unmapped with gaps (-12, -2) at a min_score between its two scores"""
    from poly_amd import mapper
    d = mai.dataset()
    P, reads = mai.z_params(), mai.z_reads()
    hits, infos = mai.affine_each(d["T"], reads, -12, -2, P)
    got = _map(index, nuc4_scoring, reads, P, -12, -2)
    _assert_equal(got, hits)
    _assert_info(mai.total(infos))
    assert got.flags[0] == 0
    buf, offs = _pack(reads)
    assert mapper.map_reads_packed(index, nuc4_scoring, buf, offs, _params(P)).flags[0] & 1


# ---------------------------------------------------------------- 2. gap_open == gap_extend is the linear mapper
@pytest.mark.parametrize("which", ["a", "b"])
def test_equal_gaps_are_map_reads(which, nuc4_scoring):
    from poly_amd import align, alphabet, bwt, mapper, matrix
    d = mi.dataset()
    P = _params(mi.PARAMS_A if which == "a" else mi.PARAMS_B)
    idx = bwt.New(d["T"])
    buf, offs = _pack(d["reads"])
    a = alphabet.NewAlphabet(list("-ACGT"))
    for g in (-2, -3):
        lin = mapper.map_reads_packed(idx, align.NewScoring(matrix.NewSubstitutionMatrix(a, a, matrix.NUC_4), g), buf, offs, P)
        want = mapper.last_info()
        aff = mapper.map_reads_affine_packed(idx, nuc4_scoring, g, g, buf, offs, P)   # (the handle's own gap is ignored)
        have = mapper.last_affine_info()
        for f in ("score", "second", "flags", "votes", "ref_start", "ref_end", "read_start", "read_end", "err", "aln_off"):
            assert (getattr(lin, f) == getattr(aff, f)).all(), (g, f)
        assert lin.alignA == aff.alignA and lin.alignB == aff.alignB
        assert {k: have[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS} and have["pairs_traced"] == have["reads_mapped"]


# ---------------------------------------------------------------- 3. chunks of reads
def test_chunks_of_reads(index, nuc4_scoring):
    from poly_amd import _lib
    d = mai.dataset()
    go, ge = mai.GAPS[0]
    hits, info = mai.expected(go, ge)
    need = _chunk_bytes(index, nuc4_scoring, d["reads"], mai.PARAMS, go, ge)
    got = _map(index, nuc4_scoring, d["reads"], mai.PARAMS, go, ge, work_limit=need)
    _assert_equal(got, hits)
    assert _assert_info(info)["chunks"] >= 2
    with pytest.raises(_lib.PolyhipError) as ei:
        _map(index, nuc4_scoring, d["reads"], mai.PARAMS, go, ge, work_limit=need - 1)
    assert ei.value.status == _lib.ERR_INVALID and "workspace" in ei.value.message


# ---------------------------------------------------------------- 4. traceback sub-chunks
def test_traceback_sub_chunks(index, nuc4_scoring, monkeypatch):
    d = mai.dataset()
    go, ge = mai.GAPS[1]
    hits, info = mai.expected(go, ge)
    monkeypatch.setenv("POLYHIP_SWA_CHUNK_PAIRS", "64")
    got = _map(index, nuc4_scoring, d["reads"], mai.PARAMS, go, ge)
    _assert_equal(got, hits)
    got_info = _assert_info(info)
    assert got_info["chunks"] == 1 and got_info["tb_chunks"] == -(-info["reads_mapped"] // 64) > 1
    # ... and inside chunks of reads
    need = _chunk_bytes(index, nuc4_scoring, d["reads"], mai.PARAMS, go, ge)
    got = _map(index, nuc4_scoring, d["reads"], mai.PARAMS, go, ge, work_limit=need)
    _assert_equal(got, hits)
    got_info = _assert_info(info)
    assert got_info["chunks"] >= 2 and got_info["tb_chunks"] > got_info["chunks"]


# ---------------------------------------------------------------- 5. no winners
@pytest.mark.parametrize("name", ["short", "unrelated", "below_min_score", "err"])
def test_no_winner(index, name, nuc4_scoring):
    d = mai.dataset()
    reads, P = mai.no_winner_cases()[name]
    for go, ge in mai.GAPS:
        hits, infos = mai.affine_each(d["T"], reads, go, ge, P)
        got = _map(index, nuc4_scoring, reads, P, go, ge)
        _assert_equal(got, hits)
        got_info = _assert_info(mai.total(infos))
        assert got_info["reads_mapped"] == 0 and got_info["tb_chunks"] == 0 and got_info["tb_cells"] == 0
        assert got.status == 0 and not got.score.any() and not got.ref_start.any() and not got.read_start.any()
        assert (got.aln_off == 0).all() and len(got.aln_off) == len(reads) + 1 and all(s == b"" for s in got.alignA + got.alignB)


def test_no_reads(index, nuc4_scoring):
    from poly_amd import mapper
    got = _map(index, nuc4_scoring, [], mai.PARAMS, -5, -2)
    assert got.status == 0 and len(got.score) == 0 and got.alignA == [] and int(got.aln_off[0]) == 0
    assert mapper.last_affine_info() == dict(seeds=0, seeds_over_max_occ=0, hits=0, clusters=0, pairs_aligned=0, reads_mapped=0,
                                             pairs_traced=0, tb_cells=0, chunks=0, tb_chunks=0)
    assert mapper.MapReadsAffine(index, nuc4_scoring, [], -5, -2, _params(mai.PARAMS)) == []


def test_a_whole_chunk_without_a_winner(index, nuc4_scoring):
    go, ge = mai.GAPS[0]
    reads, _ = mai.sandwich()
    hits, info, _ = mai.sandwich_expected(go, ge)
    need = _chunk_bytes(index, nuc4_scoring, reads, mai.PARAMS, go, ge)
    got = _map(index, nuc4_scoring, reads, mai.PARAMS, go, ge, work_limit=need)
    _assert_equal(got, hits)
    got_info = _assert_info(info)
    assert got_info["chunks"] == 3 and got_info["tb_chunks"] == 2    # the middle chunk traced nothing
    assert (got.aln_off[256:513] == got.aln_off[256]).all() and got.aln_off[256] > 0 and got.aln_off[-1] > got.aln_off[512]


# ---------------------------------------------------------------- 6. strings
def test_strings(index, nuc4_scoring):
    from poly_amd import _lib
    d = mai.dataset()
    go, ge = mai.GAPS[0]
    hits, info = mai.expected(go, ge)
    without = _map(index, nuc4_scoring, d["reads"], mai.PARAMS, go, ge, strings=False)
    assert without.status == 0 and without.alignA is None
    _assert_equal(without, hits, strings=False)          # ref_start / read_start come from strings nobody asked for
    _assert_info(info)
    needed = sum(len(h.alignA) for h in hits)
    exact = _map(index, nuc4_scoring, d["reads"], mai.PARAMS, go, ge, capacity=needed)
    assert exact.status == 0
    _assert_equal(exact, hits)
    short = _map(index, nuc4_scoring, d["reads"], mai.PARAMS, go, ge, capacity=needed - 1)
    assert short.status == _lib.ERR_INVALID and int(short.aln_off[-1]) == needed
    _assert_equal(short, hits, strings=False)
    _assert_info(info)
    want_off = np.concatenate([[0], np.cumsum([len(h.alignA) for h in hits])])
    assert (np.asarray(short.aln_off).astype(np.int64) == want_off).all()


# ---------------------------------------------------------------- 7. other shapes
def test_max_len_of_the_caller(index, nuc4_scoring):
    d = mai.dataset()
    go, ge = mai.GAPS[0]
    hits, info = mai.expected(go, ge)
    _assert_equal(_map(index, nuc4_scoring, d["reads"], mai.PARAMS, go, ge, max_len=300), hits)
    _assert_info(info)


def test_offsets_not_starting_at_zero(index, nuc4_scoring):
    d = mai.dataset()
    go, ge = mai.GAPS[1]
    hits, infos = mai.expected_each(go, ge)
    buf, offs = _pack(d["reads"])
    k = 200
    got = _map(index, nuc4_scoring, d["reads"][k:], mai.PARAMS, go, ge, packed=(buf, offs[k:]))
    _assert_equal(got, hits[k:])
    _assert_info(mai.total(infos[k:]))


def test_one_candidate(index, nuc4_scoring):
    """max_cand = 1: X keeps the copy with the insertion whatever the gaps are, second = 0"""
    from poly_amd import mapper
    d = mai.dataset()
    P1 = dataclasses.replace(mai.PARAMS, max_cand=1)
    some = d["reads"][:30] + d["reads"][290:]
    hits, infos = mai.affine_each(d["T"], some, -12, -2, P1)
    x = 30 + d["special"]["X"] - 290
    assert hits[x].second == 0 and hits[x].score == 750 - 12 - 5 * 2 and hits[x].alignA.count(b"-") == 6
    _assert_equal(_map(index, nuc4_scoring, some, P1, -12, -2), hits)
    _assert_info(mai.total(infos))
    rec = mapper.MapReadsAffine(index, nuc4_scoring, [r.decode() for r in some[:3]], -12, -2, _params(P1))
    assert [(r.mapped, r.reverse, r.score, r.ref_start, r.alignA) for r in rec] == \
        [(bool(h.flags & 1), bool(h.flags & 2), h.score, h.ref_start, h.alignA.decode()) for h in hits[:3]]


def test_general_text_and_a_table_in_global_memory():
    from poly_amd import bwt
    g = mai.general_case()
    idx = bwt.New(g["T"])
    assert idx.Layout() == "general"
    got = _map(idx, g["mat"].scoring(), g["reads"], g["P"], g["go"], g["ge"])
    _assert_equal(got, g["hits"])
    _assert_info(g["info"])


# ---------------------------------------------------------------- 8. errors, in the documented order
def test_errors(index, nuc4_scoring):
    from poly_amd import _lib, bwt
    d = mai.dataset()
    reads = d["reads"][:4]

    def status(P, go, ge, scoring=nuc4_scoring, idx=index, **kw):
        with pytest.raises(_lib.PolyhipError) as ei:
            _map(idx, scoring, reads, P, go, ge, **kw)
        return ei.value.status, ei.value.message

    st, msg = status(dataclasses.replace(mai.PARAMS, max_cand=65), 1, 0)          # a bad field wins over a bad gap
    assert st == _lib.ERR_INVALID and "max_cand" in msg
    st, msg = status(dataclasses.replace(mai.PARAMS, band=1025), 1, 0)
    assert st == _lib.ERR_UNSUPPORTED and "band" in msg
    for go, ge in ((-2, -3), (-5, 0), (-5, 1), (0, 0)):
        st, msg = status(mai.PARAMS, go, ge)
        assert st == _lib.ERR_UNSUPPORTED and "gap_open" in msg
    # the int32 cells: |gap_open| * (max_len + (max_len + 3 * band)) reaches 2^30 at max_len = 4072
    big = ao.big_matrix().scoring()
    g = mai.general_case()
    idx = bwt.New(g["T"])
    P = dataclasses.replace(g["P"], band=16)
    with pytest.raises(_lib.PolyhipError) as ei:
        _map(idx, big, g["reads"][:4], P, -(1 << 17), -2, max_len=4072)
    assert ei.value.status == _lib.ERR_UNSUPPORTED and "int32" in ei.value.message
    hits, infos = mai.affine_each(g["T"], g["reads"][:4], -(1 << 17), -2, P, g["mat"])
    _assert_equal(_map(idx, big, g["reads"][:4], P, -(1 << 17), -2, max_len=4071), hits)
    _assert_info(mai.total(infos))
