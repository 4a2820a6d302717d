"""polyhip_map_pairs on the GPU against its CPU oracle (tests/map_pairs_oracle.py): every per-mate array, tlen, both aligned
strings of every mate and all counters are compared exactly.  Inputs: tests/map_pairs_inputs.py (what they hold is asserted
in tests/test_map_pairs_cpu.py)."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_pairs_inputs as mpi  # noqa: E402
import map_pairs_oracle as mpo  # noqa: E402
from map_check import FIELDS, _assert_equal, _pack, _params, layout, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def _pp(PP):
    from poly_amd import mapper
    return mapper.PairParams(PP.min_insert, PP.max_insert, PP.rescue)


def _map(index, scoring, reads1, reads2, go, ge, P=mpi.PARAMS, PP=mpi.PAIR, max_len=mpi.MAX_LEN, **kw):
    from poly_amd import mapper
    return mapper.map_pairs_packed(index, scoring, go, ge, *_pack(reads1), *_pack(reads2), _params(P), _pp(PP), max_len=max_len, **kw)


def _assert_pairs(got, results, strings=True):
    hits, tlen = mpi.flat(results)
    assert len(got.score) == len(hits) == 2 * len(got.tlen)
    _assert_equal(got, hits, strings)
    bad = np.nonzero(np.asarray(got.tlen) != np.array(tlen, np.int64))[0]
    assert bad.size == 0, f"tlen: {bad.size} pairs differ, first {bad[0]}: got {got.tlen[bad[0]]}, want {tlen[bad[0]]}"


def _assert_info(info):
    """every counter equals the oracle's, and every mapped mate was traced, no other"""
    from poly_amd import mapper
    got = mapper.last_pairs_info()
    assert {k: got[k] for k in mpo.COUNTERS} == {k: info[k] for k in mpo.COUNTERS}
    assert got["pairs_traced"] == got["reads_mapped"]
    return got


def _chunk_bytes(index, scoring, reads1, reads2, go, ge):
    """what one chunk of min(npairs, 128) pairs needs, as the error of a limit that is too small states it"""
    from poly_amd import _lib
    with pytest.raises(_lib.PolyhipError) as ei:
        _map(index, scoring, reads1, reads2, go, ge, work_limit=1)
    assert ei.value.status == _lib.ERR_INVALID
    m = re.search(r"a chunk of (\d+) pairs \((\d+) bytes\)", ei.value.message)
    assert m and int(m.group(1)) == min(len(reads1), 128)
    return int(m.group(2))


@pytest.fixture(scope="module")
def index():
    from poly_amd import bwt
    return bwt.New(mpi.dataset()["T"])


# ---------------------------------------------------------------- 1. parity with the oracle
@pytest.mark.parametrize("gaps", mpi.GAPS, ids=lambda g: f"{g[0]}_{g[1]}")
def test_parity(layout, gaps, nuc4_scoring):
    from poly_amd import bwt
    d = mpi.dataset()
    res, info = mpi.expected(*gaps)
    idx = bwt.New(d["T"])
    assert idx.Layout() == ("nucleotide" if layout == "auto" else "general")
    got = _map(idx, nuc4_scoring, d["reads1"], d["reads2"], *gaps)
    _assert_pairs(got, res)
    got_info = _assert_info(info)
    assert got_info["chunks"] == 1 and got_info["rescued"] > 20 and got_info["proper_pairs"] > got_info["rescued"]


def test_parity_without_rescue(index, nuc4_scoring):
    d = mpi.dataset()
    go, ge = mpi.GAPS[0]
    res, info = mpi.expected(go, ge, False)
    got = _map(index, nuc4_scoring, d["reads1"], d["reads2"], go, ge, PP=dataclasses.replace(mpi.PAIR, rescue=False))
    _assert_pairs(got, res)
    got_info = _assert_info(info)
    assert got_info["rescue_attempts"] == 0 and got_info["rescued"] == 0 and not (got.flags & 8).any()


# ---------------------------------------------------------------- 2. without pairing it is the single-read mapper
def test_no_pairing_is_map_reads_affine(index, nuc4_scoring):
    from poly_amd import mapper
    d = mpi.dataset()
    never = mpo.PairParams(0xFFFFFFFF, 0xFFFFFFFF, False)
    inter = [r for pair in zip(d["reads1"], d["reads2"]) for r in pair]
    for go, ge in mpi.GAPS:
        got = _map(index, nuc4_scoring, d["reads1"], d["reads2"], go, ge, PP=never)
        have = mapper.last_pairs_info()
        one = mapper.map_reads_affine_packed(index, nuc4_scoring, go, ge, *_pack(inter), _params(mpi.PARAMS), max_len=mpi.MAX_LEN)
        want = mapper.last_affine_info()
        for f in FIELDS + ["aln_off"]:
            assert (getattr(got, f) == getattr(one, f)).all(), (go, ge, f)
        assert got.alignA == one.alignA and got.alignB == one.alignB
        assert not (got.flags & 12).any() and not got.tlen.any() and got.flags.any()
        for k in ("seeds", "seeds_over_max_occ", "hits", "clusters", "pairs_aligned", "reads_mapped", "pairs_traced"):
            assert have[k] == want[k], k
        assert have["proper_pairs"] == have["rescue_attempts"] == have["rescued"] == 0


# ---------------------------------------------------------------- 3. the named pairs
@pytest.mark.parametrize("max_cand", [1, 4, 9])
def test_named_pairs(index, nuc4_scoring, max_cand):
    r1, r2, names = mpi.named_pairs()
    byname, res, info = mpi.expected_named(max_cand)
    got = _map(index, nuc4_scoring, r1, r2, *mpi.GAPS[0], P=mpi.PARAMS_BY_CAND[max_cand])
    for i, name in enumerate(names):       # name the pair that differs
        for f in FIELDS:
            want = [getattr(h, f) for h in (res[i].h1, res[i].h2)]
            assert [int(x) for x in getattr(got, f)[2 * i:2 * i + 2]] == want, (name, f)
        assert int(got.tlen[i]) == res[i].tlen, name
    _assert_pairs(got, res)
    _assert_info(info)
    if max_cand == 9:
        k = names.index("combos81")
        assert byname["combos81"].combos == 81 and got.flags[2 * k] == 5 and got.flags[2 * k + 1] == 7 and got.tlen[k] == 355


# ---------------------------------------------------------------- 4. chunks of pairs, traceback sub-chunks
def test_chunks_of_pairs(index, nuc4_scoring):
    from poly_amd import _lib
    r1, r2 = mpi.many_pairs()
    go, ge = mpi.GAPS[0]
    res, info = mpi.many_expected(go, ge)
    assert len(r1) >= 257
    need = _chunk_bytes(index, nuc4_scoring, r1, r2, go, ge)
    got = _map(index, nuc4_scoring, r1, r2, go, ge, work_limit=need)
    _assert_pairs(got, res)
    assert _assert_info(info)["chunks"] == 3
    whole = _map(index, nuc4_scoring, r1, r2, go, ge)
    assert _assert_info(info)["chunks"] == 1
    for f in FIELDS + ["aln_off", "tlen"]:
        assert (getattr(got, f) == getattr(whole, f)).all(), f
    assert got.alignA == whole.alignA and got.alignB == whole.alignB
    with pytest.raises(_lib.PolyhipError) as ei:
        _map(index, nuc4_scoring, r1, r2, go, ge, work_limit=need - 1)
    assert ei.value.status == _lib.ERR_INVALID and "workspace" in ei.value.message


def test_traceback_sub_chunks(index, nuc4_scoring, monkeypatch):
    d = mpi.dataset()
    go, ge = mpi.GAPS[1]
    res, info = mpi.expected(go, ge)
    assert info["reads_mapped"] > 3 * 64
    monkeypatch.setenv("POLYHIP_SWA_CHUNK_PAIRS", "64")
    got = _map(index, nuc4_scoring, d["reads1"], d["reads2"], go, ge)
    _assert_pairs(got, res)
    _assert_info(info)
    need = _chunk_bytes(index, nuc4_scoring, d["reads1"], d["reads2"], go, ge)      # ... and inside chunks of pairs
    got = _map(index, nuc4_scoring, d["reads1"], d["reads2"], go, ge, work_limit=need)
    _assert_pairs(got, res)
    assert _assert_info(info)["chunks"] == 2


# ---------------------------------------------------------------- 5. nothing to trace, nothing to rescue
def test_no_winner_and_no_request(index, nuc4_scoring):
    d = mpi.dataset()
    go, ge = mpi.GAPS[0]
    rng = np.random.default_rng(mpi.SEED + 1)
    # no mate is mapped: no anchor, so no request either
    r1 = [mpi.mi.dna(rng, 120) for _ in range(6)] + d["reads1"][:6]
    r2 = [mpi.mi.dna(rng, 110) for _ in range(6)] + d["reads2"][:6]
    P = dataclasses.replace(mpi.PARAMS, min_score=10 ** 6)
    res, info = mpi.run(r1, r2, go, ge, P, mpi.PAIR)
    got = _map(index, nuc4_scoring, r1, r2, go, ge, P=P)
    _assert_pairs(got, res)
    got_info = _assert_info(info)
    assert got_info["reads_mapped"] == got_info["pairs_traced"] == got_info["rescue_attempts"] == 0 and got_info["pairs_aligned"] > 0
    assert got.status == 0 and not got.score.any() and not got.tlen.any() and (got.aln_off == 0).all()
    assert all(s == b"" for s in got.alignA + got.alignB)
    # every pair is proper from its candidates: winners, and no request
    n = d["named"]
    some = [n[k] for k in ("repeat_pairing", "tie_k1k2", "ins_min", "ins_max")]
    r1, r2 = [d["reads1"][i] for i in some], [d["reads2"][i] for i in some]
    res, info = mpi.run(r1, r2, go, ge, mpi.PARAMS, mpi.PAIR)
    got = _map(index, nuc4_scoring, r1, r2, go, ge)
    _assert_pairs(got, res)
    got_info = _assert_info(info)
    assert got_info["rescue_attempts"] == 0 and got_info["proper_pairs"] == 4 and got_info["pairs_traced"] == 8


def test_no_pairs(index, nuc4_scoring):
    from poly_amd import mapper
    got = _map(index, nuc4_scoring, [], [], -5, -2)
    assert got.status == 0 and len(got.score) == 0 and len(got.tlen) == 0 and got.alignA == [] and int(got.aln_off[0]) == 0
    assert mapper.last_pairs_info() == dict.fromkeys(list(mpo.COUNTERS) + ["pairs_traced", "chunks"], 0)
    assert mapper.MapPairs(index, nuc4_scoring, [], [], -5, -2, _pp(mpi.PAIR), _params(mpi.PARAMS)) == []


# ---------------------------------------------------------------- 6. strings
def test_strings(index, nuc4_scoring):
    from poly_amd import _lib
    r1, r2, _ = mpi.named_pairs()
    go, ge = mpi.GAPS[0]
    _, res, info = mpi.expected_named(4)
    hits, _ = mpi.flat(res)
    without = _map(index, nuc4_scoring, r1, r2, go, ge, strings=False)
    assert without.status == 0 and without.alignA is None
    _assert_pairs(without, res, strings=False)
    needed = sum(len(h.alignA) for h in hits)
    exact = _map(index, nuc4_scoring, r1, r2, go, ge, capacity=needed)
    assert exact.status == 0
    _assert_pairs(exact, res)
    short = _map(index, nuc4_scoring, r1, r2, go, ge, capacity=needed - 1)
    assert short.status == _lib.ERR_INVALID and int(short.aln_off[-1]) == needed
    _assert_pairs(short, res, strings=False)
    _assert_info(info)
    want_off = np.concatenate([[0], np.cumsum([len(h.alignA) for h in hits])])
    assert (np.asarray(short.aln_off).astype(np.int64) == want_off).all()


# ---------------------------------------------------------------- 7. errors, in the documented order
def test_errors(index, nuc4_scoring):
    from poly_amd import _lib
    d = mpi.dataset()
    r1, r2 = d["reads1"][:4], d["reads2"][:4]
    one_strand = dataclasses.replace(mpi.PARAMS, both_strands=False)
    backwards = mpo.PairParams(300, 200, True)

    def status(P, PP, go=-5, ge=-2, **kw):
        with pytest.raises(_lib.PolyhipError) as ei:
            _map(index, nuc4_scoring, r1, r2, go, ge, P=P, PP=PP, **kw)
        return ei.value.status, ei.value.message

    # what polyhip_map_reads_affine checks comes first
    st, msg = status(dataclasses.replace(one_strand, max_cand=65), backwards, 1, 0)
    assert st == _lib.ERR_INVALID and "max_cand" in msg
    st, msg = status(dataclasses.replace(one_strand, band=1025), backwards, 1, 0)
    assert st == _lib.ERR_UNSUPPORTED and "band" in msg
    for go, ge in ((-2, -3), (-5, 0), (0, 0)):
        st, msg = status(one_strand, backwards, go, ge)
        assert st == _lib.ERR_UNSUPPORTED and "gap_open" in msg
    # the int32 cells over the rescue window: 2^17 * (150 + 10182) >= 2^30, while the mapping window alone is far below
    wide = mpo.PairParams(0, 10000, True)
    st, msg = status(one_strand, wide, -(1 << 17), -2)
    assert st == _lib.ERR_UNSUPPORTED and "int32" in msg
    res, info = mpi.run(r1, r2, -(1 << 17), -2, mpi.PARAMS, dataclasses.replace(wide, rescue=False))
    _assert_pairs(_map(index, nuc4_scoring, r1, r2, -(1 << 17), -2, PP=dataclasses.replace(wide, rescue=False)), res)
    _assert_info(info)
    # the pair parameters
    st, msg = status(one_strand, backwards)
    assert st == _lib.ERR_INVALID and "both_strands" in msg
    st, msg = status(mpi.PARAMS, dataclasses.replace(backwards, rescue=2))
    assert st == _lib.ERR_INVALID and "min_insert" in msg
    st, msg = status(mpi.PARAMS, mpo.PairParams(0, 8000, 2))
    assert st == _lib.ERR_INVALID and "rescue" in msg
    # the cap on the rescue window: max_insert - min_insert + max_len + 2 * band columns
    cap = 7168
    st, msg = status(mpi.PARAMS, mpo.PairParams(100, 100 + cap - 150 - 32 + 1, True))
    assert st == _lib.ERR_UNSUPPORTED and str(cap) in msg and "rescue window" in msg
    st, msg = status(one_strand, mpo.PairParams(100, 100 + cap, True))
    assert st == _lib.ERR_INVALID and "both_strands" in msg
    at_cap = mpo.PairParams(100, 100 + cap - 150 - 32, True)
    res, info = mpi.run(r1, r2, -12, -2, mpi.PARAMS, at_cap)
    _assert_pairs(_map(index, nuc4_scoring, r1, r2, -12, -2, PP=at_cap), res)
    _assert_info(info)


# ---------------------------------------------------------------- 8. the list interface
def test_map_pairs_on_str_and_bytes(index, nuc4_scoring):
    from poly_amd import mapper
    r1, r2, names = mpi.named_pairs()
    _, res, _ = mpi.expected_named(4)
    keep = [names.index(k) for k in ("repeat_pairing", "rescue_anchor_rev", "discordant", "unrelated")]
    r1, r2, res = [r1[i] for i in keep], [r2[i] for i in keep], [res[i] for i in keep]
    for conv in (lambda b: b, lambda b: b.decode("latin-1")):
        got = mapper.MapPairs(index, nuc4_scoring, [conv(r) for r in r1], [conv(r) for r in r2], *mpi.GAPS[0], _pp(mpi.PAIR),
                              _params(mpi.PARAMS))
        assert len(got) == 4
        for (a, b, proper, tlen), want in zip(got, res):
            assert (proper, tlen) == (want.proper, want.tlen)
            for rec, h in ((a, want.h1), (b, want.h2)):
                assert (rec.mapped, rec.reverse, rec.score, rec.second, rec.votes, rec.ref_start, rec.ref_end, rec.read_start,
                        rec.read_end, rec.err) == (bool(h.flags & 1), bool(h.flags & 2), h.score, h.second, h.votes, h.ref_start,
                                                   h.ref_end, h.read_start, h.read_end, h.err)
                assert (rec.alignA, rec.alignB) == (conv(h.alignA), conv(h.alignB))
    assert mapper.FLAG_PROPER == 4 and mapper.FLAG_RESCUED == 8
