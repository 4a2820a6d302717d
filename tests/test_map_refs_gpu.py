"""polyhip_refs_*, polyhip_map_reads_refs and polyhip_map_pairs_refs on the GPU against the CPU oracle
(tests/map_refs_oracle.py): every per-entry array with rid, tlen, both aligned strings of every entry and all counters are
compared exactly.  Inputs: tests/map_refs_inputs.py (what they hold is asserted in tests/test_map_refs_cpu.py); with one
contig the calls are compared with the existing oracles' answers on the existing inputs."""
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
import map_pairs_inputs as mpi  # noqa: E402
import map_refs_inputs as ri  # noqa: E402
import map_refs_oracle as mro  # noqa: E402
import pileup_oracle as po  # noqa: E402
from map_check import FIELDS, _assert_equal, _pack, _params, layout, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def _set(contigs):
    from poly_amd import refs
    return refs.New([f"c{i}" for i in range(len(contigs))], list(contigs))


def _pp(PP):
    from poly_amd import mapper
    return mapper.PairParams(PP.min_insert, PP.max_insert, PP.rescue)


def _map(rs, scoring, reads, P=ri.P, go=ri.GO, ge=ri.GE, **kw):
    from poly_amd import mapper
    return mapper.map_reads_refs_packed(rs, scoring, go, ge, *_pack(list(reads)), _params(P), **kw)


def _map_pairs(rs, scoring, reads1, reads2, P=ri.PP, PP=ri.PAIR, go=ri.GO, ge=ri.GE, **kw):
    from poly_amd import mapper
    return mapper.map_pairs_refs_packed(rs, scoring, go, ge, *_pack(list(reads1)), *_pack(list(reads2)), _params(P), _pp(PP), **kw)


def _assert_hits(got, hits, strings=True):
    _assert_equal(got, hits, strings)
    want = np.array([getattr(h, "rid", 0) for h in hits], np.int64)
    bad = np.nonzero(np.asarray(got.rid).astype(np.int64) != want)[0]
    assert bad.size == 0, f"rid: {bad.size} entries differ, first {bad[0]}: got {got.rid[bad[0]]}, want {want[bad[0]]}"


def _assert_pairs(got, results, strings=True):
    hits, tlen = ri.flat(results)
    assert len(got.score) == len(hits) == 2 * len(got.tlen)
    _assert_hits(got, hits, strings)
    assert [int(x) for x in got.tlen] == tlen


def _assert_info(info, ncontigs, pairs=False):
    from poly_amd import mapper
    got = mapper.last_pairs_info() if pairs else mapper.last_affine_info()
    keys = mro.PAIR_COUNTERS if pairs else mro.COUNTERS
    assert {k: got[k] for k in keys} == {k: info[k] for k in keys}
    assert got["pairs_traced"] == got["reads_mapped"]
    refs_info = mapper.last_refs_info()
    assert refs_info == dict(contigs=ncontigs, straddling=info.get("straddling", 0))
    return got


def _chunk_bytes(call, n, unit):
    """what one chunk needs, as the error of a limit that is too small states it"""
    from poly_amd import _lib
    with pytest.raises(_lib.PolyhipError) as ei:
        call(work_limit=1)
    assert ei.value.status == _lib.ERR_INVALID
    m = re.search(rf"a chunk of (\d+) {unit} \((\d+) bytes\)", ei.value.message)
    assert m and int(m.group(1)) == n
    return int(m.group(2))


# ---------------------------------------------------------------- 1. one contig is the single-text call
@pytest.mark.parametrize("gaps", mai.GAPS, ids=lambda g: f"{g[0]}_{g[1]}")
def test_one_contig_is_map_reads_affine(gaps, nuc4_scoring):
    d = mai.dataset()
    hits, info = mai.expected(*gaps)
    got = _map(_set([d["T"]]), nuc4_scoring, d["reads"], mai.PARAMS, *gaps)
    _assert_hits(got, hits)
    _assert_info(info, 1)
    assert not got.rid.any() and got.flags.any()


def test_one_contig_with_equal_gaps_is_map_reads(nuc4_scoring):
    d = mai.dataset()
    hits, info = mai.expected_linear(-2)
    got = _map(_set([d["T"]]), nuc4_scoring, d["reads"], mai.PARAMS, -2, -2)
    _assert_hits(got, hits)
    _assert_info(info, 1)


@pytest.mark.parametrize("gaps", mpi.GAPS, ids=lambda g: f"{g[0]}_{g[1]}")
def test_one_contig_is_map_pairs(gaps, nuc4_scoring):
    d = mpi.dataset()
    res, info = mpi.expected(*gaps)
    got = _map_pairs(_set([d["T"]]), nuc4_scoring, d["reads1"], d["reads2"], mpi.PARAMS, mpi.PAIR, *gaps, max_len=mpi.MAX_LEN)
    _assert_pairs(got, res)
    _assert_info(info, 1, pairs=True)
    assert not got.rid.any() and (got.flags & 8).any()


# ---------------------------------------------------------------- 2, 4, 5, 6, 8, 9: the hand-made sets, on both layouts
@pytest.mark.parametrize("name", list(ri.SINGLE))
def test_cases(layout, name, nuc4_scoring):
    case = ri.SINGLE[name]()
    hits, info = ri.expected(name)
    rs = _set(case.contigs)
    assert rs.index.Layout() == ("general" if layout == "general" or name == "with_n" else "nucleotide")
    got = _map(rs, nuc4_scoring, case.reads, case.P)
    for i, h in enumerate(hits):            # name the read that differs
        assert [int(getattr(got, f)[i]) for f in FIELDS + ["rid"]] == [getattr(h, f) for f in FIELDS + ["rid"]], (name, i)
    _assert_hits(got, hits)
    _assert_info(info, len(case.contigs))
    if name == "straddle":
        assert info["straddling"] >= 1 and got.read_end[0] - got.read_start[0] == 15
    if name == "overhang":
        assert got.read_start[0] == 10 and got.read_end[1] == 30
    if name == "with_n":
        assert got.err[1] != 0 and got.flags[1] == 0


def test_duplicates_have_mapq_zero(nuc4_scoring):
    from poly_amd import sam
    case = ri.duplicates()
    got = _map(_set(case.contigs), nuc4_scoring, case.reads)
    assert list(got.rid) == [2, 2] and (got.second == got.score).all() and got.score[0] == 300
    rec = sam.records(got, [len(r) for r in case.reads])
    assert list(rec.mapq) == [0, 0]


# ---------------------------------------------------------------- 3. max_occ is judged on the count in C
def test_max_occ_counts_straddlers(nuc4_scoring):
    from poly_amd import mapper
    over = []
    for k, case in enumerate(ri.max_occ_pair()):
        hits, info = ri.expected(f"max_occ{k}")
        got = _map(_set(case.contigs), nuc4_scoring, case.reads, case.P)
        _assert_hits(got, hits)
        _assert_info(info, len(case.contigs))
        over.append(mapper.last_affine_info()["seeds_over_max_occ"])
    assert over == [1, 0]


# ---------------------------------------------------------------- 7. many contigs
@pytest.fixture(scope="module")
def many_set():
    return _set(ri.many().contigs)


@pytest.mark.parametrize("max_cand", [1, 4, 64])
def test_many_contigs(many_set, nuc4_scoring, max_cand):
    case = ri.many()
    hits, info = ri.expected("many", max_cand)
    got = _map(many_set, nuc4_scoring, case.reads, dataclasses.replace(case.P, max_cand=max_cand))
    _assert_hits(got, hits)
    _assert_info(info, 300)
    assert {0, 299} <= set(int(x) for x in got.rid)


# ---------------------------------------------------------------- 10. chunks
def test_chunks_of_reads(many_set, nuc4_scoring):
    case = ri.many()
    reads = list(case.reads) * 3
    hits, info = ri.expected("many")
    need = _chunk_bytes(lambda **kw: _map(many_set, nuc4_scoring, reads, **kw), 256, "reads")
    got = _map(many_set, nuc4_scoring, reads, work_limit=need)
    _assert_hits(got, hits * 3)
    assert _assert_info({k: 3 * v for k, v in info.items()}, 300)["chunks"] == 3
    whole = _map(many_set, nuc4_scoring, reads)
    assert _assert_info({k: 3 * v for k, v in info.items()}, 300)["chunks"] == 1
    for f in FIELDS + ["rid", "aln_off"]:
        assert (getattr(got, f) == getattr(whole, f)).all(), f
    assert got.alignA == whole.alignA and got.alignB == whole.alignB


def test_chunks_of_pairs(nuc4_scoring):
    case = ri.many_pairs()
    res, info = ri.many_pairs_expected()
    rs = _set(case.contigs)
    need = _chunk_bytes(lambda **kw: _map_pairs(rs, nuc4_scoring, case.reads, case.reads2, **kw), 128, "pairs")
    got = _map_pairs(rs, nuc4_scoring, case.reads, case.reads2, work_limit=need)
    _assert_pairs(got, res)
    got_info = _assert_info(info, 6, pairs=True)
    assert got_info["chunks"] == 3 and got_info["rescued"] > 10
    whole = _map_pairs(rs, nuc4_scoring, case.reads, case.reads2)
    assert _assert_info(info, 6, pairs=True)["chunks"] == 1
    for f in FIELDS + ["rid", "aln_off", "tlen"]:
        assert (getattr(got, f) == getattr(whole, f)).all(), f
    assert got.alignA == whole.alignA and got.alignB == whole.alignB


# ---------------------------------------------------------------- 11. string capacity
def test_short_string_capacity(many_set, nuc4_scoring):
    from poly_amd import _lib
    case = ri.many()
    hits, _ = ri.expected("many")
    need = sum(len(h.alignA) for h in hits)
    got = _map(many_set, nuc4_scoring, case.reads, capacity=need - 1)
    assert got.status == _lib.ERR_INVALID and got.alignA is None and int(got.aln_off[-1]) == need
    _assert_hits(got, hits, strings=False)
    assert got.rid.any()
    exact = _map(many_set, nuc4_scoring, case.reads, capacity=need)
    assert exact.status == _lib.OK
    _assert_hits(exact, hits)


# ---------------------------------------------------------------- 12, 13, 14: pairs
@pytest.mark.parametrize("name", list(ri.PAIRED))
def test_pairs(name, nuc4_scoring):
    case = ri.PAIRED[name]()
    res, info = ri.expected_pairs(name)
    got = _map_pairs(_set(case.contigs), nuc4_scoring, case.reads, case.reads2, case.P)
    _assert_pairs(got, res)
    _assert_info(info, len(case.contigs), pairs=True)
    if name == "adjacent_pair":
        assert list(got.flags) == [1, 3] and list(got.rid) == [0, 1] and got.tlen[0] == 0
    if name == "rescue_clip":
        assert list(got.flags) == [1, 0] and got.tlen[0] == 0
    if name == "rescue_inside":
        assert list(got.flags) == [5, 15, 13, 7, 5, 7, 5, 7] and list(got.rid) == [3, 3, 3, 3, 2, 2, 1, 1]


# ---------------------------------------------------------------- 15, 16: the handle
def test_index_and_resolve():
    contigs = (b"ACGTACGTAC", b"G", b"TTGACCA", b"ACGTAGG")
    rs = _set(contigs)
    C_ = ri.join(contigs)
    st = [0, 10, 11, 18, 25]
    assert len(rs) == 4 and list(rs.starts) == st and list(rs.lengths) == [10, 1, 7, 7] and rs.text() == C_
    assert rs.index.Len() == 25 and rs.index.Count(b"ACGTA") == 3 and sorted(rs.index.Locate(b"ACGTA")) == [0, 4, 18]
    assert rs.index.Count(b"ACGT") == 4 and rs.index.Count(b"CGTT") == 1          # one "ACGT" and the "CGTT" lie across contigs
    # every contig's first and last position, the last of C, and one past it
    pos = [st[c] for c in range(4)] + [st[c + 1] - 1 for c in range(4)] + [24, 25, 0xFFFFFFFF]
    rid, local, err = rs.resolve(pos)
    assert list(rid) == [0, 1, 2, 3, 0, 1, 2, 3, 3, 0, 0]
    assert list(local) == [0, 0, 0, 0, 9, 0, 6, 6, 6, 0, 0]
    assert list(err) == [0] * 9 + [1, 1]
    # spans that end exactly at a contig's end, and one past it
    rid, local, err = rs.resolve([5, 5, 10, 10, 11, 11, 18, 18, 9], [5, 6, 1, 2, 7, 8, 7, 8, 4])
    assert list(err) == [0, 2, 0, 2, 0, 2, 0, 2, 2] and list(rid) == [0, 0, 1, 1, 2, 2, 3, 3, 0] and local[8] == 9
    rid, local, err = rs.resolve(np.array([4, 18, 0], np.uint32), 5)              # where "ACGTA" was located
    assert list(zip(rid, local, err)) == [(0, 4, 0), (3, 0, 0), (0, 0, 0)]
    assert all(len(a) == 0 for a in rs.resolve([]))


def test_create_errors_and_destroy_order():
    from poly_amd import _lib, refs
    for seqs, word in (([], "at least one contig"), ([b"ACGT", b"", b"AC"], "contig 1 is empty"), ([b"ACGT", b"A$C"], "nullChar")):
        with pytest.raises(_lib.PolyhipError) as ei:
            refs.New([str(i) for i in range(len(seqs))], seqs)
        assert ei.value.status == _lib.ERR_INVALID and word in ei.value.message
    with pytest.raises(ValueError):
        refs.New(["a"], [b"ACGT", b"AC"])
    rs = refs.New(["a", "b"], ["ACGTAC", "GGT"])
    idx = rs.index
    del rs                                   # the view keeps the set alive
    assert idx.Count("ACG") == 2 and idx.Count("CGG") == 1 and idx.Extract(4, 8) == "ACGG"
    rs = refs.from_fasta(b">one first\nACGT\nAC\n>two\nGGT\n")
    assert rs.names == ["one", "two"] and list(rs.lengths) == [6, 3] and rs.text() == b"ACGTACGGT"


# ---------------------------------------------------------------- 17. pileup of one contig
def test_pileup_refs(many_set, nuc4_scoring):
    from poly_amd import pileup
    case = ri.many()
    got = _map(many_set, nuc4_scoring, case.reads)
    for c in (2, ri.MANY_REPEAT[0], 299):
        keep = [i for i in range(len(case.reads)) if got.rid[i] == c]
        a, b = b"".join(got.alignA[i] for i in keep), b"".join(got.alignB[i] for i in keep)
        off = np.concatenate([[0], np.cumsum([len(got.alignA[i]) for i in keep])]).astype(np.int64)
        want = po.pileup(got.flags[keep], None, got.ref_start[keep], got.ref_end[keep], a, b, off, case.contigs[c], min_depth=1,
                         min_alt_count=1)
        have = pileup.pileup_refs(got, many_set, c)
        assert (have.counts == want.counts).all() and (have.consensus == want.consensus).all()
        assert [tuple(int(x) for x in s) for s in have.sites.tolist()] == want.site_list()
        assert have.region_lo == 0 and not have.err.any() and have.last_info()["used"] == want.info["used"]
    assert any(got.rid[i] == ri.MANY_REPEAT[0] and got.flags[i] & 1 for i in range(len(case.reads)))
    part = pileup.pileup_refs(got, many_set, ri.MANY_REPEAT[0], region=(10, 40))
    whole = pileup.pileup_refs(got, many_set, ri.MANY_REPEAT[0])
    assert part.region_lo == 10 and (part.counts == whole.counts[:, 10:40]).all() and whole.depth().any()
