"""polyhip_map_pairs on the GPU at the pair shapes tests/map_gap_shapes.py builds, against its CPU oracle
(tests/map_pairs_oracle.py): as in tests/test_map_pairs_gpu.py every per-mate array, tlen, both aligned strings of both mates
and all counters are compared exactly, with no exclusions.  That each input reaches the branch it is named for is asserted in
tests/test_map_gap_shapes_cpu.py."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import aln_records_oracle as aro  # noqa: E402
import map_gap_shapes as mg  # noqa: E402
import map_pairs_inputs as mpi  # noqa: E402
import map_pairs_oracle as mpo  # noqa: E402
import oracle  # noqa: E402
from map_check import FIELDS, _assert_equal, _pack, _params, layout, nuc4_scoring  # noqa: E402,F401

pytestmark = pytest.mark.gpu

GO, GE = mg.GAPS[0]
RECORD_ARRAYS = ("cigar_off", "cigar", "md_off", "md", "nm", "mapq", "sam_flag", "err")


def _index(T, layout=None):
    from poly_amd import bwt
    index = bwt.New(T)
    if layout is not None:
        assert index.Layout() == ("nucleotide" if layout == "auto" else "general")
    return index


def _map(index, scoring, s, packed=None, **kw):
    from poly_amd import mapper
    p1, p2 = (_pack(s.reads1), _pack(s.reads2)) if packed is None else packed
    PP = mapper.PairParams(s.PP.min_insert, s.PP.max_insert, s.PP.rescue)
    return mapper.map_pairs_packed(index, scoring, GO, GE, *p1, *p2, _params(s.P), PP, max_len=s.max_len, **kw)


def _assert_pairs(got, results):
    hits, tlen = mpi.flat(results)
    assert got.status == 0 and len(got.score) == len(hits) == 2 * len(got.tlen)
    _assert_equal(got, hits)
    bad = np.nonzero(np.asarray(got.tlen) != np.array(tlen, np.int64))[0]
    assert bad.size == 0, f"tlen: {bad.size} pairs differ, first {bad[0]}: got {got.tlen[bad[0]]}, want {tlen[bad[0]]}"


def _assert_info(info):
    """every counter equals the oracle's, and every mapped mate was traced, no other"""
    from poly_amd import mapper
    got = mapper.last_pairs_info()
    assert {k: got[k] for k in mpo.COUNTERS} == {k: info[k] for k in mpo.COUNTERS}
    assert got["pairs_traced"] == got["reads_mapped"]
    return got


def _same(a, b):
    for f in FIELDS + ["aln_off", "tlen"]:
        assert (getattr(a, f) == getattr(b, f)).all(), f
    assert a.alignA == b.alignA and a.alignB == b.alignB


def _chunk_bytes(index, scoring, s):
    """what one chunk of 128 pairs needs, as the error of a limit that is too small states it"""
    from poly_amd import _lib
    with pytest.raises(_lib.PolyhipError) as ei:
        _map(index, scoring, s, work_limit=1)
    assert ei.value.status == _lib.ERR_INVALID
    m = re.search(r"a chunk of (\d+) pairs \((\d+) bytes\)", ei.value.message)
    assert m and int(m.group(1)) == mg.CHUNK
    return int(m.group(2))


def _records(result, s):
    """the mapper's result through sam.records, against aln_records_oracle.records on the same arrays; the text under every
    live mate comes back from its CIGAR and MD"""
    from poly_amd import sam
    reads = [r for pair in zip(s.reads1, s.reads2) for r in pair]
    read_len = np.array([len(r) for r in reads], np.uint32)
    a, b = b"".join(result.alignA), b"".join(result.alignB)
    for eqx in (False, True):
        got = sam.records(result, read_len, eqx=eqx, paired=True)
        want = aro.records(result.flags, result.score, result.second, result.read_start, result.read_end, read_len, a, b, result.aln_off,
                           eqx, True)
        for f in RECORD_ARRAYS:
            have, need = getattr(got, f), getattr(want, f)
            assert have.dtype == need.dtype and have.shape == need.shape, (f, have.dtype, have.shape, need.shape)
            bad = np.nonzero(have != need)[0]
            assert bad.size == 0, f"{f}: {bad.size} items differ, first {bad[0]}: got {have[bad[0]]}, want {need[bad[0]]}"
        assert sam.last_info() == want.info
        live = (got.sam_flag & 4) == 0
        assert (got.err == 0).all() and (live == ((result.flags & 1) == 1)).all() and live.any()
        for i in np.nonzero(live)[0]:
            q = oracle.reverse_complement(reads[i]) if result.flags[i] & 2 else reads[i]
            cigar = got.cigar[int(got.cigar_off[i]):int(got.cigar_off[i + 1])]
            text, used = aro.rebuild_text(q, cigar, got.md[int(got.md_off[i]):int(got.md_off[i + 1])].tobytes())
            assert text == s.T[int(result.ref_start[i]):int(result.ref_end[i])] and used == len(reads[i]), i
    return got


# ---------------------------------------------------------------- 1. 64 x 64 combinations: late trips, late lanes, late anchors
@pytest.mark.parametrize("max_cand", [64, 63, 5, 1])
def test_many_combinations(layout, max_cand, nuc4_scoring):
    """pair_reduce_kernel's 64 trips over up to 4096 combinations: a winner in the second half of the trips, nc2 that does not
    divide 64, equal sums in different trips and lanes, a rescue anchored on a winner of rank 62"""
    s = mg.pairs_many_combos(max_cand)
    got = _map(_index(s.T, layout), nuc4_scoring, s)
    for i, name in enumerate(s.names):       # name the pair that differs
        for f in FIELDS:
            want = [getattr(h, f) for h in (s.results[i].h1, s.results[i].h2)]
            assert [int(x) for x in getattr(got, f)[2 * i:2 * i + 2]] == want, (name, f)
        assert int(got.tlen[i]) == s.results[i].tlen, name
    _assert_pairs(got, s.results)
    _assert_info(s.info)


def test_many_combinations_without_rescue(nuc4_scoring):
    s = mg.pairs_many_combos(64, False)
    got = _map(_index(s.T), nuc4_scoring, s)
    _assert_pairs(got, s.results)
    have = _assert_info(s.info)
    assert have["rescue_attempts"] == 0 and have["rescued"] == 0 and not (got.flags & 8).any()


# ---------------------------------------------------------------- 2. a chunk without requests, a chunk without winners
@pytest.mark.parametrize("variant", mg.SANDWICHES)
def test_chunks_without_requests_or_winners(variant, nuc4_scoring):
    s = mg.pairs_sandwich(variant)
    index = _index(s.T)
    need = _chunk_bytes(index, nuc4_scoring, s)
    got = _map(index, nuc4_scoring, s, work_limit=need)
    _assert_pairs(got, s.results)
    assert _assert_info(s.info)["chunks"] == 3
    whole = _map(index, nuc4_scoring, s)
    assert _assert_info(s.info)["chunks"] == 1
    _same(got, whole)
    if variant == "empty_middle":
        lo, hi = 2 * mg.CHUNK, 4 * mg.CHUNK      # the middle chunk's mates
        assert (got.aln_off[lo:hi + 1] == got.aln_off[lo]).all() and 0 < got.aln_off[lo] < got.aln_off[-1]
        for f in FIELDS:
            assert not getattr(got, f)[lo:hi].any(), f
        assert not got.tlen[mg.CHUNK:2 * mg.CHUNK].any() and all(x == b"" for x in got.alignA[lo:hi] + got.alignB[lo:hi])


# ---------------------------------------------------------------- 3. off1[0] != off2[0] != 0
def test_offsets_not_starting_at_zero(nuc4_scoring):
    s = mg.pairs_offsets()
    index = _index(s.T)
    (buf1, offs1), (buf2, offs2) = s.note["packed"]
    assert int(offs1[0]) == 37 and int(offs2[0]) == 5
    got = _map(index, nuc4_scoring, s, packed=((buf1, offs1), (buf2, offs2)))
    assert int(got.aln_off[0]) == 0
    _assert_pairs(got, s.results)
    _assert_info(s.info)
    _same(got, _map(index, nuc4_scoring, s))


# ---------------------------------------------------------------- 4. the rescue's complement table
def test_rescue_of_lower_case_and_iupac_mates():
    s = mg.pairs_alphabet()
    index = _index(s.T)
    assert index.Layout() == "general"
    got = _map(index, s.mat.scoring(), s)
    _assert_pairs(got, s.results)
    _assert_info(s.info)
    _records(got, s)


# ---------------------------------------------------------------- 5. a text shorter than the rescue window
def test_text_shorter_than_the_rescue_window(layout, nuc4_scoring):
    s = mg.pairs_short_text()
    got = _map(_index(s.T, layout), nuc4_scoring, s)
    _assert_pairs(got, s.results)
    _assert_info(s.info)
    _records(got, s)


# ---------------------------------------------------------------- 6. an alphabet error at rank 3
def test_error_of_the_text_at_rank_3(nuc4_scoring):
    s = mg.pairs_rank3_error()
    index = _index(s.T)
    assert index.Layout() == "general"
    got = _map(index, nuc4_scoring, s)
    _assert_pairs(got, s.results)
    _assert_info(s.info)
    _records(got, s)
