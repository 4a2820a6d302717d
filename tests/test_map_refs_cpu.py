"""The refs mapper without a GPU: the CPU oracle (tests/map_refs_oracle.py) against answers written out by hand; that the
inputs of tests/map_refs_inputs.py are not vacuous (the existing single-text oracles, run on the concatenation, answer
differently); sam.write_refs on a hand-built result; the new symbols; the errors decided before any device call."""
import ctypes as C
import io
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import map_refs_inputs as ri  # noqa: E402


# ---------------------------------------------------------------- the oracle against hand-written answers
def test_oracle_straddling_read_by_hand():
    """X | Y of 100 bases each, the read = X[85:100] + Y[0:15].  Seeds at 0 and 5 lie in X on the local diagonal 85, the seed
    at 10 exists only across the junction, seeds at 15 and 20 lie in Y on the diagonal -15.  Two clusters of two votes, X's
    first (contig ascending); each window aligns 15 bases (15 * 5 = 75), the tie goes to rank 0."""
    (h,), info = ri.expected("straddle")
    assert (h.flags, h.rid, h.score, h.second, h.votes) == (1, 0, 75, 75, 2)
    assert (h.ref_start, h.ref_end, h.read_start, h.read_end) == (85, 100, 0, 15)
    assert [(c[0], c[1], c[2], c[4], c[5]) for c in h.cands] == [(2, 0, 0, 79, 100), (2, 0, 1, 0, 21)]
    assert info["straddling"] == 1 and info["hits"] == 4 and info["clusters"] == 2 and info["seeds"] == 10


def test_oracle_short_contigs_by_hand():
    """the 16-mer M at local position 2 of contig 1 ("AC" + M) and 0 of contig 2 (M + "GTA"), band 24: one vote each, ranked
    by contig, equal scores (16 * 5), so contig 1 wins with second == score"""
    (h,), info = ri.expected("short_contigs")
    assert [(c[0], c[2], c[4], c[5]) for c in h.cands] == [(1, 1, 0, 18), (1, 2, 0, 19)]
    assert (h.flags, h.rid, h.score, h.second, h.votes, h.ref_start, h.ref_end) == (1, 1, 80, 80, 1, 2, 18)
    assert info["clusters"] == 2 and info["hits"] == 2 and info["straddling"] == 0


def test_oracle_overhang_by_hand():
    """P | Q | R with Q of 90 bases.  Read 0 = P's last 10 + Q's first 30: in Q it is soft-clipped by 10 at its start; read 1 =
    Q's last 30 + R's first 10: clipped by 10 at its end.  30 * 5 = 150; the neighbour's cluster (one seed, 10 bases) scores
    50."""
    (a, b), info = ri.expected("overhang")
    assert (a.flags, a.rid, a.score, a.second, a.ref_start, a.ref_end, a.read_start, a.read_end) == (1, 1, 150, 50, 0, 30, 10, 40)
    assert (b.flags, b.rid, b.score, b.second, b.ref_start, b.ref_end, b.read_start, b.read_end) == (1, 1, 150, 50, 60, 90, 0, 30)
    assert a.alignA == a.alignB == ri.overhang().contigs[1][:30]
    assert info["straddling"] == 2


# ---------------------------------------------------------------- the inputs separate the two definitions
def test_single_text_oracle_on_the_concatenation_differs():
    (r,), _ = ri.expected("straddle")
    (s,), _ = ri.single_text("straddle")
    assert s.score == 150 and s.read_end - s.read_start == 30 and s.ref_start == 85 and s.ref_end == 115   # across the junction
    assert r.score == 75
    (r,), _ = ri.expected("short_contigs")
    (s,), _ = ri.single_text("short_contigs")
    assert s.clusters == 1 and s.cands[0][0] == 2 and r.clusters == 2 and r.votes == 1                      # one merged cluster
    ra, _ = ri.expected("overhang")
    sa, _ = ri.single_text("overhang")
    for r, s in zip(ra, sa):
        assert s.score == 200 and s.read_end - s.read_start == 40 and r.read_end - r.read_start == 30


def test_single_text_pairs_oracle_on_the_concatenation_differs():
    (r,), info = ri.expected_pairs("adjacent_pair")
    (s,), _ = ri.single_text_pairs("adjacent_pair")
    assert s.proper and s.case == "pair" and s.tlen == 120
    assert not r.proper and r.tlen == 0 and r.case == "fallback" and (r.h1.flags, r.h2.flags) == (1, 3)
    assert (r.h1.rid, r.h1.ref_start, r.h2.rid, r.h2.ref_start) == (0, 230, 1, 10)
    (r,), info = ri.expected_pairs("rescue_clip")
    (s,), _ = ri.single_text_pairs("rescue_clip")
    assert s.case == "rescue" and s.h2.flags == 15 and s.h2.ref_start == 305
    assert r.case == "fallback" and r.h2.flags == 0 and r.h1.flags == 1 and info["rescue_attempts"] == 1 and info["rescued"] == 0
    at = r.attempts[0]
    assert at.raw == (254, 446) and (at.wlo, at.whi) == (254, 300)   # unclipped it holds the copy, C[305, 345); clipped to X


def test_rescue_inside_a_later_contig():
    res, info = ri.expected_pairs("rescue_inside")
    assert [r.case for r in res] == ["rescue", "rescue", "pair", "pair"] and [r.anchor for r in res[:2]] == [1, 2]
    assert [(r.h1.rid, r.h2.rid) for r in res] == [(3, 3), (3, 3), (2, 2), (1, 1)] and all(r.tlen == 140 for r in res)
    assert len(res[3].proper_combos) == 2                      # contigs 1 and 4: the smallest (k1, k2) is contig 1's
    assert (res[0].h2.ref_start, res[1].h1.ref_start) == (150, 60) and info["rescued"] == 2


def test_max_occ_counts_the_straddling_occurrence():
    (_, info_with), (_, info_without) = ri.expected("max_occ0"), ri.expected("max_occ1")
    assert info_with["seeds_over_max_occ"] == 1 and info_without["seeds_over_max_occ"] == 0
    assert info_without["hits"] == info_with["hits"] + 2 and info_with["straddling"] == 0    # a dropped seed locates nothing
    with_, without = ri.max_occ_pair()
    S = with_.reads[0][10:20]
    assert ri.join(with_.contigs).count(S) == 3 and sum(c.count(S) for c in with_.contigs) == 2
    assert ri.join(without.contigs).count(S) == 2


def test_inputs_have_the_shapes_the_cases_name():
    m = ri.many()
    assert len(m.contigs) == 300 and len(m.reads) == 200 and all(40 <= len(c) <= 90 for c in m.contigs)
    hits, info = ri.expected("many")
    rids = {h.rid for h in hits if h.flags & 1}
    assert 0 in rids and 299 in rids and len(rids) > 100 and info["straddling"] >= 1
    assert {h.flags & 3 for h in hits} >= {1, 3} and max(h.clusters for h in hits) >= 6
    d = ri.degenerate()
    assert min(len(c) for c in d.contigs) == 1 and len(d.contigs[1]) < ri.P.seed_len and len(d.reads[0]) > len(d.contigs[3])
    (h, *_), _ = ri.expected("degenerate")
    assert h.rid == 3 and (h.ref_start, h.ref_end, h.read_start, h.read_end) == (0, 25, 5, 30) and h.cands[0][4:6] == (0, 25)
    (a, b), _ = ri.expected("duplicates")
    assert a.rid == b.rid == 2 and a.second == a.score == 300 and b.flags == 3


# ---------------------------------------------------------------- sam.write_refs
def test_write_refs_on_a_hand_built_result():
    from poly_amd import mapper, sam
    u32 = lambda *x: np.array(x, np.uint32)   # noqa: E731
    n = 6
    strings = [b"AACC", b"GGTT", b"AACC", b"AACC", b"", b"AACC"]
    res = mapper.MapResult(np.full(n, 20, np.int64), np.zeros(n, np.int64), u32(5, 7, 1, 1, 0, 1), u32(1, 1, 1, 1, 0, 1),
                           u32(10, 60, 5, 7, 0, 20), u32(14, 64, 9, 11, 0, 24), u32(0, 0, 0, 0, 0, 0), u32(4, 4, 4, 4, 0, 4),
                           np.zeros(n, np.uint32), strings, strings, tlen=np.array([54, 0, 0], np.int64), rid=u32(0, 0, 0, 1, 0, 1))
    live = [1, 1, 1, 1, 0, 1]
    rec = sam.AlnRecords(np.cumsum([0] + live).astype(np.uint64), np.full(5, 4 << 4, np.uint32),
                         np.cumsum([0] + live).astype(np.uint64), np.frombuffer(b"44444", np.uint8), np.zeros(n, np.uint32),
                         np.full(n, 60, np.uint8), u32(99, 147, 65, 129, 69, 137), np.zeros(n, np.uint32))
    refs = types.SimpleNamespace(names=["chrA", "chrB"], lengths=np.array([100, 80]))
    out = io.StringIO()
    sam.write_refs(out, refs, [f"r{i}" for i in range(n)], [b"AACC"] * n, None, res, rec, paired=True)
    lines = out.getvalue().splitlines()
    assert lines[:3] == ["@HD\tVN:1.6\tSO:unsorted", "@SQ\tSN:chrA\tLN:100", "@SQ\tSN:chrB\tLN:80"]
    body = [ln.split("\t") for ln in lines[3:]]
    assert len(body) == n
    # QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ
    assert body[0][:10] == ["r0", "99", "chrA", "11", "60", "4M", "=", "61", "54", "AACC"]
    assert body[1][:10] == ["r1", "147", "chrA", "61", "60", "4M", "=", "11", "-54", "GGTT"]
    assert body[2][:10] == ["r2", "65", "chrA", "6", "60", "4M", "chrB", "8", "0", "AACC"]      # mates on two contigs
    assert body[3][:10] == ["r3", "129", "chrB", "8", "60", "4M", "chrA", "6", "0", "AACC"]
    assert body[4][:10] == ["r4", "69", "chrB", "21", "0", "*", "=", "21", "0", "AACC"]         # placed with its live mate
    assert body[5][:10] == ["r5", "137", "chrB", "21", "60", "4M", "*", "0", "0", "AACC"]
    assert body[0][11:] == ["NM:i:0", "MD:Z:4", "AS:i:20"] and len(body[4]) == 11


# ---------------------------------------------------------------- the symbols, and the errors before any device call
NEW = ["polyhip_refs_create", "polyhip_refs_destroy", "polyhip_refs_count", "polyhip_refs_starts", "polyhip_refs_index",
       "polyhip_refs_resolve", "polyhip_map_reads_refs", "polyhip_map_pairs_refs", "polyhip_map_refs_last_info"]


def test_symbols_are_exported_and_bound():
    from poly_amd import _lib, mapper, pileup, refs, sam
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert not [n for n in NEW if n.endswith("_dev")]
    for mod, names in ((mapper, ["map_reads_refs_packed", "MapReadsRefs", "map_pairs_refs_packed", "MapPairsRefs", "last_refs_info"]),
                       (refs, ["RefSet", "New", "new_packed", "from_fasta"]), (sam, ["write_refs"]), (pileup, ["pileup_refs"])):
        for n in names:
            assert callable(getattr(mod, n)), n
    assert mapper.MapRecord(True, False, 1, 0, 1, 0, 1, 0, 1, b"", b"", 0).rid == 0
    assert mapper.MapResult(*[None] * 11).rid is None
    info = mapper.last_refs_info()
    assert set(info) == {"contigs", "straddling"}


def _create(buf: bytes, offs, k=None, null_seqs=False, null_off=False, null_out=False):
    from poly_amd import _lib
    b = np.frombuffer(buf, np.uint8) if buf else np.zeros(1, np.uint8)
    o = np.array(offs, np.uint64)
    h = C.c_void_p()
    rc = _lib.lib().polyhip_refs_create(None if null_seqs else b.ctypes.data, None if null_off else o.ctypes.data,
                                        len(offs) - 1 if k is None else k, None if null_out else C.byref(h))
    return rc, _lib.lib().polyhip_last_error().decode(), h


def test_create_errors_are_decided_before_any_device_call():
    from poly_amd import _lib
    for kw in (dict(null_seqs=True), dict(null_off=True), dict(null_out=True)):
        rc, msg, h = _create(b"ACGTACGT", [0, 4, 8], **kw)
        assert rc == _lib.ERR_INVALID and "null" in msg and not h.value
    rc, msg, _ = _create(b"ACGT", [0], k=0)
    assert rc == _lib.ERR_INVALID and "at least one contig" in msg
    rc, msg, _ = _create(b"ACGTACGT", [0, 4, 4, 8])
    assert rc == _lib.ERR_INVALID and "contig 1 is empty" in msg
    rc, msg, _ = _create(b"ACGTACGT", [0, 5, 4, 8])
    assert rc == _lib.ERR_INVALID and "not ascending at 1" in msg
    rc, msg, _ = _create(b"ACGT$CGT", [0, 4, 8])
    assert rc == _lib.ERR_INVALID and msg == "Provided sequence contains the nullChar $. BWT cannot be constructed"
    rc, msg, _ = _create(b"ACGT", [0, 4], k=(1 << 24) + 1)
    assert rc == _lib.ERR_UNSUPPORTED and "2^24" in msg
    rc, msg, _ = _create(b"", [0, 0xFFFFFFFF], k=1)            # the length is judged from the offsets: nothing is read
    assert rc == _lib.ERR_INVALID and "too long" in msg
    assert _lib.lib().polyhip_refs_count(None) == _lib.ERR_INVALID and _lib.lib().polyhip_refs_index(None) is None
    assert _lib.lib().polyhip_refs_destroy(None) == _lib.OK


def test_null_set_and_bad_parameters_without_gpu():
    from poly_amd import _lib, mapper
    out = [np.zeros(2, np.int64) for _ in range(2)] + [np.zeros(2, np.uint32) for _ in range(8)]
    reads, off = np.frombuffer(b"ACGTACGTAC", np.uint8), np.array([0, 10], np.uint64)
    sc = C.c_void_p(1)                                          # never looked at: the handle check comes first
    p = mapper.MapParams(seed_len=0)._c()
    call = lambda p_: _lib.lib().polyhip_map_reads_refs(None, sc, C.byref(p_), -5, -2, reads.ctypes.data, off.ctypes.data, 1, 10, 0,  # noqa: E731
                                                        *[a.ctypes.data for a in out], None, None, None, 0)
    assert call(p) == _lib.ERR_INVALID and b"seed_len" in _lib.lib().polyhip_last_error()
    assert call(mapper.MapParams()._c()) == _lib.ERR_INVALID and b"null index handle" in _lib.lib().polyhip_last_error()
    with pytest.raises(ValueError):
        mapper.map_pairs_refs_packed(None, None, -5, -2, reads, off, reads, off)
