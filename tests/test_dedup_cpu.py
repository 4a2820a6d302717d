"""polyhip_mark_duplicates and polyhip_coord_order without a GPU: the oracle (tests/dedup_oracle.py) against answers written out
by hand, what the hand-built inputs (tests/dedup_inputs.py) hold, the declarations, the argument errors that need no device,
sam.write's ``order`` and ``dup``, and the conditions of the end-to-end test through the CPU oracle of the affine mapper."""
import ctypes as C
import io
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import aln_records_inputs as ari  # noqa: E402
import aln_records_oracle as aro  # noqa: E402
import dedup_inputs as di  # noqa: E402
import dedup_oracle as do  # noqa: E402

M, R = di.MAPPED, di.REVERSE


def _mark(rows, **kw):
    """rows: (flags, ref_start, ref_end, read_start, read_end, read_len[, weight[, rid]])"""
    c = [list(x) for x in zip(*[tuple(r) + (0, 0)[:8 - len(r)] for r in rows])]
    return do.mark(c[0], c[1], c[2], c[3], c[4], c[5], rid=c[7], weight=c[6], **kw)


def _dr(m):
    return m.dup.tolist(), m.rep.tolist()


# ---------------------------------------------------------------- 1. the oracle against answers worked out by hand
def test_oracle_fragments_by_hand():
    f = lambda u, w=0, clip=0, rid=0: (M, u + clip, u + 50, clip, 50, 50, w, rid)                   # noqa: E731
    r = lambda u, w=0, clip=0, rid=0: (M | R, u - 49, u + 1 - clip, 0, 50 - clip, 50, w, rid)       # noqa: E731
    assert _dr(_mark([f(100, 1), f(100, 2)])) == ([1, 0], [1, 1])                                  # 1. the greater weight wins
    assert _dr(_mark([f(100, 7), f(100, 7, clip=3), f(100, 7)])) == ([0, 1, 1], [0, 0, 0])         # 2. a tie: the lowest index
    assert _dr(_mark([f(100, 1), r(100, 2), f(101, 3)])) == ([0, 0, 0], [0, 1, 2])                 # 3. strands and positions apart
    # 4. reverse entries: ref_end 201 and 198, the clip added back: one end
    a, b = (M | R, 151, 201, 0, 50, 50, 1, 0), (M | R, 151, 198, 0, 47, 50, 2, 0)
    assert do.end_key(0, 1, *a[1:6]) == do.end_key(0, 1, *b[1:6]) == (0, 200, 1) and _dr(_mark([a, b])) == ([1, 0], [1, 1])
    # 5. forward entries: the same ref_start, read_start 0 and 3: two ends
    assert _dr(_mark([(M, 100, 150, 0, 50, 50, 1, 0), (M, 100, 147, 3, 50, 50, 2, 0)])) == ([0, 0], [0, 1])
    # 6. an unmapped entry and an err 2 entry between two duplicates: neither is a candidate, neither is judged further
    m = _mark([f(100, 1), (0, 100, 150, 0, 50, 50, 9, 0), (M, 100, 150, 5, 4, 50, 9, 0), f(100, 2)])
    assert _dr(m) == ([1, 0, 0, 0], [3, 1, 2, 3]) and m.err.tolist() == [0, 0, 2, 0] and m.weight.tolist() == [1, 0, 0, 2]
    assert m.info == dict(entries=4, candidates=2, bad=1, pairs=0, fragments=2, dup_pairs=0, dup_fragments=1, pair_sets=0, end_sets=1)
    # 7. a negative u: read_start 10 at ref_start 5
    neg = [(M, 5, 45, 10, 50, 50, 1, 0), (M, 2, 45, 7, 50, 50, 2, 0), (M, 6, 45, 10, 50, 50, 3, 0)]
    assert do.end_key(0, 0, *neg[0][1:6]) == (0, -5, 0) and _dr(_mark(neg)) == ([1, 0, 0], [1, 1, 2])
    # 8. contigs keep entries apart; without rid they are one contig
    two = [f(100, 1, rid=0), f(100, 2, rid=1), f(100, 3, rid=0)]
    assert _dr(_mark(two)) == ([1, 0, 0], [2, 1, 2])
    c = list(zip(*two))
    assert _dr(do.mark(c[0], c[1], c[2], c[3], c[4], c[5], weight=c[6])) == ([1, 1, 0], [2, 2, 2])
    # the three forms of err 2, and ref_start == ref_end is none of them
    assert [do.entry_err(1, *x, None, 0, 33)[0] for x in ((0, 9, 5, 4, 9), (0, 9, 0, 10, 9), (9, 8, 0, 9, 9), (9, 9, 0, 0, 0))] == [2, 2, 2, 0]


def test_oracle_pairs_by_hand():
    f = lambda u, w=0, rid=0: (M, u, u + 50, 0, 50, 50, w, rid)                   # noqa: E731
    r = lambda u, w=0, rid=0: (M | R, u - 49, u + 1, 0, 50, 50, w, rid)           # noqa: E731
    un = (0, 0, 0, 0, 0, 50, 0, 0)
    # 9. read 1 left in pair 0, read 2 left in pair 1: one key; lo goes to lo and hi to hi
    m = _mark([f(100, 5), r(400, 5), r(400, 1), f(100, 1)], paired=True)
    assert _dr(m) == ([0, 0, 1, 1], [0, 1, 1, 0])
    assert m.info == dict(entries=4, candidates=4, bad=0, pairs=2, fragments=0, dup_pairs=1, dup_fragments=0, pair_sets=1, end_sets=2)
    assert _dr(_mark([f(100, 5), r(400, 5), r(400, 1), f(100, 1)])) == ([0, 0, 1, 1], [0, 1, 1, 0])      # as reads: by end alone
    # 10. a fragment loses to a pair mate at its end whatever its weight; its unmapped mate stays as it is
    assert _dr(_mark([f(100, 1), r(400, 1), f(100, 1000), un], paired=True)) == ([0, 0, 1, 0], [0, 1, 0, 3])
    # 11. ... also to the mates of a pair that is itself a duplicate, and its representative is the head of the end set
    m = _mark([f(100, 1), r(400, 1), f(100, 9), r(400, 9), f(100, 1000), un], paired=True)
    assert _dr(m) == ([1, 1, 0, 0, 1, 0], [2, 3, 2, 3, 2, 5])
    assert m.info == dict(entries=6, candidates=5, bad=0, pairs=2, fragments=1, dup_pairs=1, dup_fragments=1, pair_sets=1, end_sets=2)
    # 12. FR and FF at the same two positions are two keys; both mates at one end: lo is the lower index
    assert _dr(_mark([f(100), r(400), f(100), f(400), f(100), r(400)], paired=True))[0] == [0, 0, 0, 0, 1, 1]
    assert _dr(_mark([f(100, 1), f(100, 1), f(100, 2), f(100, 2)], paired=True)) == ([1, 1, 0, 0], [2, 3, 2, 3])
    # 13. the pair weight is a 33-bit sum
    top = di.TOP
    assert _dr(_mark([f(100, top), r(400, 1), f(100, top), r(400, 2)], paired=True)) == ([1, 1, 0, 0], [2, 3, 2, 3])
    # 14. mates on two contigs: lo is the mate on the lower contig
    assert _dr(_mark([f(100, 1, 1), r(400, 1, 0), r(400, 2, 0), f(100, 2, 1)], paired=True)) == ([1, 1, 0, 0], [3, 2, 2, 3])


def test_oracle_quality_weights_and_coord_order_by_hand():
    rows = [(M, 100, 103, 0, 3, 3)] * 5
    c = list(zip(*rows))
    q = b"III" + b"555" + b"II" + b"I5\x20" + b"~5I"                       # Q 40 40 40 | 20 20 20 | too short | byte 32 | Q 93
    off = [0, 3, 6, 8, 11, 14]
    m = do.mark(*c, qual=q, qual_off=off, min_weight_qual=15, qual_offset=33)
    assert m.err.tolist() == [0, 0, 6, 7, 0] and m.weight.tolist() == [120, 60, 0, 0, 153] and _dr(m) == ([1, 1, 0, 0, 0], [4, 4, 2, 3, 4])
    m = do.mark(*c, qual=q, qual_off=off, min_weight_qual=41, qual_offset=33)
    assert m.weight.tolist() == [0, 0, 0, 0, 93] and m.rep.tolist() == [4, 4, 2, 3, 4]
    m = do.mark(*c, qual=q, qual_off=off, min_weight_qual=0, qual_offset=53)           # '5' is Q 0; 'I' is Q 20; '~' is Q 73
    assert m.err.tolist() == [0, 0, 6, 7, 0] and m.weight.tolist() == [60, 0, 0, 0, 93]
    # coordinate order: live by (rid, ref_start); the unmapped mate beside its live mate; the rest last, in index order
    sf, fs, rid = [0, 4, 0x10, 4], [50, 0, 10, 0], [1, 0, 0, 0]
    assert do.coord_order(sf, fs, rid).tolist() == [2, 0, 1, 3] and do.coord_order(sf, fs, rid, paired=True).tolist() == [2, 3, 0, 1]
    assert do.coord_order(sf, fs).tolist() == [2, 0, 1, 3] and do.coord_order([0, 0, 0], [7, 3, 7]).tolist() == [1, 0, 2]
    assert do.coord_order([4, 4, 0, 4], [1, 2, 3, 4], None, True).tolist() == [2, 3, 0, 1]


# ---------------------------------------------------------------- 2. what the hand-built inputs hold
def _want(s, mode):
    return do.mark(**s.kwargs(mode))


def test_inputs_sizes_and_sets():
    assert [len(di.sized(n).flags) for n in di.SIZES] == [1, 2, 255, 256, 257, 4095, 4096, 4097] == list(di.SIZES)
    names = [s.name for s in di.all_sets()]
    assert len(names) == len(set(names)) and all(s.modes for s in di.all_sets())
    for s in di.all_sets():
        assert all(not m["paired"] or len(s.flags) % 2 == 0 for m in s.modes) and len(s.flags) <= 20000
    for k in di.SET_SIZES:
        s = di.end_set(k)
        w = _want(s, s.modes[0])
        members = [i for i in range(len(s.flags)) if s.flags[i] == M and s.u()[i] == 300]
        assert len(members) == k and w.dup[members].sum() == k - 1 and set(w.rep[members]) == {members[k // 2]}
        assert s.weight[members[k // 2]] == 1000 and len({int(x) for x in s.read_start[members]}) == min(k, 4)
    one = di.one_set()
    assert len(one.flags) == 10000 and _want(one, one.modes[0]).info["end_sets"] == 1 and _want(one, one.modes[0]).info["dup_fragments"] == 9999
    assert _want(one, one.modes[1]).info["pair_sets"] == 1 and _want(one, one.modes[1]).info["dup_pairs"] == 4999
    rnd = di.random_set()
    assert len(rnd.flags) == 20000 and set(rnd.rid[(rnd.flags & 1) == 1]) == {0, 1, 2}
    for mode in rnd.modes:
        i = _want(rnd, mode).info
        assert i["bad"] > 100 and i["candidates"] < 19000 and i["end_sets"] <= 50 * 3 * 2 and i["dup_fragments"] > 0
    paired = _want(rnd, rnd.modes[1]).info
    assert paired["pairs"] > 8000 and paired["fragments"] > 1000 and 0 < paired["dup_pairs"] < paired["pairs"] - paired["pair_sets"] + 1
    assert len(di.empty().flags) == 0 and _want(di.empty(), {"paired": True}).info["entries"] == 0


def test_inputs_weights_and_ends():
    w = lambda name, k=0: _want(di.by_name(name), di.by_name(name).modes[k])       # noqa: E731
    assert len(set(di.by_name("w_equal").weight)) == 1 and w("w_equal").rep.tolist() == [0] * 5
    assert w("w_bit0").rep.tolist() == [1, 1, 1, 3, 3] and w("w_bit31").rep.tolist() == [1, 1, 1, 3, 3]
    assert int(di.by_name("w_bit31").weight[1]) ^ int(di.by_name("w_bit31").weight[2]) == di.TOP
    assert set(w("w_winner_last").rep) == {299} and w("w_winner_last", 1).info["dup_pairs"] == 149
    big = di.by_name("w_pair_sum_bit32")
    assert all(int(big.weight[2 * p]) + int(big.weight[2 * p + 1]) >= 1 << 32 for p in (0, 1)) and w("w_pair_sum_bit32").rep.tolist() == [2, 3, 2, 3, 2, 3]
    assert di.by_name("w_null").weight is None and w("w_null").rep.tolist() == [0, 0, 0]
    neg = di.by_name("u_negative")
    assert neg.u() == [-5, -5, -4, 0] and (neg.read_start[:3] > neg.ref_start[:3]).all() and w("u_negative").rep.tolist() == [1, 1, 2, 3]
    st = di.by_name("strands_equal_u")
    assert len(set(st.u())) == 1 and w("strands_equal_u").rep.tolist() == [2, 3, 2, 3]
    mg = di.by_name("reverse_clips_merge")
    assert len(set(mg.u())) == 1 and len(set(mg.ref_end)) == 3 and len(set(mg.read_len - mg.read_end)) == 3 and w("reverse_clips_merge").rep.tolist() == [2, 2, 2]
    nm = di.by_name("forward_clips_differ")
    assert len(set(nm.ref_start)) == 1 and nm.u() == [100, 97, 100] and w("forward_clips_differ").rep.tolist() == [2, 1, 2]
    wide = di.by_name("u_wide")
    biased = sorted({u + (1 << 32) for u in wide.u()})
    assert biased == [2, (1 << 32) - 1, (1 << 33) - 1, (1 << 33) + (1 << 32) - 13] and biased[-1] >> 33 == 1 and biased[-2] >> 32 == 1
    assert w("u_wide").dup.tolist() == [1, 1, 1, 1, 0, 0, 0, 0] and w("u_wide").info["end_sets"] == 4
    assert w("rid_only").rep.tolist() == [2, 3, 2, 3, 4]
    ex = di.by_name("rid_extremes")
    assert set(ex.rid) == {0, di.TOP} and w("rid_extremes").rep.tolist() == [2, 1, 2, 3, 1, 5]
    assert di.by_name("rid_null").rid is None and w("rid_null").rep.tolist() == [1, 1, 2]


def test_inputs_pairs_errs_and_qualities():
    w = lambda name, k=0: _want(di.by_name(name), di.by_name(name).modes[k])       # noqa: E731
    assert w("pair_read2_left").rep.tolist() == [0, 1, 1, 0] and w("pair_read2_left").info["pair_sets"] == 1
    assert w("pair_mates_same_end").rep.tolist() == [2, 3, 2, 3, 2, 3] and w("pair_mates_same_end").info["end_sets"] == 1
    x = w("pair_two_contigs")
    assert x.rep.tolist() == [3, 2, 2, 3, 4, 5] and x.info["pair_sets"] == 2
    o = w("pair_orientations")
    assert o.info["pair_sets"] == 4 and o.info["dup_pairs"] == 4 and o.dup.tolist() == [1] * 8 + [0] * 8
    fr = w("fragment_at_duplicate_pair")
    assert fr.dup.tolist() == [0, 0, 1, 1, 1, 0, 0, 1] and fr.rep.tolist() == [0, 1, 0, 1, 0, 5, 6, 1] and fr.info["fragments"] == 2
    al = w("fragments_alone")
    assert al.info["pairs"] == 0 and al.rep.tolist() == [2, 1, 2, 3, 4, 2, 6, 7] and al.err.tolist() == [0] * 7 + [2]
    br = w("pair_mate_unmapped_or_err2", 1)
    assert br.info["pairs"] == 2 and br.info["fragments"] == 2 and br.err.tolist() == [0, 0, 0, 2, 0, 0, 0, 0, 0, 0]
    assert br.rep.tolist() == [4, 1, 4, 3, 4, 5, 4, 5] + [8, 9] and w("pair_mate_unmapped_or_err2", 0).rep.tolist()[:3] == [4, 1, 4]
    e = w("errs")
    assert e.err.tolist() == [0, 2, 0, 2, 2, 2, 0, 0] and e.rep.tolist() == [2, 1, 2, 3, 4, 5, 6, 2] and e.weight.tolist() == [1, 0, 2, 0, 0, 0, 0, 2]
    ql = di.by_name("qual_lengths")
    assert sorted(set(np.diff(ql.qual_off).astype(int))) == list(di.QUAL_LENGTHS) and [m["min_weight_qual"] for m in ql.modes[:3]] == [0, 15, 93]
    at = len(di.QUAL_LENGTHS) * 4
    assert [w("qual_lengths", k).weight[at:at + 4].tolist() for k in range(3)] == [[93 * 64, 14 * 64, 15 * 64, 0], [93 * 64, 0, 15 * 64, 0],
                                                                                 [93 * 64, 0, 0, 0]]
    assert w("qual_lengths", 0).weight[:4].tolist() == [0, 0, 0, 0] and w("qual_lengths", 0).rep[:4].tolist() == [0, 0, 0, 0]
    qe = w("qual_errs", 1)
    assert qe.err.tolist() == [0, 6, 6, 7, 7, 2, 0, 0, 6, 0] and qe.rep.tolist()[0] == 9 and qe.rep.tolist()[7] == 9 and qe.weight[9] > qe.weight[0]
    qo = di.by_name("qual_offset64")
    assert w("qual_offset64", 0).weight.tolist() == [sum(range(5, 10)), 930, 0] and w("qual_offset64", 0).err.tolist() == [0, 0, 7]
    assert w("qual_offset64", 1).err.tolist() == [7, 7, 7] and qo.modes[1]["qual_offset"] == 162


# ---------------------------------------------------------------- 3. the declarations and the errors that need no device
def test_declarations():
    from poly_amd import _lib, dedup
    assert len(_lib.SIGNATURES["polyhip_mark_duplicates"][1]) == 16 and len(_lib.SIGNATURES["polyhip_coord_order"][1]) == 6
    assert "polyhip_dedup_last_info" in _lib.SIGNATURES
    assert C.sizeof(dedup._CParams) == 16 and C.sizeof(dedup._CInfo) == 72
    assert tuple(n for n, _ in dedup._CInfo._fields_) == do.INFO_FIELDS
    header = open(os.path.join(ROOT, "include", "polyhip.h")).read()
    assert "uint64_t entries, candidates, bad, pairs, fragments, dup_pairs, dup_fragments, pair_sets, end_sets;" in header
    for f in (dedup.mark_packed, dedup.mark, dedup.last_info, dedup.coord_order, dedup.coord_order_packed):
        assert callable(f)


def test_argument_errors_without_gpu():
    """what is decided before any device call returns its status and message without a device, in the documented order"""
    from poly_amd import _lib, dedup
    L = _lib.lib()
    a32, a8 = np.zeros(2, np.uint32), np.zeros(2, np.uint8)
    big = np.array([1 << 31, 5], np.uint32)
    up, down = np.array([0, 1, 2], np.uint64), np.array([0, 2, 1], np.uint64)
    P = dedup._CParams

    def call(params, n=2, flags=a32, read_len=a32, qual=a8, off=up, err=a32):
        p = lambda x: None if x is None else x.ctypes.data      # noqa: E731
        rc = L.polyhip_mark_duplicates(None if params is None else C.byref(params), n, p(flags), None, a32.ctypes.data, a32.ctypes.data,
                                       a32.ctypes.data, a32.ctypes.data, p(read_len), None, p(qual), p(off), None, a8.ctypes.data,
                                       a32.ctypes.data, p(err))
        return rc, L.polyhip_last_error()

    for params, kw, status, word in (
            (None, {}, _lib.ERR_INVALID, b"null params"),
            (P(2, 2, 94, 163), {}, _lib.ERR_INVALID, b"paired"),
            (P(1, 2, 94, 163), {}, _lib.ERR_INVALID, b"weight_mode"),
            (P(1, 1, 94, 163), {}, _lib.ERR_INVALID, b"min_weight_qual"),
            (P(1, 0, 93, 163), {}, _lib.ERR_INVALID, b"qual_offset"),
            (P(1, 0, 93, 162), dict(n=3, flags=None), _lib.ERR_INVALID, b"mates come in twos"),
            (P(1, 0, 93, 162), dict(n=(1 << 32) + 1), _lib.ERR_INVALID, b"mates come in twos"),
            (P(1, 0, 93, 162), dict(n=1 << 32, flags=None), _lib.ERR_UNSUPPORTED, b"2^32"),
            (P(0, 0, 0, 0), dict(n=(1 << 32) + 1, flags=None), _lib.ERR_UNSUPPORTED, b"2^32"),
            (P(0, 0, 0, 0), dict(flags=None), _lib.ERR_INVALID, b"null argument"),
            (P(0, 0, 0, 0), dict(err=None), _lib.ERR_INVALID, b"null argument"),
            (P(0, 1, 0, 33), dict(off=None), _lib.ERR_INVALID, b"null argument"),
            (P(0, 1, 0, 33), dict(qual=None), _lib.ERR_INVALID, b"null argument"),
            (P(0, 1, 0, 33), dict(qual=None, off=down), _lib.ERR_INVALID, b"null argument"),
            (P(0, 1, 0, 33), dict(off=down, read_len=big), _lib.ERR_INVALID, b"not ascending"),
            (P(0, 1, 0, 33), dict(read_len=big), _lib.ERR_UNSUPPORTED, b"entry 0 has 2147483648 bases")):
        rc, msg = call(params, **kw)
        assert rc == status and word in msg and b"polyhip_mark_duplicates" in msg, (kw, rc, msg)
    # what needs no device at all: the empty batch, with nothing but params
    assert L.polyhip_mark_duplicates(C.byref(P(1, 1, 15, 33)), 0, *[None] * 14) == _lib.OK and dedup.last_info()["entries"] == 0
    with pytest.raises(_lib.PolyhipError) as ei:
        dedup.mark_packed([1], [0], [4], [0], [4], 4, min_weight_qual=94)
    assert ei.value.status == _lib.ERR_INVALID and "min_weight_qual" in ei.value.message
    with pytest.raises(ValueError):
        dedup.mark_packed([1], [0], [4], [0], [4], 4, weight=[1], qual=b"IIII", qual_off=[0, 4])

    def order(n, paired, sf=a32, fs=a32, out=a32):
        p = lambda x: None if x is None else x.ctypes.data      # noqa: E731
        return L.polyhip_coord_order(n, paired, p(sf), None, p(fs), p(out)), L.polyhip_last_error()

    for args, status, word in (((3, 2), _lib.ERR_INVALID, b"paired = 2"), ((3, 1), _lib.ERR_INVALID, b"mates come in twos"),
                               (((1 << 32) + 1, 1), _lib.ERR_INVALID, b"mates come in twos"), ((1 << 32, 1), _lib.ERR_UNSUPPORTED, b"2^32"),
                               ((2, 0, None), _lib.ERR_INVALID, b"null argument"), ((2, 0, a32, None), _lib.ERR_INVALID, b"null argument"),
                               ((2, 1, a32, a32, None), _lib.ERR_INVALID, b"null argument")):
        rc, msg = order(*args)
        assert rc == status and word in msg and b"polyhip_coord_order" in msg, (args, rc, msg)
    assert order(0, 1, None, None, None)[0] == _lib.OK
    assert dedup.coord_order_packed([], []).tolist() == []


# ---------------------------------------------------------------- 4. sam.write: order and dup
def _records(cs, paired):
    p = ari.pack(cs)
    return p, aro.records(p["flags"], p["score"], p["second"], p["read_start"], p["read_end"], p["read_len"], p["alnA"].tobytes(),
                          p["alnB"].tobytes(), p["aln_off"], eqx=False, paired=paired)


def _write(rec, ref_start, score, tlen, names, reads, quals, paired, **kw):
    from poly_amd import sam
    fh = io.StringIO()
    result = SimpleNamespace(ref_start=np.array(ref_start, np.uint32), score=np.array(score, np.int64), tlen=np.array(tlen, np.int64))
    got = SimpleNamespace(sam_flag=rec.sam_flag, mapq=rec.mapq, nm=rec.nm, cigar_string=rec.cigar_string, md_string=rec.md_string)
    sam.write(fh, "chr", 5000, names, reads, quals, result, got, paired=paired, **kw)
    return fh.getvalue()


@pytest.mark.parametrize("which", ["cases", "batch257", "paired"])
def test_sam_write_defaults_change_nothing(which):
    cs = {"cases": ari.cases, "batch257": lambda: ari.batch(257), "paired": ari.paired_batch}[which]()
    cs = [c for c in cs if len(c.A) <= 1100]
    paired = which == "paired"
    p, rec = _records(cs, paired)
    n = len(cs)
    ref_start, tlen = [(37 * i) % 4000 for i in range(n)], [(-1) ** i * (100 + i) for i in range(n // 2)]
    names, reads = [f"r{i // 2 if paired else i}" for i in range(n)], [b"ACGTN"[i % 5:] + b"GATTACA" for i in range(n)]
    quals = ["".join(chr(40 + (i + j) % 50) for j in range(len(reads[i]))) for i in range(n)]
    want = "\n".join(aro.sam_lines("chr", 5000, names, reads, quals, ref_start, p["score"], tlen, rec, paired)) + "\n"
    assert _write(rec, ref_start, p["score"], tlen, names, reads, quals, paired) == want
    assert _write(rec, ref_start, p["score"], tlen, names, reads, quals, paired, order=None, dup=None) == want
    # the identity order and no duplicates: only the header differs
    same = _write(rec, ref_start, p["score"], tlen, names, reads, quals, paired, order=np.arange(n), dup=np.zeros(n, np.uint8))
    assert same == want.replace("SO:unsorted", "SO:coordinate", 1) and want.count("SO:unsorted") == 1


def test_sam_write_order_and_dup_by_hand():
    from poly_amd import sam
    A = [b"ACGT", b"", b"GGCA"]
    flags, score = [1, 0, 1 | 2], [20, 0, 18]
    off = np.concatenate([[0], np.cumsum([len(a) for a in A])])
    rec = aro.records(flags, score, [0, 0, 0], [0, 0, 0], [4, 0, 4], [4, 3, 4], b"".join(A), b"".join(A), off)
    args = (rec, [300, 0, 100], score, [], ["a", "b", "c"], [b"ACGT", b"TTT", b"TGCC"], ["IIII", "###", "ABCD"], False)
    head = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr\tLN:5000\n"
    a = "a\t{}\tchr\t301\t60\t4M\t*\t0\t0\tACGT\tIIII\tNM:i:0\tMD:Z:4\tAS:i:20\n"
    b = "b\t{}\t*\t0\t0\t*\t*\t0\t0\tTTT\t###\n"
    c = "c\t{}\tchr\t101\t60\t4M\t*\t0\t0\tGGCA\tDCBA\tNM:i:0\tMD:Z:4\tAS:i:18\n"
    assert _write(*args, order=[2, 0, 1]) == head + c.format(16) + a.format(0) + b.format(4)
    assert _write(*args, order=[2, 0, 1], dup=[1, 0, 1]) == head + c.format(16 | 1024) + a.format(1024) + b.format(4)
    assert _write(*args, dup=np.array([0, 0, 1], np.uint8)) == head.replace("coordinate", "unsorted") + a.format(0) + b.format(4) + c.format(1040)
    assert sam.FLAG_DUPLICATE == 0x400
    with pytest.raises(ValueError):
        _write(*args, order=[2, 0, 0])


# ---------------------------------------------------------------- 5. the end-to-end reads, through the mapper's CPU oracle
def test_planted_copies_share_their_templates_end():
    """what tests/test_dedup_gpu.py::test_end_to_end_pileup_without_duplicates relies on: every read is mapped, every copy has its
    template's end whatever was clipped, and no two of the 200 independent reads share one -- so exactly the copies are duplicates"""
    import map_affine_inputs as mai
    import map_affine_oracle as mao
    d = di.planted()
    T, reads = d["T"], d["reads"]
    assert len(T) == 4000 and len(reads) == 300 and {len(r) for r in reads} == {di.PLANTED_READ} and len(set(d["sites"])) == 20
    hits, _ = mao.map_reads(T, reads, mai.MAT, *mai.GAPS[di.PLANTED_GAPS], mai.PARAMS)
    assert all(h.flags & 1 for h in hits)
    E = [do.end_key(0, h.flags >> 1 & 1, h.ref_start, h.ref_end, h.read_start, h.read_end, di.PLANTED_READ) for h in hits]
    assert len(set(E[:200])) == 200 and sum(e[2] for e in E[:200]) == 100
    clips = set()
    for t, k in enumerate(d["template"]):
        assert (E[k][2] == 1) == (t % 2 == 1)
        for j in range(di.PLANTED_COPIES):
            h = hits[200 + di.PLANTED_COPIES * t + j]
            assert E[200 + di.PLANTED_COPIES * t + j] == E[k]
            clip = di.PLANTED_READ - h.read_end if h.flags & 2 else h.read_start
            assert clip == j + 1
            clips.add((h.flags >> 1 & 1, clip))
    assert len(clips) == 10
    m = do.mark([h.flags for h in hits], [h.ref_start for h in hits], [h.ref_end for h in hits], [h.read_start for h in hits],
                [h.read_end for h in hits], di.PLANTED_READ)
    assert m.dup.tolist() == [0] * 200 + [1] * 100 and m.rep[200:].tolist() == [k for k in d["template"] for _ in range(di.PLANTED_COPIES)]
