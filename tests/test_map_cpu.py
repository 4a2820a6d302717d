"""The read mapper without a GPU: conditions on the shared test inputs (asserted on the CPU oracle alone, so that the GPU
parity test is known to cover every class of read), an invariant of the definition, and the argument errors of
polyhip_map_reads, which are decided before any device call."""
import ctypes as C
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


def test_inputs_cover_every_class():
    d = mi.dataset()
    hits, info = mi.expected("a")
    n, P = len(d["T"]), mi.PARAMS_A
    sampled = hits[:600]
    good = 0
    for h, (a, b, rev) in zip(sampled, d["origin"]):
        good += bool(h.flags & 1) and bool(h.flags & 2) == rev and h.ref_start < b and h.ref_end > a
    print(f"sampled reads mapped {sum(h.flags & 1 for h in sampled)}, on their origin {good}; info {info}")
    assert good >= 540                                                           # 90 % of the 600 sampled reads

    def chosen(h):
        return h.cands[h.best_rank]

    classes = {
        "seed over max_occ": [h for h in hits if h.over],
        "more than one candidate": [h for h in hits if len(h.cands) > 1],
        "best candidate of rank > 0": [h for h in hits if h.flags & 1 and h.best_rank > 0],
        "reverse strand": [h for h in hits if h.flags & 2],
        "clipped at 0": [h for h in hits if h.flags & 1 and chosen(h)[2] - P.band < 0],
        "clipped at n": [h for h in hits if h.flags & 1 and chosen(h)[3] + (h.read_end - h.read_start) + P.band > n
                         and chosen(h)[5] == n],
        "tie": [h for h in hits if h.flags & 1 and h.second == h.score],
        "unmapped": [h for h in hits if not h.flags & 1 and not h.err],
        "err": [h for h in hits if h.err],
    }
    print({k: len(v) for k, v in classes.items()})
    for name, members in classes.items():
        assert members, f"no read of the class '{name}': change map_inputs.SEED"
    sp = d["special"]
    assert hits[sp["short"]].clusters == 0 and not hits[sp["short"]].flags
    assert hits[sp["clip0"]].flags & 1 and hits[sp["clip0"]].cands[hits[sp["clip0"]].best_rank][4] == 0
    assert hits[sp["clipn"]].flags & 1 and hits[sp["clipn"]].cands[hits[sp["clipn"]].best_rank][5] == n
    for name in ("tie_fwd", "tie_rev"):
        h = hits[sp[name]]
        assert len(h.cands) == 3 and h.best_rank == 0 and h.second == h.score == 5 * 150, name
    assert hits[sp["tie_rev"]].flags == 3
    # (every seed of its forward strand is over max_occ; the other strand is T x 120, which the text lacks)
    assert hits[sp["polyA"]].over == len(range(0, 120 - P.seed_len + 1, P.seed_stride)) and hits[sp["polyA"]].clusters == 0
    assert hits[sp["err"]].err == (1 << 8) | ord("N") and hits[sp["err"]].score == 0
    # set (b): the three-copy seeds are all dropped and the cut to max_cand bites
    hits_b, info_b = mi.expected("b")
    assert any(h.clusters > mi.PARAMS_B.max_cand for h in hits_b)
    assert hits_b[sp["tie_fwd"]].clusters == 0 and hits_b[sp["tie_fwd"]].over > 0
    assert all(not h.flags & 2 for h in hits_b)


def test_window_never_beats_the_whole_text():
    """a window is a substring of the text: SmithWaterman over all of T scores at least what the mapper reports"""
    d = mi.dataset()
    hits, _ = mi.expected("a")
    mat = mi.nuc4()
    for i in range(0, 600, 12):
        h, r = hits[i], d["reads"][i]
        q = oracle.reverse_complement(r) if h.flags & 2 else r
        assert oracle.smith_waterman(q, d["T"], mat, mi.GAP)[0] >= h.score, i


def test_oracle_on_a_hand_case():
    """one read worked by hand: text with two copies of a 12-mer, the read = the 12-mer with 4 more bases of the first copy"""
    T = b"TTTTTTTTTT" + b"ACGTACGGTCAG" + b"CCCC" + b"GGGGGGGGGG" + b"ACGTACGGTCAG" + b"TTTT"
    P = mo.Params(seed_len=6, seed_stride=3, max_occ=4, band=2, max_cand=4, both_strands=False, min_score=1)
    (h,), info = mo.map_reads(T, [b"ACGTACGGTCAGCCCC"], mi.nuc4(), mi.GAP, P)
    # seeds at 0, 3, 6, 9: the first three occur in both copies (diagonals 10 and 36), the last only in the first
    assert info == dict(seeds=4, seeds_over_max_occ=0, hits=7, clusters=2, pairs_aligned=2, reads_mapped=1)
    assert [c[:4] for c in h.cands] == [(4, 0, 10, 10), (3, 0, 36, 36)]
    assert (h.score, h.second, h.votes, h.ref_start, h.ref_end, h.read_start, h.read_end) == (80, 60, 4, 10, 26, 0, 16)
    assert h.alignA == h.alignB == b"ACGTACGGTCAGCCCC"


# ---------------------------------------------------------------- the C ABI's argument errors (no device needed)
class _Params(C.Structure):
    _fields_ = [("seed_len", C.c_uint32), ("seed_stride", C.c_uint32), ("max_occ", C.c_uint32), ("band", C.c_uint32),
                ("max_cand", C.c_uint32), ("both_strands", C.c_uint32), ("min_score", C.c_int64)]


def _call(p, max_len=150, dev=False):
    from poly_amd import _lib
    L = _lib.lib()
    null = [None] * 12
    if dev:
        rc = L.polyhip_map_reads_dev(None, None, C.byref(p), None, None, 1, max_len, *null, 0, None, 0, None)
    else:
        rc = L.polyhip_map_reads(None, None, C.byref(p), None, None, 1, max_len, *null, 0)
    return rc, L.polyhip_last_error().decode()


@pytest.mark.parametrize("dev", [False, True])
def test_argument_errors(dev):
    from poly_amd import _lib
    good = dict(seed_len=16, seed_stride=8, max_occ=8, band=16, max_cand=4, both_strands=1, min_score=1)
    for field, bad in [("seed_len", 0), ("seed_stride", 0), ("max_occ", 0), ("max_cand", 0), ("max_cand", 65), ("min_score", 0),
                       ("min_score", -3)]:
        rc, msg = _call(_Params(**{**good, field: bad}), dev=dev)
        assert rc == _lib.ERR_INVALID and field in msg, (field, bad, rc, msg)
    # a bad parameter is named even when the sizes are unsupported and the handles missing
    rc, msg = _call(_Params(**{**good, "max_occ": 0}), max_len=5000, dev=dev)
    assert rc == _lib.ERR_INVALID and "max_occ" in msg
    rc, msg = _call(_Params(**good), dev=dev)
    assert rc == _lib.ERR_INVALID and "null index handle" in msg
    rc, msg = _call(_Params(**good), max_len=4097, dev=dev)
    assert rc == _lib.ERR_UNSUPPORTED and "4097" in msg
    rc, msg = _call(_Params(**good), max_len=4096, dev=dev)
    assert rc == _lib.ERR_INVALID
    rc, msg = _call(_Params(**{**good, "band": 1025}), dev=dev)
    assert rc == _lib.ERR_UNSUPPORTED and "band" in msg
    assert _lib.lib().polyhip_map_workspace_bytes(None, None, C.byref(_Params(**good)), 10, 150) == 0


def test_python_layer_mirrors_the_struct():
    from poly_amd import mapper
    p = mapper.MapParams()
    assert (p.seed_len, p.seed_stride, p.max_occ, p.band, p.max_cand, p.both_strands, p.min_score) == (20, 10, 32, 24, 4, True, 1)
    assert "unmeasured" in mapper.MapParams.__doc__
    assert C.sizeof(mapper._CParams) == 32 and C.sizeof(mapper._CInfo) == 56
    assert [f for f, _ in mapper._CParams._fields_] == [f for f, _ in _Params._fields_]
    assert mapper.last_info()["chunks"] == 0 or isinstance(mapper.last_info()["chunks"], int)
