"""NeedlemanWunsch on the inputs of tests/nw_shapes.py: every pair of every batch equals the CPU oracle in score, err and
both aligned strings (integers and bytes: no tolerance), and every case asserts the kernel that ran -- nw_last_path(),
with the longest A chosen so that the rows-per-lane form is the intended one (nw_shapes.wave_r restates nw_wave_r;
tests/test_nw_shapes_cpu.py asserts the inputs' properties).

  1  register-tiled, <= 64 rows      3  one wave per pair, R = 2 | 3 | 4 | 8 | 16 | 32 | 64 rows per lane for a longest A of
  65..128 | ..192 | ..256 | ..512 | ..1024 | ..2048 | ..4096      2  generic (longer A; POLYHIP_NW_GENERIC=1)

  ladder       both sides of every switch point, A ending in lane 0 / at a lane's last and first row / in lane 63,
               B of 1..190 on both sides of the 64-column reload and of every residue of a packed word
  ties         walks over tied cells (the diagonal wins over a gap move, up over left), gap -1 / 0 / +1
  error order  invalid symbols beyond the first ballot, on both sides, twice in a string, opposite an empty partner
  chunks       polyhip_nw_align_batch_dev in three launches over a workspace of 256 pairs; what it must not touch
  shared B     of 1, 63, 64, 65, 200 symbols, every pair
  int32        scores and gap of +-2^24 with max_lenA + lenB = 127 (H up to 2^31 - 2^24) and the refusal at 128"""
import numpy as np
import pytest

import nw_shapes as ns
from test_align_matrices_gpu import Table, _cmp, _pack, _setenv, check_nw, oracle_nw

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def al():
    from poly_amd import align, alphabet, matrix
    return align, alphabet, matrix


def _table(al, sc: ns.Scoring) -> Table:
    return Table(al, sc.first, sc.second, [list(r) for r in sc.scores], sc.gap)


def _env(generic: bool):
    return {"POLYHIP_NW_GENERIC": "1"} if generic else {}


def _run(al, monkeypatch, sc: ns.Scoring, A, B, generic: bool, want_path: int, shared: bool = False):
    """the host entry point on one batch: every pair equals the oracle, the kernel is the one named"""
    seen = check_nw(al, monkeypatch, _table(al, sc), list(A), list(B), shared=shared, variants=[_env(generic)])
    assert seen == {("nw", want_path)}


# ---- 1. ladder -------------------------------------------------------------------------------------------------------------

LADDER_CASES = [(n, False) for n in ns.LADDER] + [(n, True) for n in ns.LADDER_GENERIC]


@pytest.mark.parametrize("max_a,generic", LADDER_CASES, ids=[f"{n}{'-generic' if g else ''}" for n, g in LADDER_CASES])
def test_ladder(al, monkeypatch, max_a, generic):
    """longest A on both sides of every switch point: path 1 at 64, R = 2 at 65 and 128, 3 at 129 and 192, 4 at 193 and
    256, 8 at 257 and 512, 16 at 513 and 1024, 32 at 1025 and 2048, 64 at 2049 and 4096, path 2 at 4097; the asymmetric
    DNA table with gap -2 and 0 (+1 up to 256 rows), BLOSUM62 above 1024 rows"""
    want = 2 if generic or max_a == 4097 else 1 if max_a == 64 else 3
    assert ns.path(max_a, generic) == want and ns.wave_r(max_a) == ns.LADDER_R[max_a]
    for sc, protein in ns.ladder_scorings(max_a):
        b = ns.ladder(max_a, protein)
        assert b.max_a == max_a
        _run(al, monkeypatch, sc, b.A, b.B, generic, want)


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gap", ns.TIE_GAPS)
@pytest.mark.parametrize("cls", list(ns.TIE_CLASSES))
def test_ties(al, monkeypatch, cls, gap):
    """G = t > d (the diagonal wins a tie with a gap move) and L = left > up (up is tested before the final else) where
    the walk stands on such cells hundreds of times: homopolymers, AC against CA, two-letter strings, indels"""
    max_a, generic = ns.TIE_CLASSES[cls]
    b = ns.ties(cls)
    for match, mismatch in ns.TIE_TABLES:
        _run(al, monkeypatch, ns.simple(match, mismatch, gap), b.A, b.B, generic, ns.path(max_a, generic))


# ---- 3. error order --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", list(ns.ERR_CLASSES))
def test_error_order(al, monkeypatch, cls):
    """err = side << 8 | symbol of the first failing Score() in row-major order, score 0, both strings empty; no error
    opposite an empty partner (score len * gap)"""
    max_a, generic = ns.ERR_CLASSES[cls]
    b, want, what = ns.errors(cls)
    sc = ns.asym(-2)
    _run(al, monkeypatch, sc, b.A, b.B, generic, ns.path(max_a, generic))
    _setenv(monkeypatch, _env(generic))
    score, err, sa, sb = al[0].nw_align_packed(_table(al, sc).sc, *_pack(list(b.A)), *_pack(list(b.B)))
    _setenv(monkeypatch, {})
    for p, (w, name) in enumerate(zip(want, what)):
        assert int(err[p]) == w, f"{name}: err {int(err[p]):#x}, want {w:#x}"
        if w:
            assert (int(score[p]), sa[p], sb[p]) == (0, b"", b""), name
        if name.endswith("no error"):
            assert (int(score[p]), sa[p], sb[p]) == (-2 * max(len(b.A[p]), len(b.B[p])), b"", b""), name


# ---- 4. the device entry point over a workspace of 256 pairs ---------------------------------------------------------------

S64, S32, S8 = -0x5A5A5A5A5A5A5A5B, 0x5A5A5A5A, 0xEE
GUARD = 64


class _Dev:
    """the device buffers of one polyhip_nw_align_batch_dev call, outputs preset to a sentinel, 64 guard entries behind
    score / err / alnLen, one guard row behind alnA / alnB, and the workspace of ALL pairs allocated while the call is
    handed the first `work_bytes` of it: nothing behind those may change"""

    def __init__(self, al, b: ns.Batch, stride: int, work_bytes: int):
        import torch
        self.torch, self.align = torch, al[0]
        dev = torch.device("cuda:0")
        self.n, self.stride, self.max_a, self.max_b = len(b.A), stride, b.max_a, b.max_b
        pa, oa = _pack(list(b.A))
        pb, ob = _pack(list(b.B))
        up = lambda x, dt: torch.from_numpy(x.view(dt)).to(dev)   # noqa: E731
        self.A, self.offA, self.B, self.offB = up(pa, np.uint8), up(oa, np.int64), up(pb, np.uint8), up(ob, np.int64)
        self.score = torch.full((self.n + GUARD,), S64, dtype=torch.int64, device=dev)
        self.err = torch.full((self.n + GUARD,), S32, dtype=torch.int32, device=dev)
        self.len = torch.full((self.n + GUARD,), S32, dtype=torch.int32, device=dev)
        self.alnA = torch.full((self.n + 1, stride), S8, dtype=torch.uint8, device=dev)
        self.alnB = torch.full((self.n + 1, stride), S8, dtype=torch.uint8, device=dev)
        full = self.align.nw_workspace_bytes(self.n, self.max_a, self.max_b)
        self.work = torch.full((max(full, work_bytes),), 0xA5, dtype=torch.uint8, device=dev)
        self.work_bytes = work_bytes

    def call(self, sc, stride=None):
        self.align.nw_align_dev(sc, self.A, self.offA, self.max_a, self.B, self.offB, self.max_b, self.score[:self.n],
                                self.err[:self.n], self.alnA[:self.n, :self.stride if stride is None else stride],
                                self.alnB[:self.n], self.len[:self.n], self.work[:self.work_bytes])
        self.torch.cuda.synchronize()

    def outputs(self):
        return [t.cpu().numpy() for t in (self.score, self.err, self.len, self.alnA, self.alnB)]

    def untouched(self):
        score, err, ln, alnA, alnB = self.outputs()
        assert (score == S64).all() and (err == S32).all() and (ln == S32).all() and (alnA == S8).all() and (alnB == S8).all()
        assert bool((self.work == 0xA5).all())


def _per_pair(align, max_a, max_b):
    per_pair, rest = divmod(align.nw_workspace_bytes(ns.DEV_CHUNK, max_a, max_b) - 256, ns.DEV_CHUNK)
    assert rest == 0 and align.nw_workspace_bytes(ns.DEV_PAIRS, max_a, max_b) == 3 * ns.DEV_CHUNK * per_pair + 256
    return per_pair


@pytest.mark.parametrize("extra", [0, 37], ids=["stride", "stride+37"])
@pytest.mark.parametrize("cls", list(ns.DEV_CLASSES))
def test_three_launches(al, monkeypatch, cls, extra):
    """600 pairs over a workspace of exactly 256 pairs: launches of 256, 256 and 88 pairs, the second and third with
    pair0 > 0.  Every pair equals the oracle; the guards behind score / err / alnLen, the bytes in front of every
    right-aligned string and the bytes behind the workspace handed over keep their sentinel"""
    align = al[0]
    max_a, max_b, generic = ns.DEV_CLASSES[cls]
    b = ns.dev_batch(cls)
    t = _table(al, ns.asym(-2))
    want = oracle_nw(t, list(b.A), list(b.B))
    per_pair = _per_pair(align, max_a, max_b)
    stride = max_a + max_b + extra
    d = _Dev(al, b, stride, ns.DEV_CHUNK * per_pair + 256)
    _setenv(monkeypatch, _env(generic))
    d.call(t.sc)
    _setenv(monkeypatch, {})
    assert align.nw_last_path() == ns.path(max_a, generic)
    score, err, ln, alnA, alnB = d.outputs()
    n = d.n
    assert (ln[:n].astype(np.int64) <= max_a + max_b).all()
    got = [(int(score[p]), int(err[p]), alnA[p, stride - int(ln[p]):].tobytes(), alnB[p, stride - int(ln[p]):].tobytes())
           for p in range(n)]
    _cmp(f"{cls}, three launches", got, want)
    assert (score[n:] == S64).all() and (err[n:] == S32).all() and (ln[n:] == S32).all()
    front = np.arange(stride)[None, :] < (stride - ln[:n].astype(np.int64))[:, None]
    assert (alnA[:n][front] == S8).all() and (alnB[:n][front] == S8).all(), "bytes in front of a string were written"
    assert (alnA[n] == S8).all() and (alnB[n] == S8).all()
    behind = d.work[d.work_bytes:]
    assert behind.numel() == 2 * ns.DEV_CHUNK * per_pair and bool((behind == 0xA5).all()), "the call wrote behind its workspace"


@pytest.mark.parametrize("cls", list(ns.DEV_CLASSES))
def test_refusals_leave_the_outputs_alone(al, monkeypatch, cls):
    """a workspace one byte short of 256 pairs and a stride of max_lenA + lenB - 1: POLYHIP_ERR_INVALID with the
    entry point's message, nothing written"""
    from poly_amd import _lib
    align = al[0]
    max_a, max_b, generic = ns.DEV_CLASSES[cls]
    b = ns.dev_batch(cls)
    t = _table(al, ns.asym(-2))
    per_pair = _per_pair(align, max_a, max_b)
    _setenv(monkeypatch, _env(generic))
    short = ns.DEV_CHUNK * per_pair - 1
    d = _Dev(al, b, max_a + max_b, short)
    with pytest.raises(_lib.PolyhipError) as e:
        d.call(t.sc)
    assert e.value.status == ERR_INVALID
    assert e.value.message == f"polyhip_nw_align_batch: workspace too small ({short} B; {per_pair} B per pair, >= 256 pairs)"
    d.untouched()
    d = _Dev(al, b, max_a + max_b, ns.DEV_CHUNK * per_pair + 256)
    with pytest.raises(_lib.PolyhipError) as e:
        d.call(t.sc, stride=max_a + max_b - 1)
    assert e.value.status == ERR_INVALID
    assert e.value.message == f"polyhip_nw_align_batch: aln_stride {max_a + max_b - 1} < max_lenA + lenB"
    d.untouched()
    _setenv(monkeypatch, {})


# ---- 5. shared B -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", list(ns.SHARED_CLASSES))
def test_shared_b(al, monkeypatch, cls):
    """one B of 1, 63, 64, 65 and 200 symbols for every read, and one with an invalid symbol at index 64: every pair"""
    max_a, generic = ns.SHARED_CLASSES[cls]
    A, Bs = ns.shared(cls)
    for gap in (-2, 0):
        for shared_b in Bs:
            _run(al, monkeypatch, ns.asym(gap), A, [shared_b], generic, ns.path(max_a, generic), shared=True)
    # the invalid symbol of the shared B is named for every read that has symbols and a valid first one
    _setenv(monkeypatch, _env(generic))
    _, err, _, _ = al[0].nw_align_packed(_table(al, ns.asym(-2)).sc, *_pack(list(A)), np.frombuffer(Bs[5], np.uint8).copy(), None)
    _setenv(monkeypatch, {})
    assert [int(e) for e in err] == [0 if not a else (1 << 8) | a[0] if a[0] not in ns.DNA else (2 << 8) | ord("N") for a in A]


# ---- 6. the int32 guard ----------------------------------------------------------------------------------------------------

def test_scoring_range(al):
    """polyhip_scoring_create takes |score| and |gap| up to 2^24"""
    from poly_amd import _lib
    for sc in (ns.simple(ns.BIG, -ns.BIG, -ns.BIG), ns.simple(ns.BIG, -ns.BIG, ns.BIG)):
        assert _table(al, sc).sc.handle()
    for sc in (ns.simple(ns.BIG + 1, -1, -1), ns.simple(1, -ns.BIG - 1, -1), ns.simple(1, -1, ns.BIG + 1), ns.simple(1, -1, -ns.BIG - 1)):
        with pytest.raises(_lib.PolyhipError) as e:
            _table(al, sc).sc.handle()
        assert e.value.status == ERR_UNSUPPORTED and "exceeds 2^24" in e.value.message


@pytest.mark.parametrize("gap", [-ns.BIG, ns.BIG], ids=["gap-2^24", "gap+2^24"])
@pytest.mark.parametrize("cls", list(ns.GUARD_CASES))
def test_next_to_the_int32_limit(al, monkeypatch, cls, gap):
    """max|score| * (max_lenA + lenB) = 2^31 - 2^24: accepted, and equal to the oracle's 64-bit matrix"""
    max_a, max_b, generic = ns.GUARD_CASES[cls]
    b = ns.guard_batch(max_a, max_b)
    _run(al, monkeypatch, ns.big(gap), b.A, b.B, generic, ns.path(max_a, generic))


@pytest.mark.parametrize("max_a,max_b", ns.GUARD_REFUSED)
@pytest.mark.parametrize("generic", [False, True], ids=["default", "generic"])
def test_at_the_int32_limit(al, monkeypatch, max_a, max_b, generic):
    """max|score| * (max_lenA + lenB) = 2^31: POLYHIP_ERR_UNSUPPORTED"""
    from poly_amd import _lib
    b = ns.guard_batch(max_a, max_b)
    _setenv(monkeypatch, _env(generic))
    for gap in (-ns.BIG, ns.BIG):
        with pytest.raises(_lib.PolyhipError) as e:
            al[0].nw_align_packed(_table(al, ns.big(gap)).sc, *_pack(list(b.A)), *_pack(list(b.B)))
        assert e.value.status == ERR_UNSUPPORTED and "could overflow int32" in e.value.message
    _setenv(monkeypatch, {})
