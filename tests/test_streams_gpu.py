"""Every device entry point of include/polyhip.h on a NON-DEFAULT stream (tests/stream_harness.py).

The parity tests of the other modules pin every kernel's arithmetic, all on torch's default stream, where the stream
itself orders the work and no ordering mistake of the library can show.  Here each call runs on a non-blocking side
stream behind a delay, with a decoy in its inputs until the true input arrives on that stream, and is compared with the
same CPU oracle its parity test uses.  COVERED lists the entry points; tests/test_streams_cpu.py checks it against the
header, so a new device entry point cannot arrive without a stream case.

Entry points the header calls asynchronous must return while the delay is still in flight; those it documents as
synchronising `stream` are listed in SYNCHRONISING and are checked for the opposite: their outputs are final on return.
"""
import concurrent.futures as cf
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import bwt_oracle as bo  # noqa: E402
import map_inputs as mi  # noqa: E402
import mash_neighbors_oracle as nbo  # noqa: E402
import oracle as orc  # noqa: E402
import stream_harness as sh  # noqa: E402
from oracle import fasta_ref, fastq_ref  # noqa: E402

pytestmark = pytest.mark.gpu

# every function of include/polyhip.h with a polyhip_stream_t parameter, and the three stream-less _dev read-backs
COVERED = [
    "polyhip_synth_dna_dev", "polyhip_mash_sketch_batch_dev",
    "polyhip_mash_shared_counts_dev", "polyhip_mash_index_build_dev", "polyhip_mash_shared_counts_reuse_dev",
    "polyhip_mash_index_build_part_dev", "polyhip_mash_index_part_spans", "polyhip_mash_index_finalize_dev",
    "polyhip_mash_index_format_dev", "polyhip_mash_index_build_info_dev", "polyhip_mash_shared_counts_mode_dev",
    "polyhip_mash_index_allgather_dev", "polyhip_mash_distance_from_counts_dev", "polyhip_mash_neighbors_dev",
    "polyhip_sw_batch_dev", "polyhip_sw_traceback_dev", "polyhip_sw_align_batch_dev", "polyhip_nw_align_batch_dev",
    "polyhip_santalucia_scan_dev", "polyhip_santalucia_scan_first_dev", "polyhip_santalucia_batch_dev",
    "polyhip_marmurdoty_batch_dev", "polyhip_least_rotation_batch_dev", "polyhip_seqhash_batch_dev",
    "polyhip_fastq_pack_dev", "polyhip_fasta_pack_dev",
    "polyhip_bwt_create_dev", "polyhip_bwt_transform_dev", "polyhip_bwt_count_dev", "polyhip_bwt_locate_dev",
    "polyhip_bwt_extract_dev", "polyhip_map_reads_dev",
    "polyhip_allgather_sketches_dev", "polyhip_allgatherv_dev",
]
# ... of which the header says that they synchronise `stream` (the sketch only with SketchSize < 2)
SYNCHRONISING = ["polyhip_mash_index_build_part_dev", "polyhip_mash_index_part_spans", "polyhip_mash_index_allgather_dev",
                 "polyhip_mash_neighbors_dev", "polyhip_bwt_create_dev", "polyhip_map_reads_dev"]

S32 = sh.SENTINEL32
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def delay(dev):
    """calibrated once per module to about 50 ms (the criterion is the in-flight query of every asynchronous case)"""
    d = sh.Delay(dev, 50.0)
    print(f"stream delay: {'_sleep' if d.cycles else 'elementwise chain'}, measured {d.measured_ms:.1f} ms")
    return d


@pytest.fixture(scope="module")
def nuc4():
    """one scoring handle for every alignment case of the module (created here: its creation copies with blocking calls)"""
    from poly_amd import align, alphabet, matrix
    a = alphabet.NewAlphabet(list("-ACGT"))
    sc = align.NewScoring(matrix.NewSubstitutionMatrix(a, a, matrix.NUC_4), -2)
    sc.handle()
    return sc


def _om():
    return orc.SubstitutionMatrix("-ACGT", "-ACGT", orc.NUC_4_SCORES)


def _pack(seqs):
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), np.uint8).copy(), offs


def _dna(rng, n) -> bytes:
    return ACGT[rng.integers(0, 4, n)].tobytes()


def _threads(fn, items):
    with cf.ThreadPoolExecutor(16) as ex:  # (the oracle's C calls release the GIL)
        return list(ex.map(fn, items))


def _b(x) -> bytes:
    return x if isinstance(x, bytes) else x.encode("latin-1")


# ---------------------------------------------------------------- the harness itself
def test_harness_can_fail_and_streams_are_not_serialised(delay):
    """FIRST: a fill queued behind the delay on a side stream is invisible to the default stream.  If this fails, the
    runtime orders the streams behind our back and no other test of this file means anything."""
    sh.self_test(delay)


# ---------------------------------------------------------------- synthetic input, K1
def test_synth_dna(dev, delay):
    import torch
    from poly_amd import mash
    n = 200_003
    c = sh.Case(dev, "synth_dna_dev")
    out = c.out((n,), torch.uint8)
    c.call = lambda st: mash.synth_dna_dev(0xD1, out, first=64, stream=st)
    r = sh.run(c, delay)
    assert (r.outs[0] == orc.synth_dna(0xD1, n + 64)[64:]).all()


def _sketch_case(dev, reads, decoy, k, s, name):
    """-> (case, check): polyhip_mash_sketch_batch_dev; the rows' prior state is the harness's sentinel"""
    import torch
    from poly_amd import mash
    bt, ot = _pack(reads)
    bd, od = _pack(decoy)
    n = len(reads)
    c = sh.Case(dev, name)
    seqs, offs = c.inp(bt, bd), c.inp(ot, od)
    out = c.out((n, s), torch.int32)
    c.call = lambda st: mash.sketch_batch_dev(seqs, offs, k, s, out, stream=st)
    want = orc.mash_sketch_batch(bt, ot, k, s, out=np.full((n, s), S32, np.uint32))

    def check(r):
        got = r.outs[0].view(np.uint32)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, f"{name}: rows {bad[:8]} differ from the oracle ({bad.size} rows)"
    return c, check


def _slab_reads(seed):
    k, s = 21, 1000
    lens = [10_000] * 64 + [0, k, k + s - 1]
    if seed & 1:
        lens = lens[::-1]
    g = orc.synth_dna(seed, sum(lens)).tobytes()
    o = np.concatenate([[0], np.cumsum(lens)])
    return [g[o[i]:o[i + 1]] for i in range(len(lens))]


def _tiny_reads(seed, k=21):
    """reads whose FIRST window holds the least hash: SketchSize 1 then panics on none of them (mash.go:98)"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < 40:
        L = int(rng.integers(k + 2, 400))
        r = np.frombuffer(_dna(rng, L), np.uint8)
        h = orc.mash_sketch_batch(r, np.array([0, L], np.uint64), k, L)[0][:L - k]  # fewer windows than s: positional
        out.append(r[int(np.argmin(h)):].tobytes())
    return out


def test_sketch_slab_and_general_kernels(dev, delay):
    """64 reads of 10 kb (the slab kernel) and lengths 0, k and k + s - 1 (the general kernel's rows)"""
    c, check = _sketch_case(dev, _slab_reads(0xA0), _slab_reads(0xA1), 21, 1000, "sketch_batch_dev k=21 s=1000")
    check(sh.run(c, delay))


def test_sketch_wide_kernel_stream_ordered_scratch(dev, delay):
    """SketchSize 10,000: the wide kernel, candidates in a hipMallocAsync / hipFreeAsync scratch on the caller's stream"""
    reads = [orc.synth_dna(0xB0 + i, 30_000).tobytes() for i in range(4)]
    decoy = [orc.synth_dna(0xB8 + i, 30_000).tobytes() for i in range(4)]
    c, check = _sketch_case(dev, reads, decoy, 21, 10_000, "sketch_batch_dev s=10000")
    check(sh.run(c, delay))


def _sketch_tiny_case(dev):
    reads = _tiny_reads(6)
    return _sketch_case(dev, reads, reads[::-1], 21, 1, "sketch_batch_dev s=1")


def test_sketch_size_one_synchronising_path(dev, delay):
    """SketchSize 1: the verdict comes from the device, through a stream-ordered allocation of its own"""
    c, check = _sketch_tiny_case(dev)
    check(sh.run(c, delay, asynchronous=False))


# ---------------------------------------------------------------- K2
def _mixed_sketches(seed, n=640, s=96):
    """the sets of test_stress_gpu.py::test_distance_mixed_sets, irregular rows included"""
    rng = np.random.default_rng(seed)
    base = [np.sort(rng.integers(0, 1 << 32, s, dtype=np.uint32)) for _ in range(40)]
    X = []
    for i in range(n):
        b = base[i % 40].copy()
        b[rng.integers(0, s, int(rng.integers(0, 30)))] = rng.integers(0, 1 << 32, 1, dtype=np.uint32)
        b.sort()
        if i % 97 == 0:
            rng.shuffle(b)          # unsorted
        if i % 131 == 0:
            b[s // 2:] = 0          # zero tail
        if i % 53 == 0:
            b[:] = b[0]             # one repeated hash
        X.append(b)
    return np.stack(X)


@functools.lru_cache(maxsize=None)
def _k2():
    """X (128 x 96), Y (512 x 96), their decoys and every pair's orc.mash_shared; callers leave it unchanged"""
    S, D = _mixed_sketches(77), _mixed_sketches(78)
    X, Y = np.ascontiguousarray(S[:128]), np.ascontiguousarray(S[128:])
    want = np.array([[orc.mash_shared(x, y) for y in Y] for x in X], np.uint16)
    assert not nbo.is_ascending(X) and not nbo.is_ascending(Y)
    return X, Y, np.ascontiguousarray(D[:128]), np.ascontiguousarray(D[128:]), want


def _k2_case(dev, name):
    import torch
    from poly_amd import mash
    X, Y, Xd, Yd, want = _k2()
    c = sh.Case(dev, name)
    c.Yt = c.inp(Y, Yd)
    c.Xt = c.inp(X, Xd, after_setup=True)
    c.counts = c.out(want.shape, torch.int16)
    c.wk = c.work(mash.shared_counts_workspace_bytes(128, 96, 512, 96))

    def check(r):
        got = r.outs[0].view(np.uint16)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{name}: {len(bad)} pairs differ from orc.mash_shared, first {bad[0]}"
    return c, check


def test_shared_counts(dev, delay):
    from poly_amd import mash
    c, check = _k2_case(dev, "shared_counts_dev")
    c.call = lambda st: mash.shared_counts_dev(c.Xt, c.Yt, c.counts, c.wk, stream=st)
    check(sh.run(c, delay))


def test_index_build_then_reuse(dev, delay):
    """index_build_dev is the setup call on the side stream: Y is true before it, X and the counts change after it"""
    from poly_amd import mash
    c, check = _k2_case(dev, "index_build_dev + shared_counts_reuse_dev")
    c.setup = lambda st: mash.index_build_dev(c.Yt, c.wk, stream=st)
    c.call = lambda st: mash.shared_counts_reuse_dev(c.Xt, c.Yt, c.counts, c.wk, stream=st)
    check(sh.run(c, delay))


def test_index_build_alone_is_asynchronous(dev, delay):
    """... and index_build_dev as the call under test (the join behind it proves the index)"""
    from poly_amd import mash
    c, check = _k2_case(dev, "index_build_dev")

    def call(st):
        mash.index_build_dev(c.Yt, c.wk, stream=st)
        mash.shared_counts_reuse_dev(c.Xt, c.Yt, c.counts, c.wk, stream=st)
    c.call = call
    check(sh.run(c, delay))


def _parts_case(dev, name):
    """two index parts as the setup (each synchronises the stream once); `head` keeps the index's header words"""
    import torch
    from poly_amd import mash
    c, check = _k2_case(dev, name)
    c.head = c.out((128,), torch.uint8)

    def setup(st):
        mash.index_build_part_dev(c.Yt, 0, 2, c.wk, stream=st)
        mash.index_build_part_dev(c.Yt, 1, 2, c.wk, stream=st)
    c.setup = setup
    return c, check


def _default_stream_index(dev, nparts=1):
    """the workspace with the index of the true Y built on the default stream -- in one piece, or in `nparts` parts
    without the finalize -- and fully synchronised"""
    import torch
    from poly_amd import mash
    Yt = torch.from_numpy(_k2()[1].view(np.int32)).to(dev)
    wk = torch.zeros(mash.shared_counts_workspace_bytes(128, 96, 512, 96), dtype=torch.uint8, device=dev)
    if nparts == 1:
        mash.index_build_dev(Yt, wk)
    for p in range(nparts if nparts > 1 else 0):
        mash.index_build_part_dev(Yt, p, nparts, wk)
    torch.cuda.synchronize()
    return wk


def test_index_parts_then_finalize(dev, delay):
    """index_build_part_dev x 2 (setup), index_finalize_dev + the join (under test): every pair against the oracle, the
    self-join size finalize recomputes against the one-shot index's, as tests/test_comm_gpu.py compares it"""
    import torch
    from poly_amd import mash
    c, check = _parts_case(dev, "index_build_part_dev x 2 + index_finalize_dev")

    def call(st):
        mash.index_finalize_dev(512, 96, c.wk, stream=st)
        c.head.copy_(c.wk[:128])
        mash.shared_counts_reuse_dev(c.Xt, c.Yt, c.counts, c.wk, stream=st)
    c.call = call
    r = sh.run(c, delay)
    check(r)
    head = torch.from_numpy(r.outs[1].copy()).to(dev)
    assert mash.shared_counts_mode(head)[4] == mash.shared_counts_mode(_default_stream_index(dev))[4] > 0


def test_distance_from_counts(dev, delay):
    import torch
    from poly_amd import mash
    want = _k2()[4]
    rng = np.random.default_rng(3)
    c = sh.Case(dev, "distance_from_counts_dev")
    ct = c.inp(want, rng.integers(0, 97, want.shape).astype(np.uint16))
    dist = c.out(want.shape, torch.float64)
    c.call = lambda st: mash.distance_from_counts_dev(ct, 96, 96, dist, stream=st)
    r = sh.run(c, delay)
    expect = 1 - want.astype(np.float64) / np.float64(96)   # mash.go:134,139
    assert (r.outs[0].view(np.uint64) == expect.view(np.uint64)).all()


def test_streamless_readbacks_wait_for_the_side_stream(dev, delay):
    """polyhip_mash_index_format_dev, _index_build_info_dev and _shared_counts_mode_dev right after a build + join was
    enqueued on the side stream, with no synchronisation by the test: the values read after s.synchronize(), and the
    irregular-sketch counts of the true sets (a copy that does not wait sees the 0xA5 workspace, or the decoy's index)"""
    from poly_amd import mash
    X, Y = _k2()[:2]
    c, check = _k2_case(dev, "read-backs")

    def read():
        return mash.index_item_bytes(c.wk), mash.index_build_info(c.wk), mash.shared_counts_mode(c.wk)

    def call(st):
        mash.shared_counts_dev(c.Xt, c.Yt, c.counts, c.wk, stream=st)
        at_once = read()
        st.synchronize()
        return at_once, read()
    c.call = call
    r = sh.run(c, delay, asynchronous=False)
    check(r)
    at_once, after = r.ret
    assert at_once == after, f"read-backs before the stream was synchronised {at_once} differ from those after it {after}"
    irr = lambda S: int(sum(not nbo.is_ascending(x) for x in S))  # noqa: E731
    assert after[0] in (4, 8) and after[1]["build"] in (0, 1, 2) and after[2][0] in (0, 1)
    assert after[2][1:3] == (irr(X), irr(Y))


def _neighbors_case(dev):
    """the smallest Y that takes two column blocks (one dense stripe holds 113,496 sketches of 16 hashes: 250,000 of
    test_mash_neighbors_gpu.py::test_wide_y_goes_in_column_blocks take three), neighbours on both sides of the boundary"""
    import torch
    from poly_amd import mash
    ny, s, cap = 120_000, 16, 4096

    def sets(seed):
        rng = np.random.default_rng(seed)
        Y = np.sort(rng.integers(0, 1 << 31, (ny, s), dtype=np.uint32), axis=1)
        X = Y[[5, 60_000, 113_400, 113_600, 119_999, 77]].copy()
        for r, cols in {0: [7, 113_495, 113_496, 119_998], 1: [113_497, 3], 3: [0, 113_494]}.items():
            for q, j in enumerate(cols):
                Y[j, :8 + q] = X[r, :8 + q]
                Y[j].sort()
        return X, Y
    X, Y = sets(31)
    Xd, Yd = sets(32)
    c = sh.Case(dev, "neighbors_dev")
    Xt, Yt = c.inp(X, Xd), c.inp(Y, Yd)
    first = c.out((len(X) + 1,), torch.int64)
    cols, shared, dist = c.out((cap,), torch.int32), c.out((cap,), torch.int16), c.out((cap,), torch.float64)
    wk = c.work(mash.neighbors_workspace_bytes(len(X), s, ny, s))
    c.call = lambda st: mash.neighbors_dev(Xt, Yt, first, cols, shared, dist, wk, min_shared=1, k=0, stream=st)
    want = nbo.neighbors_from_counts(nbo.shared_matrix_ascending(X, Y), s, s)

    def check(r):
        n = int(want[0][-1])
        assert 8 < n <= cap
        nbo.assert_same((r.outs[0].view(np.uint64), r.outs[1].view(np.uint32)[:n], r.outs[2].view(np.uint16)[:n], r.outs[3][:n]),
                        want, "neighbors_dev on a side stream")
        assert (r.outs[1][n:] == np.int32(S32)).all(), "written beyond the list"
        assert mash.neighbors_last_info()["column_blocks"] == 2
    return c, check


def test_neighbors_two_column_blocks(dev, delay):
    c, check = _neighbors_case(dev)
    check(sh.run(c, delay, asynchronous=False))


# ---------------------------------------------------------------- K3: SmithWaterman, NeedlemanWunsch
def _mutated_windows(rng, ref: bytes, n, L, sub=0.05):
    r = np.frombuffer(ref, np.uint8)
    reads = r[rng.integers(0, len(r) - L, n)[:, None] + np.arange(L)].copy()
    hit = rng.random(reads.shape) < sub
    reads[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    return reads


@functools.lru_cache(maxsize=None)
def _sw_inputs(kind):
    """(reads, refs | one reference, decoy reads, decoy refs | reference) of the three score-pass shapes"""
    def make(seed):
        rng = np.random.default_rng(seed)
        if kind == "packed":      # 4096 reads of 150 against one reference of 1000
            ref = _dna(rng, 1000)
            reads = _mutated_windows(rng, ref, 4096, 150)
            reads[::64] = ACGT[rng.integers(0, 4, (64, 150))]        # unrelated reads
            return [x.tobytes() for x in reads], ref
        if kind == "chunks":      # 3072 reads of 150 against 1000: the traceback workspace holds a third
            ref = _dna(rng, 1000)
            return [x.tobytes() for x in _mutated_windows(rng, ref, 3072, 150)], ref
        if kind == "pair":        # 2000 pairs of 150 x 150, every pair its own B
            A = ACGT[rng.integers(0, 4, (2000, 150))]
            B = A.copy()
            hit = rng.random(B.shape) < 0.08
            B[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
            B[::50] = ACGT[rng.integers(0, 4, (40, 150))]
            return [x.tobytes() for x in A], [np.roll(x, int(rng.integers(0, 20))).tobytes() for x in B]
        if kind == "pair64":      # 2000 pairs of 64 x 90: at most 64 rows, the register-tiled kernel for per-pair B
            A = ACGT[rng.integers(0, 4, (2000, 64))]
            B = ACGT[rng.integers(0, 4, (2000, 90))]
            B[:, 13:77] = A
            hit = rng.random(B.shape) < 0.08
            B[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
            return [x.tobytes() for x in A], [x.tobytes() for x in B]
        ref = _dna(rng, 900)      # "wave": 48 reads of 300..600 against 900, one wave per pair
        lens = np.linspace(300, 600, 48).astype(int)
        if seed & 1:
            lens = lens[::-1]
        return [_mutated_windows(rng, ref, 1, int(L), 0.06)[0].tobytes() for L in lens], ref
    seed = {"packed": 10, "chunks": 20, "pair": 30, "wave": 40, "pair64": 44}[kind]
    return make(seed) + make(seed + 1)


@functools.lru_cache(maxsize=None)
def _sw_oracle(kind):
    """orc.smith_waterman of every pair: [(score, alignA, alignB, endA, endB)]; callers leave it unchanged"""
    A, B = _sw_inputs(kind)[:2]
    om = _om()
    pairs = list(zip(A, B if isinstance(B, list) else [B] * len(A)))
    return _threads(lambda ab: orc.smith_waterman(ab[0], ab[1], om, -2), pairs)


def _sw_case(dev, sc, A, B, Ad, Bd, which, name, tb_pairs=None):
    """which: 'batch' = sw_batch_dev; 'traceback' = sw_batch_dev as the setup call, then sw_traceback_dev on its outputs;
    'align' = sw_align_dev.  tb_pairs: pairs the traceback workspace is sized for (default: all)"""
    import torch
    from poly_amd import align
    shared = not isinstance(B, list)
    pa, oa = _pack(A)
    pad, oad = _pack(Ad)
    n, maxA = len(A), max(len(a) for a in A)
    c = sh.Case(dev, name)
    At, offA = c.inp(pa, pad), c.inp(oa, oad)
    if shared:
        Bt, offB, lenB = c.inp(np.frombuffer(B, np.uint8), np.frombuffer(Bd, np.uint8)), None, len(B)
    else:
        pb, ob = _pack(B)
        pbd, obd = _pack(Bd)
        Bt, offB, lenB = c.inp(pb, pbd), c.inp(ob, obd), max(len(b) for b in B)
    res = c.mid if which == "traceback" else c.out
    score = res((n,), torch.int64)
    ea, eb, er = (res((n,), torch.int32) for _ in range(3))
    wk = c.work(align.sw_workspace_bytes(sc, n, maxA, lenB, shared))
    stride = align.sw_traceback_stride(sc, maxA, lenB)
    if which != "batch":
        alnA, alnB = c.out((n, stride), torch.uint8), c.out((n, stride), torch.uint8)
        ln = c.out((n,), torch.int32)
        tbw = c.work(align.sw_traceback_workspace_bytes(sc, tb_pairs or n, maxA, lenB))

    def batch(st):
        align.sw_batch_dev(sc, At, offA, maxA, Bt, offB, lenB, score, ea, eb, er, wk, stream=st)
    if which == "batch":
        c.call = batch
    elif which == "traceback":
        c.setup = batch
        c.call = lambda st: align.sw_traceback_dev(sc, At, offA, maxA, Bt, offB, lenB, ea, eb, er, alnA, alnB, ln, tbw,
                                                   stream=st, score_t=score)
    else:
        c.call = lambda st: align.sw_align_dev(sc, At, offA, maxA, Bt, offB, lenB, score, ea, eb, er, alnA, alnB, ln, wk,
                                               tbw, stream=st)
    c.stride = stride
    return c


def _sw_check(r, which, want, stride, name, sample=None):
    """score, end cell and error of every pair (of `sample`), and both strings, against the oracle's tuples"""
    o = r.outs
    if which == "batch":
        score, ea, eb, er = o[:4]
    elif which == "traceback":
        alnA, alnB, ln, score, ea, eb, er = o      # (the setup call's tensors are cloned behind the outputs)
    else:
        score, ea, eb, er, alnA, alnB, ln = o
    idx = range(len(score)) if sample is None else sample
    for p, w in zip(idx, want):
        assert (int(score[p]), int(ea[p]), int(eb[p]), int(er[p])) == (w[0], w[3], w[4], 0), \
            f"{name}: pair {p}: score / end cell {(int(score[p]), int(ea[p]), int(eb[p]), int(er[p]))}, oracle {(w[0], w[3], w[4])}"
        if which != "batch":
            L = int(ln[p])
            got = (alnA[p, stride - L:].tobytes(), alnB[p, stride - L:].tobytes())
            assert got == (_b(w[1]), _b(w[2])), f"{name}: pair {p}: aligned strings differ from the oracle"


# the score pass each shape takes by sw_batch.hip's choose() (polyhip_sw_last_path): 4096 reads are fewer than the 49,152
# from which the packed pass is taken (the one-wave-per-pair kernel for small batches, 4; the packed pass itself runs on
# a side stream in the three tests on _fork_inputs() below and in test_score_pass_split_into_sub_batches); per-pair B
# takes the register-tiled kernel (5) up to 64 rows and the one-wave-per-pair kernel (6) beyond
SW_PATHS = {"packed": 4, "pair": 6, "pair64": 5, "wave": 6}


@pytest.mark.parametrize("which", ["batch", "traceback", "align"])
@pytest.mark.parametrize("kind", ["packed", "pair", "pair64", "wave"])
def test_smith_waterman(dev, delay, nuc4, kind, which):
    """sw_batch_dev, sw_traceback_dev and sw_align_dev: 4096 reads of 150 against one reference of 1000, 2000 pairs of
    150 x 150 and of 64 x 90 with per-pair B, 48 reads of 300..600 against 900 (one wave per pair); every pair"""
    from poly_amd import align
    A, B, Ad, Bd = _sw_inputs(kind)
    name = f"sw {which} ({kind})"
    c = _sw_case(dev, nuc4, A, B, Ad, Bd, which, name)
    r = sh.run(c, delay)
    assert align.last_path() == SW_PATHS[kind]
    _sw_check(r, which, _sw_oracle(kind), c.stride, name)


def _live(aln, ln):
    """the string bytes of every slot (right-aligned), the rest zeroed"""
    stride = aln.shape[1]
    return np.where(np.arange(stride)[None, :] >= (stride - ln.astype(np.int64))[:, None], aln, 0)


def _same_strings(a, b, what):
    assert (a.outs[2] == b.outs[2]).all(), f"{what}: string lengths differ"
    for q in (0, 1):
        assert (_live(a.outs[q], a.outs[2]) == _live(b.outs[q], b.outs[2])).all(), f"{what}: strings differ"
    for q in range(3, 7):
        assert (a.outs[q] == b.outs[q]).all()


def test_traceback_workspace_for_a_third_of_the_batch(dev, delay, nuc4, monkeypatch):
    """3072 pairs of 150 against 1000 through a traceback workspace sized for a third of them: the call loops over
    chunks on the caller's stream (1024 pairs per chunk are below the 2 x 16,384 at which the library forks, see the next
    test).  Equal to the POLYHIP_TB_OVERLAP=0 run and, every pair, to the oracle."""
    A, B, Ad, Bd = _sw_inputs("chunks")
    c = _sw_case(dev, nuc4, A, B, Ad, Bd, "traceback", "traceback in chunks", tb_pairs=1024)
    r = sh.run(c, delay)
    _sw_check(r, "traceback", _sw_oracle("chunks"), c.stride, "traceback in chunks")
    monkeypatch.setenv("POLYHIP_TB_OVERLAP", "0")
    _same_strings(r, sh.run(c, delay), "chunks vs POLYHIP_TB_OVERLAP=0")


FORK_N, FORK_TB_PAIRS = 98_304, 33_280


@functools.lru_cache(maxsize=None)
def _fork_inputs():
    """98,304 reads of 150 against 1000 and a traceback workspace for 33,280 of them: the batch does not fit, and half the
    workspace holds 16,640 >= 16,384 pairs -- the smallest shape class at which traceback_impl forks its chunks onto the
    library's second stream (six chunks, alternating).  Oracle: every 101st pair."""
    def make(seed):
        rng = np.random.default_rng(seed)
        ref = _dna(rng, 1000)
        return [x.tobytes() for x in _mutated_windows(rng, ref, FORK_N, 150)], ref
    A, B = make(50)
    Ad, Bd = make(51)
    sample = list(range(0, FORK_N, 101))
    om = _om()
    want = _threads(lambda p: orc.smith_waterman(A[p], B, om, -2), sample)
    return A, B, Ad, Bd, sample, want


def test_traceback_chunks_alternate_between_caller_and_library_stream(dev, delay, nuc4, monkeypatch):
    """the chunks alternate between the side stream and the library's second stream, forked and joined by events: equal
    to the POLYHIP_TB_OVERLAP=0 run (all pairs) and to the oracle (a sample)"""
    A, B, Ad, Bd, sample, want = _fork_inputs()
    from poly_amd import align
    c = _sw_case(dev, nuc4, A, B, Ad, Bd, "traceback", "traceback on two streams", tb_pairs=FORK_TB_PAIRS)
    r = sh.run(c, delay)
    assert (align.last_path(), align.sw_traceback_last_path()) == (3, 1)   # the packed score pass is the setup call
    _sw_check(r, "traceback", want, c.stride, "traceback on two streams", sample)
    monkeypatch.setenv("POLYHIP_TB_OVERLAP", "0")
    _same_strings(r, sh.run(c, delay), "two streams vs POLYHIP_TB_OVERLAP=0")


def test_packed_pass_and_fused_align(dev, delay, nuc4):
    """sw_align_dev on the same 98,304 reads with the whole traceback workspace: the packed two-pairs-per-lane score pass
    (path 3) leaves the end cells to the byte-profile traceback kernel (path 1)"""
    from poly_amd import align
    A, B, Ad, Bd, sample, want = _fork_inputs()
    c = _sw_case(dev, nuc4, A, B, Ad, Bd, "align", "fused align, packed pass")
    r = sh.run(c, delay)
    assert (align.last_path(), align.sw_traceback_last_path()) == (3, 1)
    _sw_check(r, "align", want, c.stride, "fused align, packed pass", sample)


def test_five_caller_streams_in_one_thread(dev, delay, nuc4):
    """the two-stream traceback once on each of five distinct side streams, one after the other on this thread: the
    library keeps four second streams per thread, keyed by the caller's, so the fifth recycles an entry whose key is
    another live stream"""
    import torch
    A, B, Ad, Bd, sample, want = _fork_inputs()
    c = _sw_case(dev, nuc4, A, B, Ad, Bd, "traceback", "traceback, five caller streams", tb_pairs=FORK_TB_PAIRS)
    streams = [torch.cuda.Stream() for _ in range(5)]
    assert len({s.cuda_stream for s in streams}) == 5
    first = None
    for q, s in enumerate(streams):
        r = sh.run(c, delay, stream=s, warm=(q == 0))
        _sw_check(r, "traceback", want, c.stride, f"caller stream {q}", sample)
        if first is None:
            first = r
        else:
            _same_strings(first, r, f"caller stream {q} vs caller stream 0")


def test_score_pass_split_into_sub_batches(dev, delay, nuc4, monkeypatch):
    """524,288 reads of 150 against 5000 (workloads.config4_reads): path 3 runs them as two sub-batches, the second forked
    onto the library's stream.  All four outputs equal the POLYHIP_SW_OVERLAP=0 run of the same batch on the default
    stream (test_align_gpu.py::test_device_resident_config4_sample pins that path to the oracle), and 200 sampled pairs
    equal the oracle."""
    import torch
    from poly_amd import align, workloads
    n, LA, LB = 524_288, 150, 5000
    Bt, A2 = workloads.config4_reads(n, LA, LB, first=0, device=dev)
    _, D2 = workloads.config4_reads(n, LA, LB, first=600_000, device=dev)
    offs = torch.arange(0, (n + 1) * LA, LA, dtype=torch.int64, device=dev)
    c = sh.Case(dev, "sw_batch_dev, two sub-batches")
    At, offA, B = c.inp(A2.reshape(-1), D2.reshape(-1)), c.inp(offs, offs.clone()), c.inp(Bt, Bt.flip(0))
    del D2
    score = c.out((n,), torch.int64)
    ea, eb, er = (c.out((n,), torch.int32) for _ in range(3))
    wk = c.work(align.sw_workspace_bytes(nuc4, n, LA, LB, True))
    c.call = lambda st: align.sw_batch_dev(nuc4, At, offA, LA, B, None, LB, score, ea, eb, er, wk, stream=st)
    r = sh.run(c, delay)
    assert align.last_path() == 3
    # the same batch in one piece, on the default stream
    monkeypatch.setenv("POLYHIP_SW_OVERLAP", "0")
    ref = [torch.zeros(n, dtype=torch.int64, device=dev)] + [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3)]
    wk2 = torch.empty_like(wk)
    align.sw_batch_dev(nuc4, A2.reshape(-1), offs, LA, Bt, None, LB, *ref, wk2)
    torch.cuda.synchronize()
    for got, w, what in zip(r.outs, ref, ("score", "endA", "endB", "err")):
        assert (got == w.cpu().numpy()).all(), f"{what} differs from the POLYHIP_SW_OVERLAP=0 run"
    sample = list(range(0, n, n // 200))[:200]
    reads, refb, om = A2.cpu().numpy(), Bt.cpu().numpy().tobytes(), _om()
    want = _threads(lambda p: orc.smith_waterman(reads[p].tobytes(), refb, om, -2), sample)
    _sw_check(r, "batch", want, 0, "sw_batch_dev, two sub-batches", sample)


@pytest.mark.parametrize("kind", ["le64", "le150", "wave700"])
def test_needleman_wunsch(dev, delay, nuc4, kind):
    """300 ragged pairs of at most 64 symbols (the register-tiled kernel: it is taken up to 64 rows), 300 of at most 150
    and 8 pairs of 700 (one wave per pair, four and sixteen rows per lane); every pair"""
    import torch
    from poly_amd import align

    def make(seed):
        rng = np.random.default_rng(seed)
        top = {"le64": 64, "le150": 150}.get(kind)
        lens = rng.integers(0, top + 1, 300) if top else np.full(8, 700)
        if top:
            lens[:3] = (0, 1, top)
        A = [_dna(rng, int(L)) for L in lens]
        B = []
        for a in A:
            b = bytearray(a)
            for _ in range(int(rng.integers(0, 6)) + len(a) // 40):
                if b and rng.random() < 0.5:
                    del b[int(rng.integers(0, len(b)))]
                else:
                    b.insert(int(rng.integers(0, len(b) + 1)), int(rng.choice(list(b"ACGT"))))
            B.append(bytes(b))
        return A, B
    A, B = make(60)
    # the decoy: every string reversed, the pairs in reverse order (valid pairs in buffers of the true ones' sizes)
    Ad, Bd = [a[::-1] for a in A][::-1], [b[::-1] for b in B][::-1]
    pa, oa = _pack(A)
    pb, ob = _pack(B)
    pad, oad = _pack(Ad)
    pbd, obd = _pack(Bd)
    n, maxA, maxB = len(A), max(map(len, A)), max(map(len, B))
    c = sh.Case(dev, f"nw_align_dev ({kind})")
    At, offA, Bt, offB = c.inp(pa, pad), c.inp(oa, oad), c.inp(pb, pbd), c.inp(ob, obd)
    score, err = c.out((n,), torch.int64), c.out((n,), torch.int32)
    stride = maxA + maxB
    alnA, alnB, ln = c.out((n, stride), torch.uint8), c.out((n, stride), torch.uint8), c.out((n,), torch.int32)
    wk = c.work(align.nw_workspace_bytes(n, maxA, maxB))
    c.call = lambda st: align.nw_align_dev(nuc4, At, offA, maxA, Bt, offB, maxB, score, err, alnA, alnB, ln, wk, stream=st)
    r = sh.run(c, delay)
    assert align.nw_last_path() == (1 if kind == "le64" else 3)
    om = _om()
    for p, (a, b) in enumerate(zip(A, B)):
        w = orc.needleman_wunsch(a, b, om, -2)
        L = int(r.outs[4][p])
        got = (int(r.outs[0][p]), int(r.outs[1][p]), r.outs[2][p, stride - L:].tobytes(), r.outs[3][p, stride - L:].tobytes())
        assert got == (w[0], 0, _b(w[1]), _b(w[2])), f"pair {p}"


# ---------------------------------------------------------------- K4: primers
def _genome(seed=0xC5):
    """the 700-base genome of test_primers_gpu.py::test_scan_matches_oracle_bit_exact"""
    g = bytes(orc.synth_dna(seed, 700))
    return g[:100] + b"GAATTCGAATTCGAATTCGAATTC" + g[124:300] + b"acgtnnacgt" + g[310:500] + b"NNSWNNSWNN" + g[510:]


def _same_doubles(got, want, what):
    assert (np.isnan(got) == np.isnan(want)).all(), f"{what}: NaN pattern"
    m = ~np.isnan(want)
    assert (got[m].view(np.uint64) == want[m].view(np.uint64)).all(), f"{what}: bits differ"


def test_santalucia_scan(dev, delay):
    """santalucia_scan_dev at 18..30 with start0 = 1 and a plane stride above nstarts: the bits of tm, dH, dS"""
    import torch
    from poly_amd import primers
    g, gd = _genome(), _genome(0xC6)
    n, lo, hi, conc, na, mg = len(g), 18, 30, 500e-9, 50e-3, 0.0
    ns = n - lo          # starts 1 .. n - lo
    ld = ns + 3
    c = sh.Case(dev, "santalucia_scan_dev")
    gt = c.inp(np.frombuffer(g, np.uint8), np.frombuffer(gd, np.uint8))
    planes = [c.out((hi - lo + 1, ld), torch.float64) for _ in range(3)]
    c.call = lambda st: primers.santalucia_scan_dev(gt, n, 1, ns, lo, hi, conc, na, mg, *planes, ld)  # torch's current stream
    r = sh.run(c, delay)
    want = orc.santalucia_scan(g, lo, hi, conc, na, mg)
    for got, w, what in zip(r.outs, want, ("tm", "dH", "dS")):
        _same_doubles(got[:, :ns], w[:, 1:1 + ns], what)


def test_santalucia_scan_first(dev, delay):
    import torch
    from poly_amd import primers
    g, gd = _genome(), _genome(0xC6)
    n, lo, hi, target = len(g), 18, 30, 55.0
    ns = n - lo
    c = sh.Case(dev, "santalucia_scan_first_dev")
    gt = c.inp(np.frombuffer(g, np.uint8), np.frombuffer(gd, np.uint8))
    fl, ft = c.out((ns,), torch.int16), c.out((ns,), torch.float64)
    c.call = lambda st: primers.santalucia_scan_first_dev(gt, n, 1, ns, lo, hi, 500e-9, 50e-3, 0.0, target, fl, ft, stream=st)
    r = sh.run(c, delay)
    tm = orc.santalucia_scan(g, lo, hi, 500e-9, 50e-3, 0.0)[0]
    want_len, want_tm = np.zeros(ns, np.uint16), np.full(ns, np.nan)
    for i in range(ns):                    # the grow loop of pcr.go:47-53 at start i + 1
        for L in range(lo, hi + 1):
            if i + 1 + L > n:
                break
            if not (tm[L - lo, i + 1] < target):
                want_len[i], want_tm[i] = L, tm[L - lo, i + 1]
                break
    assert (r.outs[0].view(np.uint16) == want_len).all() and (want_len > 0).any()
    _same_doubles(r.outs[1], want_tm, "first_tm")


def _primers(seed):
    rng = np.random.default_rng(seed)
    lens = np.random.default_rng(7).integers(1, 41, 600)
    lens[7] = 0                                # an empty sequence: quiet NaNs in the device flavour
    if seed & 1:
        lens = lens[::-1]
    return [bytes(rng.choice(list(b"ACGT" if i % 3 else b"ACGTacgtNnRYUu-*"), int(L)).astype(np.uint8)) for i, L in enumerate(lens)]


def test_santalucia_and_marmurdoty_batches(dev, delay):
    """santalucia_batch_dev and marmurdoty_batch_dev (poly_amd.primers wrappers): 600 ragged primers"""
    import torch
    from poly_amd import primers
    P, Pd = _primers(70), _primers(71)
    bt, ot = _pack(P)
    bd, od = _pack(Pd)
    conc, na, mg = 250e-9, 50e-3, 1.5e-3
    c = sh.Case(dev, "santalucia_batch_dev + marmurdoty_batch_dev")
    seqs, offs = c.inp(bt, bd), c.inp(ot, od)
    tm, dH, dS, md = (c.out((len(P),), torch.float64) for _ in range(4))

    def call(st):
        primers.santalucia_batch_dev(seqs, offs, conc, na, mg, tm, dH, dS, stream=st)
        primers.marmurdoty_batch_dev(seqs, offs, md)   # torch's current stream
    c.call = call
    r = sh.run(c, delay)
    want = np.array([orc.santalucia(p, conc, na, mg) if p else (np.nan,) * 3 for p in P])
    for q, what in enumerate(("tm", "dH", "dS")):
        _same_doubles(r.outs[q], np.ascontiguousarray(want[:, q]), what)
    keep = np.array([len(p) > 0 for p in P])
    assert (r.outs[3][keep] == np.array([orc.marmur_doty(p) for p in P if p])).all()


# ---------------------------------------------------------------- K5, seqhash
def _circular_set(seed):
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in np.random.default_rng(8).integers(1, 10_001, 196)] + [9000, 7169, 4000, 3001]
    if seed & 1:
        lens = lens[::-1]
    seqs = [_dna(rng, L) for L in lens]
    q = lens.index(4000)
    seqs[q] = b"ACGTTGCA" * 500                                  # an exact tandem repeat
    q = lens.index(3001)
    seqs[q] = seqs[q][:1500] + b"X" + seqs[q][1501:]             # one letter outside the alphabet
    return seqs


def test_least_rotation_and_seqhash(dev, delay):
    """least_rotation_batch_dev and seqhash_batch_dev (DNA, circular, double-stranded): 200 sequences of 1..10 kb, two
    above the 7168 bytes a wave takes alone (the workgroup kernel), an exact tandem repeat, one alphabet error"""
    import torch
    from poly_amd import seqhash
    S, Sd = _circular_set(80), _circular_set(81)
    bt, ot = _pack(S)
    bd, od = _pack(Sd)
    n, total, maxlen = len(S), len(bt), max(map(len, S))
    c = sh.Case(dev, "least_rotation_batch_dev + seqhash_batch_dev")
    seqs, offs = c.inp(bt, bd), c.inp(ot, od)
    rot, rotated = c.out((n,), torch.int64), c.out((total,), torch.uint8)
    hashes, err = c.out((n, 72), torch.uint8), c.out((n,), torch.int32)
    wk = c.work(seqhash.seqhash_workspace_bytes(n, total, True, True))

    def call(st):
        seqhash.least_rotation_batch_dev(seqs, offs, maxlen, rot, rotated, stream=st)
        seqhash.seqhash_batch_dev(seqs, offs, total, maxlen, 0, True, True, hashes, err, wk, stream=st)
    c.call = call
    r = sh.run(c, delay)
    o = ot.astype(np.int64)
    nerr = 0
    for i, q in enumerate(S):
        assert int(r.outs[0][i]) == orc.booth_least_rotation(q), i
        assert r.outs[1][o[i]:o[i + 1]].tobytes() == orc.rotate_sequence(q), i
        got = r.outs[2][i].tobytes().split(b"\0", 1)[0].decode("ascii")
        try:
            assert (got, int(r.outs[3][i])) == (orc.seqhash(q, "DNA", True, True), 0), i
        except orc.SeqhashError:
            assert (got, int(r.outs[3][i])) == ("", (2 << 8) | ord("X")), i
            nerr += 1
    assert nerr == 1


# ---------------------------------------------------------------- read feeders
def _fastq_image(seed, lens):
    rng = np.random.default_rng(seed)
    out = []
    for i, L in enumerate(lens):
        seq = bytes(rng.choice(list(b"ACGTN"), L).astype(np.uint8))
        qual = bytes(rng.integers(33, 74, L, dtype=np.uint8))
        out.append(b"@read%03d ch=%d\n" % (i, i % 7) + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out)


def _fasta_image(seed, lens):
    rng = np.random.default_rng(seed)
    out = []
    for i, L in enumerate(lens):
        seq = bytes(rng.choice(list(b"ACGTN"), L).astype(np.uint8))
        out.append(b">rec%03d\n" % i + b"".join(seq[j:j + 60] + b"\n" for j in range(0, L, 60)))
    return b"".join(out)


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_read_feeders(dev, delay, fmt):
    """fastq.pack_dev and fasta.pack_dev: 300 records, the image at byte offset 5 of its buffer, against the restated
    parsers (the decoy is another file of the same size)"""
    import torch
    from poly_amd import fasta, fastq
    lens = [int(x) for x in np.random.default_rng(90).integers(1, 400, 300)]
    image, mod, ref = (_fastq_image, fastq, fastq_ref) if fmt == "fastq" else (_fasta_image, fasta, fasta_ref)
    data, decoy = image(91, lens), image(92, lens[::-1])
    assert len(data) == len(decoy)
    nb = len(data)
    cap = nb // 7 + 2 if fmt == "fastq" else nb // 2 + 3
    c = sh.Case(dev, f"{fmt}.pack_dev")
    img = c.inp(np.frombuffer(data, np.uint8), np.frombuffer(decoy, np.uint8), offset=5)
    assert img.data_ptr() % 16 == 5
    seqs, offs, rec, res = c.out((nb,), torch.uint8), c.out((cap,), torch.int64), c.out((cap,), torch.int64), c.out((4,), torch.int64)
    wk = c.work(mod.workspace_bytes(nb))
    c.call = lambda st: mod.pack_dev(img, seqs, offs, rec, res, wk, stream=st)
    r = sh.run(c, delay)
    parsed = ref.parse_all(data)
    assert parsed[1] == 0
    want = [w[-2] if fmt == "fastq" else w[1] for w in parsed[0]]    # the Sequence of every record
    n, total = len(want), sum(map(len, want))
    assert n == 300
    res_h = [int(x) for x in r.outs[3]]
    assert (res_h[0], res_h[1], res_h[3 if fmt == "fastq" else 2]) == (n, 0, total)
    assert (r.outs[1][:n + 1] == np.concatenate([[0], np.cumsum([len(w) for w in want])])).all()
    assert r.outs[0][:total].tobytes() == b"".join(want)
    mark = b"@read" if fmt == "fastq" else b">rec"
    starts = [i for i in range(nb) if data.startswith(mark, i) and (i == 0 or data[i - 1:i] == b"\n")]
    assert len(starts) == n and list(r.outs[2][:n]) == starts


# ---------------------------------------------------------------- search/bwt
BWT_N = 70_001
_BWT = {}


def _bwt_text(alpha, seed):
    rng = np.random.default_rng(seed)
    a = ACGT if alpha == "dna" else np.frombuffer(b"\x00!#\x80\xffAz", np.uint8)   # "specials" of test_bwt_gpu.py
    return a[rng.integers(0, len(a), BWT_N)].tobytes()


def _bwt_create_case(dev, alpha):
    """bwt.new_dev: the text is an input of the side stream (the call synchronises it and returns the built handle)"""
    from poly_amd import bwt
    seq = _bwt_text(alpha, 100)
    c = sh.Case(dev, f"bwt.new_dev ({alpha})")
    st_ = c.inp(np.frombuffer(seq, np.uint8), np.frombuffer(_bwt_text(alpha, 101), np.uint8))
    wk = c.work(bwt.workspace_bytes(BWT_N))
    c.call = lambda st: bwt.new_dev(st_, wk, stream=st)
    o = bo.Oracle(seq, width=12)

    def check(r):
        assert r.ret.Layout() == ("nucleotide" if alpha == "dna" else "general")
        assert (r.ret.SuffixArray() == o.sa).all(), "the suffix array differs from the oracle's"
        assert r.ret.GetTransform() == o.transform()
        return r.ret, o, seq
    return c, check


def _bwt_index(dev, delay, alpha):
    """(index built by new_dev on a side stream, oracle, text), once per alphabet"""
    if alpha not in _BWT:
        c, check = _bwt_create_case(dev, alpha)
        _BWT[alpha] = check(sh.run(c, delay, asynchronous=False))
    return _BWT[alpha]


def _bwt_patterns(seq, seed):
    rng = np.random.default_rng(seed)
    pats = [seq[i:i + 12] for i in rng.integers(0, BWT_N - 12, 2000)]
    for q in range(0, 2000, 4):                               # a quarter with one byte changed
        p = bytearray(pats[q])
        p[int(rng.integers(0, 12))] = seq[int(rng.integers(0, BWT_N))]
        pats[q] = bytes(p)
    return pats + [b"", b"$" + seq[:5], b"NNNN"]


def _count_case(dev, idx, o, seq, seed=110, name="bwt.count_dev"):
    import torch
    from poly_amd import bwt
    pats = _bwt_patterns(seq, seed)
    bt, ot = _pack(pats)
    bd, od = _pack(_bwt_patterns(seq, seed + 1))
    n = len(pats)
    c = sh.Case(dev, name)
    pat, off = c.inp(bt, bd), c.inp(ot, od)
    c.iv = [c.out((n,), torch.int32) for _ in range(3)]
    c.call = lambda st: bwt.count_dev(idx, pat, off, *c.iv, stream=st)
    want = [o.interval(p) if p else (0, 0) for p in pats]

    def check(r, at=0):
        got = list(zip(r.outs[at].view(np.uint32).tolist(), r.outs[at + 1].view(np.uint32).tolist()))
        bad = [i for i in range(n) if got[i] != want[i]]
        assert not bad, f"{name}: {len(bad)} intervals differ from the oracle, first: pattern {bad[0]} got {got[bad[0]]} want {want[bad[0]]}"
        assert r.outs[at + 2].tolist() == [int(len(p) == 0) for p in pats]
    c.want = want
    return c, check


@pytest.mark.parametrize("alpha", ["dna", "specials"])
def test_bwt_create_transform_count_locate_extract(dev, delay, alpha):
    """n = 70,001; new_dev on a side stream builds the index the other calls use; 2000 patterns of 12, an empty one, one
    holding '$' (cyclic) and one of a byte the text lacks"""
    import torch
    from poly_amd import bwt
    idx, o, seq = _bwt_index(dev, delay, alpha)
    # transform
    c = sh.Case(dev, "bwt.transform_dev")
    L_t = c.out((BWT_N + 1,), torch.uint8)
    c.call = lambda st: bwt.transform_dev(idx, L_t, stream=st)
    assert sh.run(c, delay).outs[0].tobytes() == o.transform()
    # count
    c, check = _count_case(dev, idx, o, seq)
    check(sh.run(c, delay))
    # locate, on the intervals a count_dev on the same stream leaves (the setup call)
    want = c.want
    total = sum(e - s for s, e in want)
    c, check = _count_case(dev, idx, o, seq, name="bwt.count_dev + locate_dev")
    iv = c.iv
    c.outputs, c.mids = [], iv      # the intervals are now what the setup call writes and the call under test reads
    first, out = c.out((len(want) + 1,), torch.int64), c.out((total,), torch.int32)
    wk = c.work(bwt.locate_workspace_bytes(len(want)))
    c.setup = c.call
    c.call = lambda st: bwt.locate_dev(idx, iv[0], iv[1], first, out, wk, stream=st)
    r = sh.run(c, delay)
    check(r, at=2)
    assert (r.outs[0] == np.concatenate([[0], np.cumsum([e - s for s, e in want])])).all()
    assert (r.outs[1].view(np.uint32) == np.concatenate([o.sa[s:e] for s, e in want])).all()
    # extract: valid requests and each of the reference's failing checks
    def requests(seed):
        rng = np.random.default_rng(seed)
        a = rng.integers(0, BWT_N - 1, 60)
        b = np.minimum(a + rng.integers(1, 300, 60), BWT_N)
        a[:4], b[:4] = (5, 0, -1, 0), (5, BWT_N + 1, 3, BWT_N)
        width = np.where((a < b) & (b <= BWT_N) & (a >= 0), b - a, 0)
        width[4] -= 1                                            # a slot shorter than its request: error 4
        return a.astype(np.int64), b.astype(np.int64), np.concatenate([[0], np.cumsum(width)]).astype(np.int64)
    a, b, oo = requests(120)
    ad, bd_, ood = requests(121)
    c = sh.Case(dev, "bwt.extract_dev")
    at, bt_, ot_ = c.inp(a, ad), c.inp(b, bd_), c.inp(oo, ood)
    ob, er = c.out((int(max(oo[-1], ood[-1])) + 1,), torch.uint8), c.out((60,), torch.int32)
    c.call = lambda st: bwt.extract_dev(idx, at, bt_, ot_, ob, er, stream=st)
    r = sh.run(c, delay)
    assert r.outs[1].tolist() == [1, 2, 3, 0, 4] + [0] * 55
    for i in range(60):
        if r.outs[1][i] == 0:
            assert r.outs[0][oo[i]:oo[i + 1]].tobytes() == seq[a[i]:b[i]], i


# ---------------------------------------------------------------- read mapping
MAP_FIELDS = ["score", "second", "flags", "votes", "ref_start", "ref_end", "read_start", "read_end", "err"]
MAP_COUNTERS = ["seeds", "seeds_over_max_occ", "hits", "clusters", "pairs_aligned", "reads_mapped"]


def _map_case(dev, sc):
    """map_inputs.dataset() with PARAMS_A through a workspace of 0.34 x the full size: at least three chunks, each with
    its own read-back of two counts"""
    import dataclasses
    import torch
    from poly_amd import bwt, mapper
    d = mi.dataset()
    reads = d["reads"]
    hits, info = mi.expected("a")
    index = bwt.New(d["T"])
    P = mapper.MapParams(**dataclasses.asdict(mi.PARAMS_A))
    bt, ot = _pack(reads)
    bd, od = _pack([r[::-1] for r in reads][::-1])
    n, maxlen = len(reads), max(map(len, reads))
    cap = len(bt) * 2 + 1024
    c = sh.Case(dev, "map_reads_dev")
    rt, off = c.inp(bt, bd), c.inp(ot, od)
    i64 = [c.out((n,), torch.int64) for _ in range(2)]
    i32 = [c.out((n,), torch.int32) for _ in range(7)]
    sa, sb, so = c.out((cap,), torch.uint8), c.out((cap,), torch.uint8), c.out((n + 1,), torch.int64)
    wk = c.work(int(mapper.workspace_bytes(index, sc, P, n, maxlen) * 0.34))
    c.call = lambda st: mapper.map_reads_dev(index, sc, rt, off, maxlen, P, *i64, *i32, sa, sb, so, wk, stream=st)

    def check(r):
        assert r.ret == 0
        for q, f in enumerate(MAP_FIELDS):
            want = np.array([getattr(h, f) for h in hits], dtype=np.int64)
            have = r.outs[q].astype(np.int64) if q < 2 else r.outs[q].view(np.uint32).astype(np.int64)
            bad = np.nonzero(want != have)[0]
            assert bad.size == 0, f"{f}: {bad.size} reads differ, first {bad[0]}: got {have[bad[0]]}, want {want[bad[0]]}"
        a, b, o = r.outs[9], r.outs[10], r.outs[11]
        for i, h in enumerate(hits):
            assert (a[o[i]:o[i + 1]].tobytes(), b[o[i]:o[i + 1]].tobytes()) == (h.alignA, h.alignB), f"aligned strings of read {i}"
        got = mapper.last_info()
        assert {k: got[k] for k in MAP_COUNTERS} == {k: info[k] for k in MAP_COUNTERS} and got["chunks"] >= 3
    return c, check


def test_map_reads(dev, delay, nuc4):
    c, check = _map_case(dev, nuc4)
    check(sh.run(c, delay, asynchronous=False))


# ---------------------------------------------------------------- collectives on a one-rank communicator
def _comm():
    from poly_amd import comm
    return comm.Comm(comm.unique_id(), 0, 1)


def test_allgather_collectives_one_rank(dev, delay):
    """allgather_sketches_dev and allgatherv_dev as tests/test_comm_gpu.py runs them on one GPU"""
    import torch
    rng = np.random.default_rng(130)
    cm = _comm()
    local = rng.integers(0, 1 << 32, (300, 64), dtype=np.uint32)
    c = sh.Case(dev, "allgather_sketches_dev + allgatherv_dev")
    lt = c.inp(local, rng.integers(0, 1 << 32, (300, 64), dtype=np.uint32))
    bufv = rng.integers(0, 1 << 32, 4096, dtype=np.uint32)
    bt = c.inp(bufv, rng.integers(0, 1 << 32, 4096, dtype=np.uint32))
    out, kept = c.out((300, 64), torch.int32), c.out((4096,), torch.int32)

    def call(st):
        cm.allgather_sketches(lt, out, stream=st)
        cm.allgatherv(bt, [64, 4096 * 4 - 128], stream=st)
        kept.copy_(bt)                                     # (in place: rank 0 owns the whole range)
    c.call = call
    r = sh.run(c, delay)
    assert (r.outs[0].view(np.uint32) == local).all() and (r.outs[1].view(np.uint32) == bufv).all()
    cm.close()


def _index_allgather_case(dev):
    """index_build_part_dev(part 0 of 1) as the setup, then mash_index_allgather_dev and the join"""
    from poly_amd import mash
    cm = _comm()
    c, check = _k2_case(dev, "index_build_part_dev + mash_index_allgather_dev")
    c.setup = lambda st: mash.index_build_part_dev(c.Yt, 0, 1, c.wk, stream=st)

    def call(st):
        cm.index_allgather(512, 96, c.wk, stream=st)
        mash.shared_counts_reuse_dev(c.Xt, c.Yt, c.counts, c.wk, stream=st)
    c.call = call

    def check2(r):
        check(r)
        cm.close()
    return c, check2


def test_index_allgather_one_rank(dev, delay):
    c, check = _index_allgather_case(dev)
    check(sh.run(c, delay, asynchronous=False))


# ---------------------------------------------------------------- two calls in flight
def test_two_calls_in_flight_on_two_streams(dev, delay, nuc4):
    """one thread, two side streams: the sketch case on s1 and the packed Smith-Waterman case on s2 (the module's one
    scoring handle), each behind its own delay; then a count_dev on each stream against ONE index handle"""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    idx, o, seq = _bwt_index(dev, delay, "dna")
    sk, sk_check = _sketch_case(dev, _slab_reads(0xA0), _slab_reads(0xA1), 21, 1000, "sketch on s1")
    A, B, Ad, Bd, sample, want = _fork_inputs()   # (98,304 reads: the packed pass)
    sw = _sw_case(dev, nuc4, A, B, Ad, Bd, "batch", "packed SmithWaterman on s2")
    c1, c1_check = _count_case(dev, idx, o, seq, 140, "count_dev on s1")
    c2, c2_check = _count_case(dev, idx, o, seq, 150, "count_dev on s2")
    for c in (sk, sw, c1, c2):
        c.prepare()
    sk.enqueue(s1, delay)
    sw.enqueue(s2, delay)
    c1.enqueue(s1, delay)
    c2.enqueue(s2, delay)
    r = [c.finish() for c in (sk, sw, c1, c2)]
    sk_check(r[0])
    _sw_check(r[1], "batch", want, 0, "packed SmithWaterman on s2", sample)
    c1_check(r[2])
    c2_check(r[3])


# ---------------------------------------------------------------- the calls documented as synchronising
def _part_spans_case(dev):
    from poly_amd import mash
    c, _ = _parts_case(dev, "index_part_spans")

    def call(st):
        spans = mash.index_part_spans(512, 96, 2, c.wk, stream=st)
        c.head.copy_(c.wk[:128])
        return spans
    c.call = call

    def check(r):
        import torch
        it, st_ = r.ret
        regular = sum(nbo.is_ascending(y) for y in _k2()[1])
        item_bytes = mash.index_item_bytes(torch.from_numpy(r.outs[1].copy()).to(dev))
        assert all(it[p] <= it[p + 1] and st_[p] <= st_[p + 1] for p in range(2))
        assert int(it[2] - it[0]) == regular * 96 * item_bytes, "the parts do not hold every item of the regular sketches"
        again = mash.index_part_spans(512, 96, 2, _default_stream_index(dev, 2))   # the same build, default stream
        assert (list(again[0]), list(again[1])) == (list(it), list(st_))
    return c, check


@pytest.mark.parametrize("which", ["sketch_size_one", "index_part_spans", "index_allgather", "neighbors_dev", "bwt_create_dev",
                                   "map_reads_dev"])
def test_documented_synchronising_calls_return_final_outputs(dev, delay, nuc4, which):
    """The calls the header documents as synchronising `stream`: when they return, the delay in front of them is over
    and their outputs are final.  No stream synchronise by the test: the clones taken on the side stream are read with a
    synchronous copy."""
    build = {"sketch_size_one": lambda: _sketch_tiny_case(dev), "index_part_spans": lambda: _part_spans_case(dev),
             "index_allgather": lambda: _index_allgather_case(dev), "neighbors_dev": lambda: _neighbors_case(dev),
             "bwt_create_dev": lambda: _bwt_create_case(dev, "dna"), "map_reads_dev": lambda: _map_case(dev, nuc4)}[which]
    c, check = build()
    r = sh.run(c, delay, asynchronous=False, synchronize=False)
    assert not r.in_flight, f"{which} returned while the work in front of it on the stream was still running"
    check(r)
