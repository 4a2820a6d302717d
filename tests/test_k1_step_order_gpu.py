"""K1 slab pass: the order of a step's LDS traffic at the slab edges.  A step stages the next slab into the other half
of the byte ring, premixes it, and hashes the current slab, whose last windows read their tail bytes from the bytes
just staged and their blocks from the quads just premixed; what can go wrong is a tail byte or a quad read before it
is written, or after its ring slot was rewritten.  ACGT input hides that (four table entries: many stale values hash
alike), so the reads are uniformly random bytes, and one set has 48 distinct bytes around every slab edge.  k = 17, 21
(one tail byte through the table) and 31 (three tail bytes from two dwords), all four alignments of the first byte,
slab counts 4, 8, 12 (balanced quarters), 39 (10/10/10/9, a wave starting on an odd slab) and 40, the last slab holding
1, 20, 236, 252, 255 and 256 windows (the epilogue with one and two guarded slabs).  SketchSize is 0.39-0.52 of the
windows, so that a wrong hash in any window is likely to change the sketch, and small enough that the slab pass keeps
the read: checked here with plan()'s arithmetic."""
import math

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

SLABS_S = ((4, 400), (8, 800), (12, 1200), (39, 4000), (40, 4000))
LAST = (1, 20, 236, 252, 255, 256)
WAVES, SIG, CW, CAPK = 4, 6, 6, 12


@pytest.fixture(scope="module")
def mash():
    from poly_amd import mash as m
    return m


def _isqrt_up(x):
    r = 1
    while r * r < x:
        r += 1
    return r


def _caps(s):
    """(target, capw, capf_slab) of mash_sketch.hip's plan() and sketch_slab_kernel"""
    rt = _isqrt_up(s)
    target = s + SIG * int(math.floor(math.sqrt(np.float32(s)))) + 16
    plan_target = s + SIG * rt + 16
    exp_w = (plan_target + WAVES - 1) // WAVES
    capw = (exp_w + CW * _isqrt_up(exp_w) + 8 + 63) & ~63
    capf = (((s + 3) & ~3) + CAPK * rt + 64 + 63) & ~63
    return target, capw, capf


def _slab_pass_keeps(nwin, s):
    """expected survivors of the fullest wave and of the read, six standard deviations on top, against the capacities"""
    target, capw, capf = _caps(s)
    p = min(1.0, target / nwin + 2.0 ** -16)  # the threshold is rounded up to 16 bits
    nslab = (nwin + 255) >> 8
    w = min(nwin, ((nslab + WAVES - 1) // WAVES) * 256)
    six = lambda n: 6.0 * math.sqrt(n * p * (1.0 - p))
    return w * p + six(w) < capw and nwin * p + six(nwin) < capf and nwin * p - six(nwin) >= s


def _distinct_edges(rng, read):
    """every byte of each slab's last 24 and first 24 positions distinct"""
    for edge in range(256, len(read) - 24, 256):
        read[edge - 24:edge + 24] = rng.permutation(256)[:48].astype(np.uint8)


@pytest.mark.parametrize("k", (17, 21, 31))
def test_tail_and_table_reads_at_slab_edges(mash, k):
    rng = np.random.default_rng(9100 + k)
    nreads = 0
    for nslab, s in SLABS_S:
        reads, kept, off = [], [], 0
        for r in LAST:
            n = k + 256 * (nslab - 1) + r
            assert _slab_pass_keeps(n - k, s) and 0.3 <= s / (n - k) <= 0.6, (nslab, r, s)
            for v in range(5):  # four alignments of random bytes, and one read with distinct bytes around the slab edges
                gsh = v if v < 4 else (r + nslab) % 4
                pad = (gsh - off) % 4  # a read too short for a window moves the next one's first byte
                if pad:
                    reads.append(rng.integers(0, 256, pad, dtype=np.uint8))
                    off += pad
                read = rng.integers(0, 256, n, dtype=np.uint8)
                if v == 4:
                    _distinct_edges(rng, read)
                assert off % 4 == gsh
                kept.append(len(reads))
                reads.append(read)
                off += n
        offs = np.zeros(len(reads) + 1, np.uint64)
        offs[1:] = np.cumsum([len(r) for r in reads])
        buf = np.concatenate(reads)
        got = mash.sketch_batch_packed(buf, offs, k, s)
        want = orc.mash_sketch_batch(buf, offs, k, s)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (k, nslab, s, bad[:8], [len(reads[i]) for i in bad[:8]])
        nreads += len(kept)
    assert nreads == 150
