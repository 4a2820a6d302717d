"""K1 slab pass: its grid is 32 rounds of the workgroups the chip holds (256 CUs x 8 x 32 = 65,536), and read r goes to
workgroup r mod grid.  A workgroup therefore sees a second read -- reuses its rings, segments and bins -- only in a
batch of more than 65,536 reads.  64 distinct reads of 3..7 slabs (uneven quarters; at 3, 5 and 6 slabs a wave with
none) are tiled in a fixed shuffled order to 65,536 + 8,192 + 77 reads: workgroups 0..8,268 run two reads, the others
one, and the batch is no multiple of anything.  Every row equals the oracle's row of its read (the oracle runs on the
64 distinct reads only)."""
import math

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

K, S, GRID = 21, 200, 65_536
NREADS = GRID + 8_192 + 77


def _keeps(nwin):
    """the slab pass keeps a read of nwin windows at s = 200: the fullest wave's expected survivors + 6 sigma fit its
    segment (mash_sketch.hip plan(): capw 192; the kernel's target is 200 + 6 * 14 + 16 survivors)"""
    rt = 15  # ceil(sqrt(200))
    target = S + 6 * 14 + 16
    exp_w = (S + 6 * rt + 16 + 3) // 4
    rw = math.isqrt(exp_w - 1) + 1
    capw = (exp_w + 6 * rw + 8 + 63) & ~63
    p = target / nwin + 2.0 ** -16
    w = (((nwin + 255) >> 8) + 3) // 4 * 256
    return w * p + 6.0 * math.sqrt(w * p * (1.0 - p)) < capw


def test_a_workgroup_runs_a_second_read():
    from poly_amd import mash
    rng = np.random.default_rng(4242)
    reads = []
    for i in range(64):
        nslab = 3 + i % 5
        r = int(rng.integers(1, 257))
        while not _keeps(256 * (nslab - 1) + r):  # (5 slabs: two per wave, the last slab has to be nearly full)
            r += 1
        assert r <= 256
        reads.append(rng.choice(np.frombuffer(b"ACGT", np.uint8), K + 256 * (nslab - 1) + r))
    assert {(len(r) - K + 255) >> 8 for r in reads} == set(range(3, 8))
    doffs = np.zeros(65, np.uint64)
    doffs[1:] = np.cumsum([len(r) for r in reads])
    want = orc.mash_sketch_batch(np.concatenate(reads), doffs, K, S)

    which = rng.permutation(np.arange(NREADS) % 64)
    assert set(which[GRID:].tolist()) == set(range(64))  # every distinct read is some workgroup's second
    lens = np.array([len(r) for r in reads], np.uint64)[which]
    offs = np.zeros(NREADS + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    buf = np.concatenate([reads[w] for w in which])
    got = mash.sketch_batch_packed(buf, offs, K, S)
    bad = np.nonzero((got != want[which]).any(axis=1))[0]
    assert bad.size == 0, (bad.size, bad[:8], which[bad[:8]], lens[bad[:8]])
