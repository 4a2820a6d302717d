"""K1 slab pass: the edges of its main loop (full slabs whose next-but-one slab's loads lie inside the read: no guards,
two slabs per trip) and its guarded epilogue.  Reads at every alignment of their first byte (0-3 bytes past a dword),
of lengths that put the last slab full or partial and the end of the guard-free loads one or two slabs before the
last slab, and of slab counts whose split over the four waves starts a wave on an odd slab or leaves a wave with none.
Every sketch equals the oracle's, at k = 17, 21 and 31."""
import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

KS = ((21, 1000), (17, 200), (31, 2000))


@pytest.fixture(scope="module")
def mash():
    from poly_amd import mash as m
    return m


def _split(n, k, gsh):
    """(slabs, full slabs, first slab with a guarded load, main-loop end of each wave) as the kernel computes them"""
    nwin = n - k
    nslab = (nwin + 255) >> 8
    spw = (nslab + 3) // 4
    gbytes = n + gsh
    u_inside = (((gbytes >> 2) - 65) >> 6) + 1 if gbytes >= 260 else 0
    return nslab, nwin >> 8, u_inside, spw


def _lengths(k, s):
    out = []
    for nslab in (1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 13, 17, 39, 40):
        for r in (1, 2, 3, 4, 5, 64, 128, 200, 252, 253, 254, 255, 256):
            n = k + 256 * (nslab - 1) + r
            if n - k >= s:
                out.append(n)
    return out


@pytest.mark.parametrize("k,s", KS)
def test_main_loop_and_epilogue_edges(mash, k, s):
    rng = np.random.default_rng(7000 + k)
    reads, seen = [], set()
    off = 0
    for n in _lengths(k, s):
        for gsh in range(4):
            # an ordinary read in front whose length brings this one's first byte to offset gsh mod 4
            pad = s + k + 3 + ((gsh - (off + s + k + 3)) % 4)
            for m in (pad, n):
                reads.append(rng.choice(list(b"ACGT"), m).astype(np.uint8).tobytes())
                off += m
            assert (off - n) % 4 == gsh
            nslab, nfull, u_inside, spw = _split(n, k, gsh)
            seen.add((gsh, nslab == nfull, u_inside - nslab, spw % 2 == 1 and nslab > spw, 3 * spw >= nslab))
    # every alignment, last slab full and partial, guarded loads from one and two slabs before the end, odd wave starts
    # and (for the short reads of s = 200) empty waves
    assert {g for g, *_ in seen} == {0, 1, 2, 3}
    assert {f for _, f, *_ in seen} == {True, False}
    assert {0, -1} <= {d for _, _, d, *_ in seen}
    assert any(o for *_, o, _ in seen)
    if s <= 512:
        assert any(e for *_, e in seen)
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    buf = np.frombuffer(b"".join(reads), np.uint8).copy()
    got = mash.sketch_batch_packed(buf, offs, k, s)
    want = orc.mash_sketch_batch(buf, offs, k, s)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (k, s, bad[:8], [len(reads[i]) for i in bad[:8]])
