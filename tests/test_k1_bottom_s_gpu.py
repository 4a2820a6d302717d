"""K1 fast bottom-s (bottom_s_fast): its count and scatter passes from registers and its rank pass by quads of slots.
A wave of the slab pass holds about (s + 6 sqrt(s) + 16) / 4 survivors whatever the read's length, so SketchSize alone
chooses how many candidates a lane takes: one to seven in registers, more in the looped form.  Every sketch equals the
oracle's bit for bit, and the tile pass (POLYHIP_K1_SLABS=0: the other caller, 256 candidates per trip instead of 64)
equals the slab pass row for row."""
import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

KS = (17, 21, 31)
BIG_BIN = 32  # mash_sketch.hip: a bin of more values than this is placed by whole waves


@pytest.fixture(scope="module")
def mash():
    from poly_amd import mash as m
    return m


def _random(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes()


def _pack(reads):
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads), np.uint8).copy(), offs


def _check(mash, monkeypatch, reads, k, s):
    """slab pass == oracle and tile pass == slab pass, row for row; returns the oracle's sketches"""
    buf, offs = _pack(reads)
    want = orc.mash_sketch_batch(buf, offs, k, s, faithful=False)
    monkeypatch.delenv("POLYHIP_K1_SLABS", raising=False)
    slab = mash.sketch_batch_packed(buf, offs, k, s)
    bad = np.nonzero((slab != want).any(axis=1))[0]
    assert bad.size == 0, ("slab pass", k, s, bad[:8], [len(reads[i]) for i in bad[:8]])
    monkeypatch.setenv("POLYHIP_K1_SLABS", "0")
    tile = mash.sketch_batch_packed(buf, offs, k, s)
    bad = np.nonzero((tile != slab).any(axis=1))[0]
    assert bad.size == 0, ("tile pass", k, s, bad[:8], [len(reads[i]) for i in bad[:8]])
    return want


# ---- trips: 14, 88, 163, 302, 411 and 464 survivors per wave at s = 16, 240, 500, 1000, 1400, 1600, i.e. 1, 2, 3, 5 and 7
#      trips from registers and then the loop; s = 2 .. 65 around one candidate per lane of the tile pass's first trip
@pytest.mark.parametrize("s", (2, 3, 16, 63, 64, 65, 240, 500, 1000, 1400, 1600, 4000))
@pytest.mark.parametrize("k", KS)
def test_trip_counts(mash, monkeypatch, k, s):
    rng = np.random.default_rng(100 * s + k)
    if s <= 1600:
        lens = rng.integers(2400, 3001, 200)
    else:
        lens = rng.integers(5200, 6001, 48)  # (a read needs more than s windows)
    _check(mash, monkeypatch, [_random(rng, int(n)) for n in lens], k, s)


# ---- segment edges: a wave's count is a multiple of 64 (no partial trip) about once in 64 waves
def test_many_reads_hit_whole_trips(mash, monkeypatch):
    rng = np.random.default_rng(2000)
    _check(mash, monkeypatch, [_random(rng, int(n)) for n in rng.integers(2600, 3001, 2000)], 21, 1000)


# ---- segment edges: reads of s, s + 1, s + 255 and s + 257 windows keep every hash (the threshold is 2^32 - 1), so the
#      last waves end with no survivor at all and the others hold whole slabs
@pytest.mark.parametrize("s", (64, 240, 1000))
@pytest.mark.parametrize("k", KS)
def test_reads_of_barely_s_windows(mash, monkeypatch, k, s):
    rng = np.random.default_rng(300 * s + k)
    reads = []
    for extra in (0, 1, 255, 257):
        for _ in range(12):
            reads.append(_random(rng, k + s + extra))
            reads.append(_random(rng, int(rng.integers(2000, 3001))))  # (shifts the next read's alignment)
    _check(mash, monkeypatch, reads, k, s)


# ---- the rank pass's second trip: one trip is 4 x 256 slots, and e*, the end of the bin of slot s - 1, passes 1024
@pytest.mark.parametrize("s", (1023, 1024, 1025))
@pytest.mark.parametrize("k", KS)
def test_rank_pass_second_trip(mash, monkeypatch, k, s):
    rng = np.random.default_rng(7 * s + k)
    _check(mash, monkeypatch, [_random(rng, int(n)) for n in rng.integers(2600, 3001, 200)], k, s)


# ---- equal hashes: duplicates keep distinct ranks, by slot
@pytest.mark.parametrize("k", KS)
def test_repeats(mash, monkeypatch, k):
    rng = np.random.default_rng(900 + k)
    s = 1000
    reads = [b"A" * 3000, b"C" * (k + s), b"G" * 2999]  # homopolymers: one hash, the general kernel's
    for period in (3, 7, 50):
        for _ in range(4):
            unit = _random(rng, period)
            reads.append((unit * (3000 // period + 1))[:int(rng.integers(2000, 3001))])
    reads += [_random(rng, 3000) for _ in range(8)]
    _check(mash, monkeypatch, reads, k, s)


@pytest.mark.parametrize("s", (500, 1000))
@pytest.mark.parametrize("k", KS)
def test_embedded_repeat_among_the_smallest(mash, monkeypatch, k, s):
    """Random reads with a short-period repeat in the middle: the repeat's k-mers are 40 or more EQUAL hashes each, in one
    bin.  Where the oracle puts such a hash among the s smallest, the bin holds more than BIG_BIN values at a rank below
    s and whole waves place it (rank_big_bins); the others are cut off by e* or fall behind rank s."""
    rng = np.random.default_rng(5000 + 10 * s + k)
    reads = []
    for unit in (b"A", b"C", b"G", b"T", b"AC", b"AG", b"AT", b"CG", b"CT", b"GT", b"ACG", b"ACT", b"AGT", b"CGT",
                 b"AAC", b"AAG", b"AAT", b"CCA", b"CCG", b"CCT", b"GGA", b"GGC", b"GGT", b"TTA", b"TTC", b"TTG"):
        rep = (unit * 200)[:k + 40 * len(unit) + int(rng.integers(0, 30))]
        head = int(rng.integers(200, 1500))
        reads.append(_random(rng, head) + rep + _random(rng, 3000 - head - len(rep)))
    want = _check(mash, monkeypatch, reads, k, s)
    most = [int(np.unique(row, return_counts=True)[1].max()) for row in want]
    assert sum(m > BIG_BIN for m in most) >= 3, most  # the inputs do what they are meant to
