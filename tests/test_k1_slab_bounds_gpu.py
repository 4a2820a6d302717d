"""K1 slab pass at its edges: reads built so that the survivor count of the verified threshold pass sits exactly at
SketchSize and at the sorted buffer's capacity (capf), one either side of each, and reads whose survivors fill as many
big bins (more than 32 equal values each) as the buffer can hold.  Every sketch equals the oracle's, at k = 17, 21 and 31.

The slab pass keeps its bottom-s (16-bit counting-sort bins, the sorted buffer and the big-bin list) inside the LDS its
rings free after the last slab; the big-bin list holds capf / 33 + 1 entries, more than a read that fits the buffer can
have, so the list-overflow fallback is unreachable there: the big-bin test fills the list as far as a read can."""
import math

import numpy as np
import pytest

import oracle as orc

pytestmark = pytest.mark.gpu

KS = ((21, 1000), (17, 200), (31, 2000))
L = 10_000


@pytest.fixture(scope="module")
def mash():
    from poly_amd import mash as m
    return m


def _isqrt_ceil(x):
    r = math.isqrt(x)
    return r if r * r == x else r + 1


def _caps(s):
    """capf and capw of the slab pass (mash_sketch.hip, plan())."""
    rt = _isqrt_ceil(s)
    capf = (((s + 3) & ~3) + 12 * rt + 64 + 63) & ~63
    exp_w = (s + 6 * rt + 16 + 3) // 4
    capw = (exp_w + 6 * _isqrt_ceil(exp_w) + 8 + 63) & ~63
    return capf, capw


def _tauq(nwin, s):
    """the slab pass's threshold; a hash survives iff it is <= this value"""
    target = s + 6 * int(math.sqrt(s)) + 16
    return ((target << 32) // nwin) | 0xFFFF if target < nwin else 0xFFFFFFFF


def _wave_counts(surv):
    """survivors per wave: wave w hashes slabs [w * spw, (w + 1) * spw) of 256 windows"""
    nslab = (len(surv) + 255) // 256
    spw = (nslab + 3) // 4
    return [int(surv[256 * w * spw: 256 * (w + 1) * spw].sum()) for w in range(4)]


def _with_survivors(rng, k, s, want):
    """a random read of L bases mutated one base at a time until exactly `want` windows survive the threshold"""
    read = bytearray(rng.choice(list(b"ACGT"), L).astype(np.uint8).tobytes())
    nwin = L - k
    tau = _tauq(nwin, s)
    surv = np.array([orc.murmur3_32(bytes(read[i:i + k])) <= tau for i in range(nwin)])
    c = int(surv.sum())
    for _ in range(200_000):
        if c == want:
            return bytes(read), surv
        p = int(rng.integers(0, L))
        b = int(rng.choice(list(b"ACGT")))
        if read[p] == b:
            continue
        old, read[p] = read[p], b
        lo, hi = max(0, p - k + 1), min(nwin, p + 1)
        new = np.array([orc.murmur3_32(bytes(read[i:i + k])) <= tau for i in range(lo, hi)], dtype=bool)
        d = int(new.sum()) - int(surv[lo:hi].sum())
        if abs(c + d - want) < abs(c - want):
            surv[lo:hi] = new
            c += d
        else:
            read[p] = old
    raise AssertionError(f"no read with {want} survivors")


def _check(mash, reads, k, s):
    offs = np.zeros(len(reads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    buf = np.frombuffer(b"".join(reads), np.uint8).copy()
    got = mash.sketch_batch_packed(buf, offs, k, s)
    want = orc.mash_sketch_batch(buf, offs, k, s)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (k, s, bad[:8])


@pytest.mark.parametrize("k,s", KS)
def test_survivor_count_at_sketch_size_and_buffer_capacity(mash, k, s):
    capf, capw = _caps(s)
    rng = np.random.default_rng(1000 + k)
    reads = []
    for want in (s - 1, s, s + 1, capf - 1, capf, capf + 1):
        read, surv = _with_survivors(rng, k, s, want)
        if want <= capf:  # the read stays in the slab pass only if no wave's segment overflows
            assert max(_wave_counts(surv)) <= capw, (want, _wave_counts(surv), capw)
        reads.append(read)
    _check(mash, reads, k, s)


def _unit_with_low_kmers(rng, k, s, p, m):
    """a unit of p bases of which exactly m cyclic k-mers survive the threshold of a read of L bases"""
    tau = _tauq(L - k, s)
    for _ in range(20_000):
        unit = rng.choice(list(b"ACGT"), p).astype(np.uint8).tobytes()
        ring = unit + unit[:k]
        hs = [orc.murmur3_32(ring[i:i + k]) for i in range(p)]
        if sum(h <= tau for h in hs) == m and len(set(hs)) == p:
            return unit
    raise AssertionError("no unit found")


@pytest.mark.parametrize("k,s", KS)
def test_as_many_big_bins_as_the_buffer_holds(mash, k, s):
    """a tandem repeat of `copies` units: each surviving k-mer of the unit fills one bin with `copies` equal values
    (> 32), and there are as many of them as capf allows"""
    capf, _ = _caps(s)
    rng = np.random.default_rng(2000 + k)
    copies = 40
    p = L // copies
    reads = []
    # (the k-mers of the last k positions of the unit lack their last copy: 39 or 40 of each)
    for m in (capf // copies, capf // copies - 1, s // copies + 2):
        unit = _unit_with_low_kmers(rng, k, s, p, m)
        reads.append(unit * copies)
    # 1,000 random bases + 36 units: big bins next to ordinary ones
    rnd = rng.choice(list(b"ACGT"), L - 36 * p).astype(np.uint8).tobytes()
    unit = _unit_with_low_kmers(rng, k, s, p, (capf - 2 * (L - 36 * p) * (s + 6 * int(math.sqrt(s)) + 16) // L) // 36)
    reads.append(rnd + unit * 36)
    _check(mash, reads, k, s)
