"""One seeded K2 input at the smallest shapes at which the bucket walk shared by the matrix join and the list join can go
wrong (BucketWalk in poly_amd/csrc/mash_distance.hip).  Built from integers, not sketched; the expected counts come from
the oracle's merge, pair by pair, once per row length.  Used by test_distance_gpu.py (as a matrix, in every join_kind)
and by test_mash_neighbors_gpu.py (as lists, in every walk form).

Y   700 sketches of 64 values.  24 planted values with 1, 60..70, 124..134 and 200 items between them: the index has 4096
    value buckets for these 44,800 items, each planted value has a bucket of its own (no other value comes within two
    bucket widths of it), so the bucket lengths are exactly those numbers -- on both sides of the walk's 64- and 128-item
    steps, one beyond them.  The first sketch of a planted value holds it 3 times, the second twice.
    Values stay below 2^21 (the issue asks for "below 2^30"): the bucket shift is then 9 and a sketch repeats a value at
    most 3 times, which is what the compact 4-byte item format takes -- larger values would leave the compact walk untested.
X   600 rows: more than two rounds of the 256-workgroup grid and a partial one, so the rows-ahead pipeline starts, runs and
    drains.  Every 7th row (86 of them) has two unequal elements swapped: non-ascending, the merge's, skipped by the walk
    between two regular rows.  Every 5th of the others holds SX distinct values of Y: as many non-empty buckets as the row
    is long (at SX = 1025 wave 0 gets a 65th descriptor, the second chunk).  The rest are the union of a few Y sketches'
    values, six planted values 1, 2 and 3 times, and random filler.
"""
import functools

import numpy as np

import oracle as orc

NY, SY, NX = 700, 64, 600
ROW_LENGTHS = (64, 1000, 1024, 1025)  # one wave / last wave holds 40 of 64 / full / staged, no rows ahead, second chunk
N_IRREGULAR_X = 86
COPIES = [1] + list(range(60, 71)) + list(range(124, 135)) + [200]
VALUE_BITS = 21
BUCKET_WIDTH = (1 << VALUE_BITS) >> 12  # 4096 buckets (16 items per bucket, a power of two, at least 2048)


def _sets(sx):
    rng = np.random.default_rng(0xB0C4)
    # planted values: each alone in its bucket, two bucket widths from the next one
    slots = rng.choice((1 << VALUE_BITS) // (4 * BUCKET_WIDTH) - 2, len(COPIES), replace=False) + 1
    planted = (slots * 4 * BUCKET_WIDTH + BUCKET_WIDTH // 2).astype(np.int64)
    filler = np.arange(1 << VALUE_BITS, dtype=np.int64)
    filler = filler[(np.abs(filler[:, None] - planted[None, :]) >= 2 * BUCKET_WIDTH).all(axis=1)]
    held = [[] for _ in range(NY)]
    for v, c in zip(planted, COPIES):
        times = [3, 2] + [1] * (c - 5) if c >= 6 else [1] * c
        for j, t in zip(rng.choice(NY, len(times), replace=False), times):
            held[j] += [v] * t
    Y = np.stack([np.sort(np.concatenate([np.array(h, np.int64), rng.choice(filler, SY - len(h), replace=False)])) for h in held])
    pool = np.unique(Y)
    X = np.empty((NX, sx), np.int64)
    for i in range(NX):
        if i % 7 != 0 and i % 5 == 2:
            X[i] = np.sort(rng.choice(pool, sx, replace=False))
            continue
        row = np.repeat(rng.choice(planted, 6, replace=False), [1, 2, 3, 1, 2, 3])
        per = min(SY, sx // 3)
        for j in rng.choice(NY, 2 if sx < 256 else 3, replace=False):
            row = np.concatenate([row, rng.choice(Y[j], per, replace=False)])
        X[i] = np.sort(np.concatenate([row, rng.choice(filler, sx - len(row))]))
        if i % 7 == 0:
            assert X[i, 0] != X[i, -1]
            X[i, [0, -1]] = X[i, [-1, 0]]
    return X.astype(np.uint32), Y.astype(np.uint32), planted


@functools.lru_cache(maxsize=None)
def case(sx):
    """-> (X, Y, counts): read-only arrays, computed once per row length and shared by every test that asks"""
    X, Y, planted = _sets(sx)
    # what the input is meant to be: exactly the planted rows are non-ascending, no Y sketch is, the planted buckets hold
    # exactly the planted numbers of items
    bad = (np.diff(X.astype(np.int64), axis=1) < 0).any(axis=1)
    assert bad.tolist() == [i % 7 == 0 for i in range(NX)] and int(bad.sum()) == N_IRREGULAR_X
    assert not (np.diff(Y.astype(np.int64), axis=1) < 0).any()
    lengths = np.bincount(Y.reshape(-1) // BUCKET_WIDTH, minlength=4096)
    assert lengths[planted // BUCKET_WIDTH].tolist() == COPIES
    assert max(len(np.unique(x)) for x in X) == sx
    shared = orc.lib().orc_mash_shared
    xp, yp = [x.ctypes.data for x in X], [y.ctypes.data for y in Y]
    M = np.array([[shared(a, sx, b, SY) for b in yp] for a in xp], np.uint16)
    assert M.max() >= 20 and (M == 0).any()
    for a in (X, Y, M):
        a.setflags(write=False)
    return X, Y, M
