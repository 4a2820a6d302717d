"""Neighbour lists of the all-vs-all Mash join, restated from their definition (include/polyhip.h, "K2 neighbour lists").

shared(i, j) is the reference's sameHashes (mash.go:107-132, early-out of :117 included) -- the CPU oracle's
orc_mash_shared, or a numpy merge for ascending sketches that the CPU tests check against it.  Threshold,
self-exclusion, top-k with its tie rule, the ordering and 1 - c / s are plain Python."""
import numpy as np

import oracle as orc


def shared_matrix(X, Y):
    """counts[i][j] = X_i.Similarity(Y_j)'s sameHashes, pair by pair through the oracle (any sketches)"""
    out = np.zeros((len(X), len(Y)), np.uint16)
    for i, x in enumerate(X):
        x = np.ascontiguousarray(x, np.uint32)
        for j, y in enumerate(Y):
            out[i, j] = orc.mash_shared(x, np.ascontiguousarray(y, np.uint32))
    return out


def is_ascending(S):
    S = np.atleast_2d(S)
    return bool((S[:, 1:] >= S[:, :-1]).all())


def shared_row_ascending(x, Y):
    """sameHashes of one ASCENDING sketch against every row of an ASCENDING set: the two-pointer merge of sorted
    multisets counts min(multiplicity in x, multiplicity in Y_j) per value (disjoint ranges share nothing, so the
    early-out changes nothing)."""
    assert is_ascending(x) and is_ascending(Y)
    out = np.zeros(len(Y), np.int64)
    vals, mult = np.unique(x, return_counts=True)
    for v, a in zip(vals, mult):
        out += np.minimum((Y == v).sum(axis=1), a)
    return out.astype(np.uint16)


def shared_matrix_ascending(X, Y):
    return np.stack([shared_row_ascending(x, Y) for x in X]) if len(X) else np.zeros((0, len(Y)), np.uint16)


def neighbors_from_counts(counts, sx, sy, min_shared=1, k=0, exclude_self=False, self_offset=0):
    """(first, cols, shared, dist) of a dense count matrix"""
    assert min_shared >= 1
    nx = counts.shape[0]
    smaller = float(min(sx, sy))
    first, cols, shared, dist = [0], [], [], []
    for i in range(nx):
        row = counts[i]
        cand = [(int(j), int(row[j])) for j in np.nonzero(row >= min_shared)[0]]
        if exclude_self:
            cand = [(j, c) for j, c in cand if j != i + self_offset]
        if k > 0:
            cand.sort(key=lambda jc: (-jc[1], jc[0]))  # most shared first, ties towards the smaller column
            cand = cand[:k]
        for j, c in cand:
            cols.append(j)
            shared.append(c)
            dist.append(1 - float(c) / smaller)
        first.append(len(cols))
    return (np.array(first, np.uint64), np.array(cols, np.uint32), np.array(shared, np.uint16),
            np.array(dist, np.float64))


def neighbors(X, Y, min_shared=1, k=0, exclude_self=False, self_offset=0):
    X = np.atleast_2d(X)
    Y = np.atleast_2d(Y)
    return neighbors_from_counts(shared_matrix(X, Y), X.shape[1], Y.shape[1], min_shared, k, exclude_self, self_offset)


def assert_same(got, want, what=""):
    """entry for entry; distances by their bits"""
    names = ("first", "cols", "shared", "dist")
    for name, g, w in zip(names, got, want):
        if g is None:
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, f"{what}: {name} has {g.shape} entries, expected {w.shape}"
        if name == "dist":
            g, w = g.view(np.uint64), w.view(np.uint64)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {name}[{bad[0]}] = {g[bad[0]]}, expected {w[bad[0]]} ({bad.size} differ)"
