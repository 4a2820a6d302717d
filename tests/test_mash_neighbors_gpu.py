"""K2 neighbour lists on the GPU (poly_amd.mash.neighbors_dev / neighbors_packed, through the C ABI), entry for entry
against tests/mash_neighbors_oracle.py, and -- wherever the dense matrix fits -- against the dense path's own
shared_counts_dev / distance_from_counts_dev output filtered on the host (an independent cross-check: the dense join
and its distance kernel are not the code under test)."""
import numpy as np
import pytest

import k2_walk_shapes
import oracle as orc
import mash_neighbors_oracle as nbo

pytestmark = pytest.mark.gpu

GUARD = 64  # entries behind the capacity that must keep their pattern


@pytest.fixture(scope="module")
def mash():
    from poly_amd import mash
    return mash


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda:0")


WALKS = ("default", "staged", "wide", "staged-wide")


@pytest.fixture
def walk(request, monkeypatch):
    """the join's walk in one of its forms: a row of at most 1024 hashes in registers or staged in LDS
    (POLYHIP_K2_REGROW=0), compact 4-byte items where they fit or 8-byte ones (POLYHIP_K2_COMPACT=0).  A test that does
    not parametrise it (indirect) runs the default form, with both variables unset."""
    form = getattr(request, "param", "default")
    monkeypatch.delenv("POLYHIP_K2_REGROW", raising=False)
    monkeypatch.delenv("POLYHIP_K2_COMPACT", raising=False)
    if "staged" in form:
        monkeypatch.setenv("POLYHIP_K2_REGROW", "0")
    if "wide" in form:
        monkeypatch.setenv("POLYHIP_K2_COMPACT", "0")
    return form


def _t(a, dev):
    import torch
    return torch.from_numpy(np.array(a, np.uint32, order="C").view(np.int32)).to(dev)  # (a copy: shared inputs are read-only)


def run_dev(mash, dev, X, Y, min_shared=1, k=0, exclude_self=False, self_offset=0, capacity=None, want_dist=True, Xt=None,
            Yt=None):
    """neighbors_dev with a guard region behind the capacity; capacity None: the counts first, then a call at first[nx].
    -> (first, cols, shared, dist) of the entries that fit, as numpy"""
    import torch
    Xt = _t(X, dev) if Xt is None else Xt
    Yt = _t(Y, dev) if Yt is None else Yt
    nx, sx = Xt.shape
    ny, sy = Yt.shape
    work = torch.empty(mash.neighbors_workspace_bytes(nx, sx, ny, sy), dtype=torch.uint8, device=dev)
    first = torch.full((nx + 1,), -1, dtype=torch.int64, device=dev)
    if capacity is None:
        mash.neighbors_dev(Xt, Yt, first, None, None, None, work, min_shared, k, exclude_self, self_offset)
        torch.cuda.synchronize()
        capacity = int(first[nx].item())
        counted = first.cpu().numpy().copy()
        first.fill_(-1)
    else:
        counted = None
    cols = torch.full((capacity + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    shared = torch.full((capacity + GUARD,), 0x5A5A, dtype=torch.int16, device=dev)
    dist = torch.full((capacity + GUARD,), -7.0, dtype=torch.float64, device=dev) if want_dist else None
    mash.neighbors_dev(Xt, Yt, first, cols[:capacity], shared[:capacity], dist[:capacity] if want_dist else None, work, min_shared,
                       k, exclude_self, self_offset)
    torch.cuda.synchronize()
    assert (cols[capacity:] == 0x5A5A5A5A).all() and (shared[capacity:] == 0x5A5A).all(), "written beyond the capacity"
    if want_dist:
        assert (dist[capacity:] == -7.0).all(), "written beyond the capacity"
    f = first.cpu().numpy().view(np.uint64)
    if counted is not None:
        assert (counted.view(np.uint64) == f).all(), "the count-only call and the filling call disagree on first[]"
    n = min(capacity, int(f[nx]))
    return (f, cols[:n].cpu().numpy().view(np.uint32), shared[:n].cpu().numpy().view(np.uint16),
            dist[:n].cpu().numpy() if want_dist else None)


def dense_counts(mash, dev, X, Y, Xt=None, Yt=None, want_dist=True):
    """the dense path: counts (u16) and distances of every pair, as numpy"""
    import torch
    Xt = _t(X, dev) if Xt is None else Xt
    Yt = _t(Y, dev) if Yt is None else Yt
    nx, sx = Xt.shape
    ny, sy = Yt.shape
    ct = torch.zeros((nx, ny), dtype=torch.int16, device=dev)
    work = torch.empty(mash.shared_counts_workspace_bytes(nx, sx, ny, sy), dtype=torch.uint8, device=dev)
    mash.shared_counts_dev(Xt, Yt, ct, work)
    dt = None
    if want_dist:
        dt = torch.zeros((nx, ny), dtype=torch.float64, device=dev)
        mash.distance_from_counts_dev(ct, sx, sy, dt)
    torch.cuda.synchronize()
    return ct.cpu().numpy().view(np.uint16), dt.cpu().numpy() if want_dist else None


def dense_filter(counts, dist, min_shared=1, k=0, exclude_self=False, self_offset=0):
    """the dense matrices filtered on the host: (first, cols, shared, dist), distances TAKEN from the dense kernel's"""
    nx, ny = counts.shape
    keep = counts >= min_shared
    if exclude_self:
        i = np.arange(nx)
        j = i + self_offset
        ok = j < ny
        keep[i[ok], j[ok]] = False
    if k == 0:
        r, c = np.nonzero(keep)  # row-major: rows in order, ascending column
        first = np.zeros(nx + 1, np.uint64)
        first[1:] = np.cumsum(keep.sum(axis=1, dtype=np.int64))
        return first, c.astype(np.uint32), counts[r, c], (dist[r, c] if dist is not None else None)
    first, cols = [0], []
    for i in range(nx):
        c = np.nonzero(keep[i])[0]
        order = np.lexsort((c, -counts[i, c].astype(np.int64)))[:k]  # shared descending, then column ascending
        cols.append(c[order])
        first.append(first[-1] + len(order))
    rows = np.repeat(np.arange(nx), np.diff(first))
    cols = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    return (np.array(first, np.uint64), cols.astype(np.uint32), counts[rows, cols],
            dist[rows, cols] if dist is not None else None)


def check_all(mash, dev, X, Y, what, oracle_counts=None, **kw):
    """one case three ways: the GPU list == the oracle's == the dense path's cells filtered on the host"""
    got = run_dev(mash, dev, X, Y, **kw)
    M = nbo.shared_matrix(X, Y) if oracle_counts is None else oracle_counts
    want = nbo.neighbors_from_counts(M, X.shape[1], Y.shape[1], **kw)
    nbo.assert_same(got, want, what + " vs oracle")
    dc, dd = dense_counts(mash, dev, X, Y)
    assert (dc == M).all()
    nbo.assert_same(got, dense_filter(dc, dd, **kw), what + " vs the dense path")
    return got


def _families(rng, nfam, copies, L, sub, k, s):
    """SURVEY 8d C3 generator in miniature: families of mutated copies, sketched by the oracle."""
    seqs = []
    for _ in range(nfam):
        g = rng.choice(list(b"ACGT"), L).astype(np.uint8)
        for _ in range(copies):
            m = g.copy()
            hit = rng.random(L) < sub
            m[hit] = rng.choice(list(b"ACGT"), int(hit.sum())).astype(np.uint8)
            seqs.append(m.tobytes())
    buf = np.frombuffer(b"".join(seqs), np.uint8)
    offs = np.arange(0, (len(seqs) + 1) * L, L, dtype=np.uint64)
    return orc.mash_sketch_batch(buf, offs, k, s)


@pytest.mark.parametrize("s,nfam,copies,L", [(200, 6, 8, 1500), (1000, 4, 6, 4000), (2000, 3, 5, 6000)])
def test_families_threshold_and_topk(mash, dev, walk, s, nfam, copies, L):
    """10-bit counters (s = 200, 1000) and 16-bit ones (s = 2000; rows beyond 1024 hashes are staged in LDS)"""
    rng = np.random.default_rng(s)
    S = _families(rng, nfam, copies, L, 0.01, 21, s)
    M = nbo.shared_matrix(S, S)
    assert (M.diagonal() == s).all() and (M == 0).any()
    for ms in (1, 2, s // 2, s):
        check_all(mash, dev, S, S, f"s={s} min_shared={ms}", oracle_counts=M, min_shared=ms)
    for k in (1, 3, len(S) + 5):
        check_all(mash, dev, S, S, f"s={s} k={k}", oracle_counts=M, k=k)
        check_all(mash, dev, S, S, f"s={s} k={k} no self", oracle_counts=M, k=k, exclude_self=True, min_shared=2)
    info = mash.neighbors_last_info()
    assert info["column_blocks"] == 1 and info["assembly"] == 1 and info["row_chunks"] == 1


@pytest.mark.parametrize("walk", WALKS[1:], indirect=True)
@pytest.mark.parametrize("s,nfam,copies,L", [(200, 6, 8, 1500), (1000, 4, 6, 4000), (2000, 3, 5, 6000)])
def test_families_threshold_and_topk_in_the_other_walk_forms(mash, dev, walk, s, nfam, copies, L):
    """the test above (the default walk) with the row staged, with 8-byte items, and with both: the same assertions"""
    test_families_threshold_and_topk(mash, dev, walk, s, nfam, copies, L)


def test_forced_ties_in_topk(mash, dev):
    """many columns share exactly as much with a row: the k best are the SMALLER columns"""
    rng = np.random.default_rng(21)
    base = np.sort(rng.choice(1 << 28, 64, replace=False).astype(np.uint32))
    Y = np.sort(rng.integers(1 << 28, 1 << 30, (40, 64), dtype=np.uint32), axis=1)
    for j in range(0, 40, 3):  # columns 0, 3, 6, ... share the same 20 hashes with the row; 1, 4, 7, ... the same 7
        Y[j, :20] = base[:20]
        Y[j].sort()
    for j in range(1, 40, 3):
        Y[j, :7] = base[:7]
        Y[j].sort()
    X = np.stack([base, Y[3], Y[4]])
    M = nbo.shared_matrix(X, Y)
    assert (M[0, 0::3] == 20).all() and (M[0, 1::3] == 7).all()
    for k in (1, 3, 14, 15, 27, 100):
        got = check_all(mash, dev, X, Y, f"ties k={k}", oracle_counts=M, k=k)
        assert got[1][:min(k, 14)].tolist() == list(range(0, 40, 3))[:k]
    check_all(mash, dev, X, Y, "ties k=3 no self", oracle_counts=M, k=3, exclude_self=True, self_offset=3)  # row 1 is column 4


def test_different_sketch_sizes_and_duplicates(mash, dev, walk):
    rng = np.random.default_rng(5)
    X = np.sort(rng.integers(0, 40, (30, 64), dtype=np.uint32), axis=1)  # heavy duplication: multiset semantics
    Y = np.sort(rng.integers(0, 40, (25, 48), dtype=np.uint32), axis=1)
    for kw in (dict(), dict(min_shared=30), dict(k=4), dict(min_shared=48)):
        check_all(mash, dev, X, Y, f"sx != sy {kw}", **kw)
        check_all(mash, dev, Y, X, f"sy != sx {kw}", **kw)
    # sketch sizes on either side of the 10-bit counters' limit
    A = np.sort(rng.integers(0, 1 << 30, (6, 1200), dtype=np.uint32), axis=1)
    B = np.sort(rng.integers(0, 1 << 30, (9, 300), dtype=np.uint32), axis=1)
    B[2, :200] = A[1, 100:300]
    B[2].sort()
    B[7] = B[2]
    check_all(mash, dev, A, B, "sx=1200 sy=300")
    check_all(mash, dev, B, A, "sx=300 sy=1200", k=2)
    # duplicated sketches: every copy lists every other copy
    S = _families(rng, 3, 1, 1500, 0.0, 21, 200)
    D = np.concatenate([S, S, S[:1], S])
    got = check_all(mash, dev, D, D, "duplicated sketches", exclude_self=True, min_shared=200)
    assert (np.diff(got[0].astype(np.int64)) >= 2).all()


@pytest.mark.parametrize("walk", WALKS[1:], indirect=True)
def test_different_sketch_sizes_and_duplicates_in_the_other_walk_forms(mash, dev, walk):
    """the test above (the default walk) with the row staged, with 8-byte items, and with both: the same assertions"""
    test_different_sketch_sizes_and_duplicates(mash, dev, walk)


@pytest.mark.parametrize("walk", WALKS, indirect=True)
@pytest.mark.parametrize("sx", k2_walk_shapes.ROW_LENGTHS)
def test_walk_shapes(mash, dev, walk, sx):
    """the bucket walk at its edges (tests/k2_walk_shapes.py), as lists: every non-zero cell, and the 3 best per row"""
    X, Y, M = k2_walk_shapes.case(sx)
    check_all(mash, dev, X, Y, f"walk shapes sx={sx} {walk}", oracle_counts=M, min_shared=1)
    check_all(mash, dev, X, Y, f"walk shapes sx={sx} {walk} k=3", oracle_counts=M, k=3)


def test_exclude_self_in_a_row_block(mash, dev):
    rng = np.random.default_rng(8)
    S = _families(rng, 5, 6, 1500, 0.02, 21, 200)
    M = nbo.shared_matrix(S, S)
    whole = check_all(mash, dev, S, S, "whole set, no self", oracle_counts=M, exclude_self=True)
    assert int(whole[0][-1]) == int((M >= 1).sum()) - len(S)
    for r0, r1 in ((0, 7), (7, 19), (19, 30)):
        got = check_all(mash, dev, S[r0:r1], S, f"rows {r0}:{r1}", oracle_counts=M[r0:r1], exclude_self=True, self_offset=r0)
        lo, hi = int(whole[0][r0]), int(whole[0][r1])
        assert (got[1] == whole[1][lo:hi]).all() and (got[2] == whole[2][lo:hi]).all()  # row blocks concatenate
        check_all(mash, dev, S[r0:r1], S, f"rows {r0}:{r1} k=2", oracle_counts=M[r0:r1], exclude_self=True, self_offset=r0, k=2)
    # a self column beyond Y excludes nothing
    check_all(mash, dev, S[:4], S, "self beyond ny", oracle_counts=M[:4], exclude_self=True, self_offset=1000)


def test_dist_bits_equal_the_distance_kernels(mash, dev):
    rng = np.random.default_rng(13)
    for sx, sy in ((10, 10), (10, 9), (5, 10), (1000, 1000), (2000, 1500)):
        X = np.sort(rng.integers(0, 4 * max(sx, sy), (12, sx), dtype=np.uint32), axis=1)
        Y = np.sort(rng.integers(0, 4 * max(sx, sy), (15, sy), dtype=np.uint32), axis=1)
        got = run_dev(mash, dev, X, Y)
        dc, dd = dense_counts(mash, dev, X, Y)
        want = dense_filter(dc, dd)
        nbo.assert_same(got, want, f"dist bits {sx}x{sy}")
        assert len(set(got[2].tolist())) >= 3  # several distinct counts, so several distinct quotients
        r = np.repeat(np.arange(12), np.diff(got[0].astype(np.int64)))
        for e in range(0, len(r), 7):  # and the oracle's own division
            assert got[3][e] == orc.lib().orc_mash_distance(X[r[e]].ctypes.data, sx, Y[got[1][e]].ctypes.data, sy)


def test_capacity(mash, dev):
    import torch
    rng = np.random.default_rng(17)
    S = _families(rng, 4, 8, 1500, 0.01, 21, 200)
    full = run_dev(mash, dev, S, S)
    total = int(full[0][-1])
    assert total >= 4 * 64
    for kw in (dict(), dict(k=3)):
        full = run_dev(mash, dev, S, S, **kw)
        total = int(full[0][-1])
        for cap in (0, 1, total // 2, total - 1):
            got = run_dev(mash, dev, S, S, capacity=cap, **kw)  # (the guard region is checked inside)
            assert (got[0] == full[0]).all(), "first[] must carry the true counts whatever the capacity"
            assert len(got[1]) == cap
            assert (got[1] == full[1][:cap]).all() and (got[2] == full[2][:cap]).all()
            assert (got[3].view(np.uint64) == full[3][:cap].view(np.uint64)).all()
        again = run_dev(mash, dev, S, S, capacity=total, **kw)  # the repeated call at first[nx]
        nbo.assert_same(again, full, "second call at first[nx]")
    # the count-only form writes first[] and nothing else
    St = _t(S, dev)
    first = torch.zeros(len(S) + 1, dtype=torch.int64, device=dev)
    work = torch.empty(mash.neighbors_workspace_bytes(len(S), 200, len(S), 200), dtype=torch.uint8, device=dev)
    mash.neighbors_dev(St, St, first, None, None, None, work)
    torch.cuda.synchronize()
    assert (first.cpu().numpy().view(np.uint64) == run_dev(mash, dev, S, S)[0]).all()


def _irregular_set(rng):
    S = np.sort(rng.integers(0, 1 << 30, (40, 100), dtype=np.uint32), axis=1)
    S[5, :50] = S[6, :50]                                      # two related sketches
    S[5].sort(); S[6].sort()
    S[3] = rng.integers(0, 1 << 30, 100, dtype=np.uint32)      # an unsorted row
    S[3, :30] = S[6, 20:50]                                    # ... that shares hashes with regular ones
    S[11] = S[6, 10]                                           # one repeated hash
    S[12] = S[6, 10]
    S[17] = S[5]
    S[17, 60:] = 0                                             # a short sequence's sketch over zeros
    S[23] = S[6]
    S[23, :40] = np.sort(rng.integers(0, 1 << 30, 40, dtype=np.uint32))  # a stale prior Sketches: new prefix over an old sketch
    S[29] = 0                                                  # mash.New, never sketched
    return S


def test_irregular_sketches(mash, dev):
    rng = np.random.default_rng(9)
    S = _irregular_set(rng)
    assert not nbo.is_ascending(S[3]) and not nbo.is_ascending(S[17]) and not nbo.is_ascending(S[23])
    R = np.sort(rng.integers(0, 1 << 30, (12, 100), dtype=np.uint32), axis=1)  # a regular set related to S
    R[2, :60] = S[6, :60]
    R[2].sort()
    R[7] = S[5]
    for X, Y, what in ((S, S, "both sides"), (S, R, "the X side"), (R, S, "the Y side")):
        M = nbo.shared_matrix(X, Y)
        assert (M > 0).sum() >= 8
        check_all(mash, dev, X, Y, f"irregular on {what}", oracle_counts=M)
        check_all(mash, dev, X, Y, f"irregular on {what}, min_shared 2", oracle_counts=M, min_shared=2)
        check_all(mash, dev, X, Y, f"irregular on {what}, k=2", oracle_counts=M, k=2, exclude_self=what == "both sides")
    # a 1500-hash set (16-bit counters, rows staged in LDS) with irregular sketches on both sides
    T = np.sort(rng.integers(0, 1 << 30, (10, 1500), dtype=np.uint32), axis=1)
    T[1, :700] = T[0, :700]
    T[1].sort()
    T[4] = T[0][::-1]
    T[6] = T[1]
    T[6, 900:] = 0
    check_all(mash, dev, T, T, "irregular, s = 1500", exclude_self=True)


def test_wide_y_goes_in_column_blocks(mash, dev):
    """250,000 sketches of 16 hashes: three column blocks, each with its own index; neighbours in the first, a middle
    and the last block arrive in ascending column order"""
    ny, s = 250_000, 16
    rng = np.random.default_rng(31)
    Y = np.sort(rng.integers(0, 1 << 31, (ny, s), dtype=np.uint32), axis=1)
    rows = [5, 60_000, 113_000, 113_600, 130_000, 200_000, 230_000, 249_999]
    X = Y[rows].copy()
    planted = {0: [7, 120_000, 249_998], 1: [113_495, 113_496, 113_497], 2: [0, 226_991, 226_992, 226_993], 4: [249_000]}
    for r, colsr in planted.items():
        for q, j in enumerate(colsr):
            Y[j, :8 + q] = X[r, :8 + q]
            Y[j].sort()
    Y[150_000] = X[3]              # an irregular column in the middle block: row 3's hashes, two of them out of order
    Y[150_000, [4, 5]] = Y[150_000, [5, 4]]
    X[6, [9, 10]] = X[6, [10, 9]]  # and an irregular row
    assert not nbo.is_ascending(Y[150_000]) and not nbo.is_ascending(X[6])
    reg = [i for i in range(len(X)) if i != 6]
    Yasc = Y.copy()
    Yasc[150_000].sort()           # (placeholder: that column comes from the oracle below)
    M = np.zeros((len(X), ny), np.uint16)
    M[reg] = nbo.shared_matrix_ascending(X[reg], Yasc)
    for i in range(len(X)):
        M[i, 150_000] = orc.mash_shared(X[i], Y[150_000])
    M[6] = [orc.mash_shared(X[6], y) for y in Y]  # the irregular row: the merge as it stands, pair by pair
    assert M[3, 150_000] >= 1 and M[6, 230_000] >= 1
    Xt, Yt = _t(X, dev), _t(Y, dev)
    for kw in (dict(), dict(min_shared=9), dict(k=2), dict(k=3, exclude_self=True, self_offset=0)):
        got = run_dev(mash, dev, X, Y, Xt=Xt, Yt=Yt, **kw)
        nbo.assert_same(got, nbo.neighbors_from_counts(M, s, s, **kw), f"wide Y {kw}")
        info = mash.neighbors_last_info()
        assert info["column_blocks"] == 3 and info["index_builds"] == 3, info
    got = run_dev(mash, dev, X, Y, Xt=Xt, Yt=Yt)
    f = got[0].astype(np.int64)
    assert set(planted[0]) <= set(got[1][f[0]:f[1]].tolist())       # first, middle and last block in one row
    assert set(planted[2]) <= set(got[1][f[2]:f[3]].tolist())       # both sides of a block boundary
    assert 150_000 in got[1][f[3]:f[4]].tolist()                    # the irregular column
    # and the dense path agrees (it stripes such a set itself)
    dc, dd = dense_counts(mash, dev, X, Y, Xt=Xt, Yt=Yt)
    nbo.assert_same(got, dense_filter(dc, dd), "wide Y vs the dense path")


def test_temporary_list_overflow_splits_the_rows(mash, dev):
    """more survivors than the temporary list holds (1024 per row): the rows are joined again in pieces, same list"""
    rng = np.random.default_rng(41)
    base = np.sort(rng.choice(1 << 30, 32, replace=False).astype(np.uint32))
    Y = np.tile(base, (3000, 1))
    Y[:, 16:] = np.sort(rng.integers(0, 1 << 30, (3000, 16), dtype=np.uint32), axis=1)
    Y.sort(axis=1)
    X = Y[:1500].copy()  # every row shares >= 16 hashes with every column: 4.5M entries, the list holds 1.5M
    got = run_dev(mash, dev, X, Y, min_shared=16)
    info = mash.neighbors_last_info()
    assert info["row_chunks"] > 1 and info["entries"] == 1500 * 3000
    dc, dd = dense_counts(mash, dev, X, Y)
    nbo.assert_same(got, dense_filter(dc, dd, min_shared=16), "overflowing list vs the dense path")
    got = run_dev(mash, dev, X, Y, min_shared=16, k=5, exclude_self=True)
    nbo.assert_same(got, dense_filter(dc, dd, min_shared=16, k=5, exclude_self=True), "overflowing list, k=5")


def test_empty_sets_and_errors(mash, dev):
    import torch
    from poly_amd import _lib
    S = np.sort(np.random.default_rng(1).integers(0, 1 << 30, (5, 32), dtype=np.uint32), axis=1)
    E = np.zeros((0, 32), np.uint32)
    for X, Y in ((E, S), (S, E), (E, E)):
        got = run_dev(mash, dev, X, Y, capacity=0)
        assert got[0].tolist() == [0] * (len(X) + 1) and got[1].size == 0
        f, c, s, d = mash.neighbors_packed(X, Y)
        assert f.tolist() == [0] * (len(X) + 1) and c.size == s.size == d.size == 0
    St = _t(S, dev)
    first = torch.zeros(6, dtype=torch.int64, device=dev)
    work = torch.empty(mash.neighbors_workspace_bytes(5, 32, 5, 32), dtype=torch.uint8, device=dev)
    Z = torch.zeros((5, 0), dtype=torch.int32, device=dev)
    for a, b in ((Z, St), (St, Z)):
        with pytest.raises(_lib.PolyhipError) as ei:
            mash.neighbors_dev(a, b, first, None, None, None, work)
        assert ei.value.status == _lib.ERR_PANIC and "mash.go:117" in str(ei.value)
    with pytest.raises(_lib.PolyhipError) as ei:
        mash.neighbors_dev(St, St, first, None, None, None, work, min_shared=0)
    assert ei.value.status == _lib.ERR_INVALID and "min_shared" in str(ei.value)
    mash.neighbors_dev(St, St, first, None, None, None, work, k=1024)  # POLYHIP_MASH_NEIGHBORS_MAX_K itself is served
    with pytest.raises(_lib.PolyhipError) as ei:
        mash.neighbors_dev(St, St, first, None, None, None, work, k=1025)
    assert ei.value.status == _lib.ERR_INVALID and "MAX_K" in str(ei.value)
    with pytest.raises(_lib.PolyhipError) as ei:
        mash.neighbors_dev(St, St, first, None, None, None, work[:1024])
    assert ei.value.status == _lib.ERR_INVALID and "workspace" in str(ei.value)
    big = torch.zeros((1, 65536), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.PolyhipError) as ei:
        mash.neighbors_dev(St, big, first, None, None, None, work)
    assert ei.value.status == _lib.ERR_INVALID and "65535" in str(ei.value)


def test_host_entry_point_and_a_device_list(mash, dev):
    from poly_amd import devices
    rng = np.random.default_rng(19)
    S = _families(rng, 5, 7, 1500, 0.01, 21, 200)
    S[9] = S[9][::-1]
    M = nbo.shared_matrix(S, S)
    try:
        for kw in (dict(), dict(k=3, exclude_self=True), dict(min_shared=100, exclude_self=True)):
            devices.set_devices([])
            one = mash.neighbors_packed(S, S, **kw)
            nbo.assert_same(one, nbo.neighbors_from_counts(M, 200, 200, **kw), f"host entry point {kw}")
            nbo.assert_same(one, run_dev(mash, dev, S, S, **kw), f"host vs device entry point {kw}")
            assert mash.neighbors_last_info()["devices"] == 1
            for ids in ([0, 0], [0, 0, 0], [0] * 8):
                devices.set_devices(ids)
                many = mash.neighbors_packed(S, S, **kw)
                nbo.assert_same(many, one, f"device list {ids} {kw}")
                assert mash.neighbors_last_info()["devices"] == len(ids)
            devices.set_devices([0, 0, 0])
            nd = mash.neighbors_packed(S, S, want_dist=False, **kw)
            assert nd[3] is None and (nd[1] == one[1]).all()
        devices.set_devices([0, 0])
        lists = mash.Neighbors([_as_mash(mash, s) for s in S[:12]], min_shared=2, k=2)
        nbo.assert_same(lists, nbo.neighbors_from_counts(M[:12, :12], 200, 200, 2, 2, True, 0), "Neighbors()")
    finally:
        devices.set_devices([])


def _as_mash(mash, sk):
    m = mash.New(21, len(sk))
    m.Sketches = sk.copy()
    return m


def test_same_input_same_bytes(mash, dev):
    rng = np.random.default_rng(23)
    S = _families(rng, 8, 12, 1500, 0.01, 21, 200)
    for kw in (dict(), dict(k=4, exclude_self=True)):
        a = run_dev(mash, dev, S, S, **kw)
        b = run_dev(mash, dev, S, S, **kw)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_full_size_config3_row_block(mash, dev):
    """The configs[2] row block, 12,500 x 100,000 sketches of 1000 hashes: at min_shared = 1 the list is EVERY non-zero
    cell of the dense block; then the 10 nearest per row without the row itself, against a host top-k of the block."""
    import torch
    from poly_amd import bench_extra
    sk = bench_extra.family_sketches(dev, 1000, 100, 10_000, 21, 1000, seed=0xC3)
    nx, ny = 12_500, 100_000
    Xt = sk[:nx]
    dc, _ = dense_counts(mash, dev, None, None, Xt=Xt, Yt=sk, want_dist=False)
    got = run_dev(mash, dev, None, None, Xt=Xt, Yt=sk)
    info = mash.neighbors_last_info()
    print("full size: entries", int(got[0][-1]), info)
    assert info["column_blocks"] == 1 and info["row_chunks"] == 1
    first = np.zeros(nx + 1, np.uint64)
    first[1:] = np.cumsum((dc != 0).sum(axis=1, dtype=np.int64))
    r, c = np.nonzero(dc)
    assert (got[0] == first).all()
    assert (got[1] == c.astype(np.uint32)).all() and (got[2] == dc[r, c]).all()
    assert (got[3].view(np.uint64) == (1 - dc[r, c].astype(np.float64) / 1000.0).view(np.uint64)).all()
    del r, c
    top = run_dev(mash, dev, None, None, Xt=Xt, Yt=sk, k=10, exclude_self=True)
    want = dense_filter(dc, None, k=10, exclude_self=True)
    nbo.assert_same(top[:3], want[:3], "full size k=10")
    assert (top[3].view(np.uint64) == (1 - want[2].astype(np.float64) / 1000.0).view(np.uint64)).all()
    del sk
    torch.cuda.empty_cache()
