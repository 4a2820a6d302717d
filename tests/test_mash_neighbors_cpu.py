"""CPU-only checks of the K2 neighbour lists: the restatement the GPU tests compare against (tests/mash_neighbors_oracle.py)
on the reference's TestMash sketches, on hand-made ties and on irregular sketches; and the drop-in boundary -- the header
declares the new entry points and the library built here exports them."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import oracle as orc
import mash_neighbors_oracle as nbo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("polyhip_mash_neighbors_workspace_bytes", "polyhip_mash_neighbors_dev", "polyhip_mash_neighbors",
       "polyhip_mash_neighbors_last_info")


def _testmash():
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "mash", "testmash_sketch_inputs.json")))
    sk = {}
    for e in spec["sketches"]:
        m = orc.Mash(e["k"], e["s"])
        if e["seq"] is not None:
            m.Sketch(e["seq"])
        sk[e["name"]] = m
    return spec, sk


def test_header_declares_and_library_exports_the_neighbour_entry_points():
    src = open(os.path.join(ROOT, "include", "polyhip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(polyhip_[a-z0-9_]+)\s*\(", src))
    from poly_amd import build, _lib
    L = C.CDLL(build.build_lib())
    for n in NEW:
        assert n in declared, f"{n} is not declared in polyhip.h"
        assert hasattr(L, n), f"{n} is not exported by libpolyhip.so"
        assert n in _lib.SIGNATURES
    assert _lib.lib().polyhip_abi_version() == 1  # additive: the version stays
    from poly_amd import mash
    for f in ("neighbors_packed", "Neighbors", "neighbors_dev", "neighbors_workspace_bytes", "neighbors_last_info"):
        assert callable(getattr(mash, f))
    # a workspace for a 1M x 1M set of 1000-hash sketches is a few GB (one block index + the temporary list), not nx * ny
    assert mash.neighbors_workspace_bytes(1_000_000, 1000, 1_000_000, 1000) < 16 << 30
    assert mash.neighbors_workspace_bytes(0, 1000, 0, 1000) > 0


def test_argument_errors_need_no_device():
    """SketchSize 0 is the reference's panic, sizes beyond the u16 counts and min_shared 0 are refused: all before any
    device call, with the dense path's messages"""
    from poly_amd import _lib, mash
    X = np.zeros((2, 4), np.uint32)
    with pytest.raises(_lib.PolyhipError) as ei:
        mash.neighbors_packed(np.zeros((2, 0), np.uint32), X)
    assert ei.value.status == _lib.ERR_PANIC and "mash.go:117" in str(ei.value)
    with pytest.raises(_lib.PolyhipError) as ei:
        mash.neighbors_packed(X, np.zeros((1, 65536), np.uint32))
    assert ei.value.status == _lib.ERR_INVALID and "65535" in str(ei.value)
    with pytest.raises(_lib.PolyhipError) as ei:
        mash.neighbors_packed(X, X, min_shared=0)
    assert ei.value.status == _lib.ERR_INVALID and "min_shared" in str(ei.value)
    for a, b in ((np.zeros((0, 4), np.uint32), X), (X, np.zeros((0, 4), np.uint32))):
        first, cols, shared, dist = mash.neighbors_packed(a, b)
        assert first.tolist() == [0] * (len(a) + 1) and cols.size == shared.size == dist.size == 0


def test_oracle_on_TestMash_sketches():
    """search/mash/mash_test.go:9-62: the distances the reference asserts come out of the lists"""
    spec, sk = _testmash()
    for d in spec["distances"]:
        a, b = sk[d["a"]], sk[d["b"]]
        first, cols, shared, dist = nbo.neighbors(a.Sketches, b.Sketches, 1)
        if "equals" in d and d["equals"] == 1:
            assert first.tolist() == [0, 0]  # nothing shared: never listed
            continue
        assert first.tolist() == [0, 1] and cols.tolist() == [0]
        assert dist[0] == a.Distance(b)
        if "equals" in d:
            assert dist[0] == d["equals"]
        else:
            assert d["between"][0] < dist[0] < d["between"][1]
    # 8 shared of min(10, 5) ... the value the reference prints for that pair: 1 - 4/5
    a, b = sk["f1"], sk["f5a"]
    assert nbo.neighbors(a.Sketches, b.Sketches)[3][0] == 1 - float(orc.mash_shared(a.Sketches, b.Sketches)) / 5.0
    # all of them as one set of equal SketchSize (the 10-hash ones): row i's list against the others
    S = np.stack([sk[n].Sketches for n in ("f1", "spoofed10", "f10b")])
    first, cols, shared, dist = nbo.neighbors(S, S, 1, 0, True, 0)
    M = nbo.shared_matrix(S, S)
    for i in range(3):
        want = [j for j in range(3) if j != i and M[i, j] >= 1]
        assert cols[first[i]:first[i + 1]].tolist() == want


def test_oracle_ties_and_ordering():
    # row 0 shares 3, 2, 3, 0, 2, 3 hashes with the six columns
    x = np.array([[10, 20, 30, 40]], np.uint32)
    Y = np.array([[10, 20, 30, 99], [10, 20, 77, 99], [20, 30, 40, 99], [1, 2, 3, 4], [5, 30, 40, 99], [10, 30, 40, 99]],
                 np.uint32)
    assert nbo.shared_matrix(x, Y).tolist() == [[3, 2, 3, 0, 2, 3]]
    f, c, s, d = nbo.neighbors(x, Y, 1)
    assert (f.tolist(), c.tolist(), s.tolist()) == ([0, 5], [0, 1, 2, 4, 5], [3, 2, 3, 2, 3])  # ascending column
    assert d.tolist() == [1 - 3 / 4.0, 1 - 2 / 4.0, 1 - 3 / 4.0, 1 - 2 / 4.0, 1 - 3 / 4.0]
    f, c, s, _ = nbo.neighbors(x, Y, 3)
    assert (c.tolist(), s.tolist()) == ([0, 2, 5], [3, 3, 3])
    f, c, s, _ = nbo.neighbors(x, Y, 1, k=2)
    assert (c.tolist(), s.tolist()) == ([0, 2], [3, 3])  # ties towards the smaller column
    f, c, s, _ = nbo.neighbors(x, Y, 1, k=4)
    assert (c.tolist(), s.tolist()) == ([0, 2, 5, 1], [3, 3, 3, 2])
    f, c, s, _ = nbo.neighbors(x, Y, 1, k=100)  # fewer candidates than k: all of them, in top-k order
    assert (f.tolist(), c.tolist()) == ([0, 5], [0, 2, 5, 1, 4])
    f, c, s, _ = nbo.neighbors(x, Y, 1, k=2, exclude_self=True, self_offset=0)  # row 0 is column 0
    assert c.tolist() == [2, 5]
    f, c, s, _ = nbo.neighbors(x, Y, 1, k=0, exclude_self=True, self_offset=2)
    assert c.tolist() == [0, 1, 4, 5]
    f, c, s, _ = nbo.neighbors(x, Y, 5)
    assert f.tolist() == [0, 0] and c.size == 0


def test_numpy_merge_equals_the_oracle_on_ascending_sketches():
    rng = np.random.default_rng(11)
    X = np.sort(rng.integers(0, 60, (12, 24), dtype=np.uint32), axis=1)  # heavy repetition: multiset semantics
    Y = np.sort(rng.integers(0, 60, (17, 16), dtype=np.uint32), axis=1)
    Y[3] = 7  # one repeated hash
    assert (nbo.shared_matrix_ascending(X, Y) == nbo.shared_matrix(X, Y)).all()
    assert (nbo.shared_matrix_ascending(Y, X) == nbo.shared_matrix(Y, X)).all()
    X2 = np.sort(rng.integers(0, 1 << 30, (5, 16), dtype=np.uint32), axis=1)
    Y2 = np.sort(rng.integers(0, 1 << 30, (9, 16), dtype=np.uint32), axis=1)
    Y2[4, :9] = X2[2, :9]
    Y2[4].sort()
    assert (nbo.shared_matrix_ascending(X2, Y2) == nbo.shared_matrix(X2, Y2)).all()


def test_oracle_irregular_sketches():
    """not ascending, one repeated hash, a stale in-place Sketches: the merge's own answer, receiver = the row"""
    a = np.array([5, 9, 12, 20, 31, 40], np.uint32)
    unsorted = np.array([40, 5, 31, 9, 20, 12], np.uint32)
    repeated = np.full(6, 20, np.uint32)
    stale = np.array([5, 9, 12, 0, 0, 0], np.uint32)  # a short sequence's sketch over mash.New's zeros
    S = np.stack([a, unsorted, repeated, stale])
    M = nbo.shared_matrix(S, S)
    assert M[0, 0] == 6 and M[0, 2] == 1 and M[2, 2] == 6
    # the merge reads an unsorted sketch as it stands: not symmetric, not the set intersection
    assert M[0, 1] == orc.mash_shared(a, unsorted) and M[1, 0] == orc.mash_shared(unsorted, a)
    assert M[0, 3] == orc.mash_shared(a, stale)
    first, cols, shared, dist = nbo.neighbors(S, S, 1, 0, True, 0)
    for i in range(4):
        want = [(j, int(M[i, j])) for j in range(4) if j != i and M[i, j] >= 1]
        assert list(zip(cols[first[i]:first[i + 1]].tolist(), shared[first[i]:first[i + 1]].tolist())) == want
