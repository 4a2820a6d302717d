"""polyhip_primer_dimer_matrix and polyhip_primer_dimer_screen on the device: every output compared exactly with the plain-Python
oracle (tests/dimers_oracle.py) on the inputs of tests/dimers_inputs.py -- the hand answers, every pair of lengths around 32 and
64, sizes of X and Y around the wave, the block and the chunk, bad primers, odd bytes, duplicates, rows without a partner, pool
mode, single planes, random pools, a Y larger than any internal tile, repeatability and the counters."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import dimers_inputs as di  # noqa: E402
import dimers_oracle as do  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = do.NONE
ANY_T, END_T = -6000, -4000


def _same_screen(got, want):
    for f in do.SCREEN_FIELDS + ("errX", "errY"):
        g = getattr(got, f)
        assert g.dtype == want[f].dtype and g.tolist() == want[f].tolist(), f


def _check(X, Y, any_t=ANY_T, end_t=END_T, table=None):
    """the matrix and the screen of (X, Y) against the oracle, and the screen against the reduction of the matrix"""
    from poly_amd import dimers
    kw = {} if table is None else {"table": table}
    want_any, want_end, errX, errY = do.matrix(X, Y, table)
    m = dimers.matrix(X, Y, **kw)
    assert m.dg_any.dtype == m.dg_end.dtype == np.int32
    assert (m.dg_any == want_any).all() and (m.dg_end == want_end).all()
    assert m.errX.tolist() == errX.tolist() and m.errY.tolist() == errY.tolist()
    s = dimers.screen(X, Y, any_threshold=any_t, end_threshold=end_t, **kw)
    _same_screen(s, do.screen(X, Y, any_t, end_t, table))
    red = do.screen_from_matrix(m.dg_any, m.dg_end, m.errX, m.errY, any_t, end_t)
    for f, v in red.items():
        assert getattr(s, f).tolist() == v.tolist(), f
    return m, s


def test_hand_answers():
    from poly_amd import dimers
    for x, y, want_any, want_end in di.hand():
        s = dimers.screen([x], [y], any_threshold=0, end_threshold=0)
        got_any = (int(s.any_dg[0]), int(s.any_shift[0]), int(s.any_pos[0]), int(s.any_pairs[0]))
        got_end = (int(s.end_dg[0]), int(s.end_shift[0]), int(s.end_pairs[0]))
        assert got_any == want_any and got_end == want_end, (x, y, got_any, got_end)
        assert s.any_partner[0] == (0 if want_any[0] else NONE) and s.end_partner[0] == (0 if want_end[0] else NONE)
        assert s.any_count[0] == 1 and s.end_count[0] == 1                 # a threshold of 0 counts every valid y
        m = dimers.matrix([x], [y])
        assert (int(m.dg_any[0, 0]), int(m.dg_end[0, 0])) == (want_any[0], want_end[0])
    X, Y = [h[0] for h in di.hand()], [h[1] for h in di.hand()]
    _check(X, Y)


@pytest.mark.parametrize("m", di.GRID)
def test_every_pair_of_lengths(m):
    """x of m bytes against y of every length of the grid, three pairs each: bit 63, both halves of the masks, shifts to +-62"""
    from poly_amd import dimers
    for n in di.GRID:
        for x, y in di.grid_pairs(m, n):
            want = do.screen([x], [y], 0, 0)
            _same_screen(dimers.screen([x], [y], any_threshold=0, end_threshold=0), want)
            p = do.pair(x, y)
            mt = dimers.matrix([x], [y])
            assert (int(mt.dg_any[0, 0]), int(mt.dg_end[0, 0])) == (p.dg_any, p.dg_end), (m, n)
            # ... and from y's side
            _same_screen(dimers.screen([y], [x], any_threshold=0, end_threshold=0), do.screen([y], [x], 0, 0))


@functools.lru_cache(maxsize=None)
def _sized_reference():
    X, Y = di.sized_pool()
    return X, Y, do.matrix(X, Y)


@pytest.mark.parametrize("nx", di.SIZED_NX)
@pytest.mark.parametrize("ny", di.SIZED_NY)
def test_sizes_of_x_and_y(nx, ny):
    """prefixes of one pool, one oracle plane for all of them; the screen's partner and counts are the plane's reduction (which
    tests/test_dimers_cpu.py and the other tests here hold to the oracle's own screen), its shift, pos and pairs the oracle's pair"""
    from poly_amd import dimers
    X, Y, (want_any, want_end, _, _) = _sized_reference()
    X, Y = X[:nx], Y[:ny]
    m = dimers.matrix(X, Y)
    assert (m.dg_any == want_any[:nx, :ny]).all() and (m.dg_end == want_end[:nx, :ny]).all()
    s = dimers.screen(X, Y, any_threshold=-3000, end_threshold=-2500)
    red = do.screen_from_matrix(want_any[:nx, :ny], want_end[:nx, :ny], np.zeros(nx), np.zeros(ny), -3000, -2500)
    for f, v in red.items():
        assert getattr(s, f).tolist() == v.tolist(), f
    for i in range(nx):
        p = do.pair(X[i], Y[s.any_partner[i]]) if s.any_partner[i] != NONE else do.Pair()
        assert (s.any_shift[i], s.any_pos[i], s.any_pairs[i]) == (p.any_shift, p.any_pos, p.any_pairs)
        p = do.pair(X[i], Y[s.end_partner[i]]) if s.end_partner[i] != NONE else do.Pair()
        assert (s.end_shift[i], s.end_pairs[i]) == (p.end_shift, p.end_pairs)


def test_bad_primers_on_both_sides():
    X, Y = di.bad_lengths()
    m, s = _check(X, Y)
    assert s.errX.tolist() == [0, 1, 0, 2, 2, 0] and s.errY.tolist() == [2, 0, 1, 0, 2]
    assert not m.dg_any[[1, 3, 4]].any() and not m.dg_any[:, [0, 2, 4]].any()
    _check(Y, X)
    _check(X, None)                                                       # the bad ones among their own partners
    _check([b"", b"A" * 65], [b"", b"C" * 200])                            # nothing valid at all


def test_odd_bytes_and_lower_case():
    X, Y = di.odd_bytes()
    m, _ = _check(X, Y)
    assert (m.dg_any[0] == m.dg_any[4]).all() and m.dg_any[0, 0] == m.dg_any[0, 1] == -16398
    _check(Y, X)


def test_duplicates_go_to_the_lowest_index():
    X, Y = di.duplicates()
    _, s = _check(X, Y)
    assert s.any_partner.tolist() == [1, 2] and s.end_partner.tolist() == [1, 2]
    # ... also when the copies sit in different waves, blocks and chunks: 3,000 copies of the two partners behind fillers
    wide = [b"ACACACAC"] * 70 + [Y[2], Y[1]] * 1500
    s = _check(X, wide)[1]
    assert s.any_partner.tolist() == [71, 70] and s.any_count.tolist() == [1500, 1500]


def test_rows_without_a_partner():
    X, Y = di.no_partner()
    _, s = _check(X, Y, 0, 0)
    assert s.any_partner.tolist()[:2] == [NONE, NONE] and s.any_dg.tolist()[:2] == [0, 0] and s.any_partner[2] == 0
    assert s.any_shift.tolist()[:2] == s.any_pos.tolist()[:2] == s.any_pairs.tolist()[:2] == [0, 0]
    # a table with zeros: a run of two pairs without energy is no partner either
    _, s = _check([b"GG", b"GGCC"], [b"CC", b"GGCC"], 0, 0, table=[0] * 16)
    assert s.any_partner.tolist() == [NONE, NONE] and s.any_count.tolist() == [2, 2]


def test_pool_mode_is_x_against_x():
    from poly_amd import dimers
    X, _ = di.bad_lengths()
    pool = X + di.random_pool()[:30]
    a, b = dimers.matrix(pool), dimers.matrix(pool, pool)
    assert (a.dg_any == b.dg_any).all() and (a.dg_end == b.dg_end).all() and a.errX.tolist() == b.errX.tolist() == b.errY.tolist()
    sa, sb = dimers.screen(pool, any_threshold=ANY_T, end_threshold=END_T), dimers.screen(pool, pool, any_threshold=ANY_T, end_threshold=END_T)
    for f in do.SCREEN_FIELDS + ("errX", "errY"):
        assert getattr(sa, f).tolist() == getattr(sb, f).tolist(), f
    assert (a.dg_any == a.dg_any.T).all()                                  # dg_any(x, y) == dg_any(y, x)


def test_one_plane_at_a_time():
    from poly_amd import dimers
    pool = di.random_pool()[:40]
    both = dimers.matrix(pool)
    only_any, only_end = dimers.matrix(pool, want_end=False), dimers.matrix(pool, want_any=False)
    assert only_any.dg_end is None and only_end.dg_any is None
    assert (only_any.dg_any == both.dg_any).all() and (only_end.dg_end == both.dg_end).all()


def test_random_pool_of_18_to_30_mers():
    """100 x 100 ordered pairs, both thresholds where some pairs pass and some do not"""
    pool = di.random_pool()
    m, s = _check(pool, None, -4500, -3000)
    assert 0 < int(s.any_count.sum()) < 10_000 and 0 < int(s.end_count.sum()) < 10_000 and (s.any_partner != NONE).all()
    _check(pool[:20], pool[50:], -30000 * 63, 0)                           # the loosest and the tightest threshold there is


def test_y_larger_than_any_tile():
    """ny = 70,000, nx = 3: the screen against the numpy reduction of the matrix call, and all three rows against the oracle"""
    from poly_amd import dimers
    X, Y = di.wide()
    m = dimers.matrix(X, Y)
    s = dimers.screen(X, Y, any_threshold=-2500, end_threshold=-1500)
    red = do.screen_from_matrix(m.dg_any, m.dg_end, m.errX, m.errY, -2500, -1500)
    for f, v in red.items():
        assert getattr(s, f).tolist() == v.tolist(), f
    _same_screen(s, do.screen(X, Y, -2500, -1500))
    assert int(s.any_count.min()) > 1024 and len(set((s.any_partner // 1024).tolist())) > 1


@functools.lru_cache(maxsize=None)
def _pool_reference():
    pool = di.random_pool()
    return pool, do.screen(pool, None, -4500, -3000)


@pytest.mark.parametrize("launch_pairs", (1, 250, 1000, 3333))
def test_row_blocks_do_not_show(monkeypatch, launch_pairs):
    """the screen cuts X into row blocks of about 2^32 pairs, one launch each; POLYHIP_DIMER_LAUNCH_PAIRS brings that down to sizes
    at which 100 rows against 100 y take 100, 50, 10 and 4 launches (the last block shorter than the others): every output is the
    oracle's, and so the one launch's"""
    from poly_amd import dimers
    pool, want = _pool_reference()
    monkeypatch.delenv("POLYHIP_DIMER_LAUNCH_PAIRS", raising=False)
    one = dimers.screen(pool, any_threshold=-4500, end_threshold=-3000)
    assert dimers.last_info()["launches"] == 3
    monkeypatch.setenv("POLYHIP_DIMER_LAUNCH_PAIRS", str(launch_pairs))
    cut = dimers.screen(pool, any_threshold=-4500, end_threshold=-3000)
    rows = max(1, launch_pairs // 100)
    assert dimers.last_info()["launches"] == 2 + -(-100 // rows)
    _same_screen(cut, want)
    for f in do.SCREEN_FIELDS:
        assert getattr(cut, f).tobytes() == getattr(one, f).tobytes(), f
    # ... with bad primers among the rows and a Y of its own
    X, Y = di.bad_lengths()
    monkeypatch.setenv("POLYHIP_DIMER_LAUNCH_PAIRS", "7")
    _same_screen(dimers.screen(X, Y), do.screen(X, Y))
    assert dimers.last_info()["launches"] == 3 + 6


def test_the_same_call_gives_the_same_bytes():
    from poly_amd import dimers
    X, Y = di.wide()
    pool = di.random_pool()
    a, b = dimers.screen(X, Y, any_threshold=-2500, end_threshold=-1500), dimers.screen(X, Y, any_threshold=-2500, end_threshold=-1500)
    c, d = dimers.screen(pool), dimers.screen(pool)
    for f in do.SCREEN_FIELDS + ("errX", "errY"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes() and getattr(c, f).tobytes() == getattr(d, f).tobytes(), f
    m1, m2 = dimers.matrix(pool), dimers.matrix(pool)
    assert m1.dg_any.tobytes() == m2.dg_any.tobytes() and m1.dg_end.tobytes() == m2.dg_end.tobytes()


def test_last_info():
    from poly_amd import dimers
    X, Y = di.bad_lengths()
    dimers.matrix(X, Y)
    assert dimers.last_info() == do.info(X, Y, launches=3)                 # two prepares, one pair kernel
    dimers.screen(X, Y)
    assert dimers.last_info() == do.info(X, Y, launches=4)                 # ... and the details
    dimers.screen(X)
    assert dimers.last_info() == do.info(X, None, launches=3)
    pool = di.random_pool()
    dimers.matrix(pool)
    info = dimers.last_info()
    assert info == do.info(pool, None, launches=2) and info["pairs"] == 10_000 and info["bad"] == 0 and info["primers"] == 100
    dimers.matrix([])                                                      # an empty call resets the counters
    assert dimers.last_info() == dict.fromkeys(do.INFO_FIELDS, 0)
