"""The closest approach of listed pairs on the device (csrc/conjunction.hip: pairs_kernel, one wave per pair) against the two
screens: with a threshold of 1e12 m a screen lists every pair that has a valid interval, and screen_pairs on that list must
return the screen's distance and time BIT FOR BIT -- the same source expressions per interval, and a minimum under the total order
(squared distance, interval) whichever lane an interval went to.  The screens themselves are held to the numpy restatement in
test_conjunction_gpu.py and test_conjunction_cross_gpu.py, so no tolerance appears here.

Grids: a lane takes the intervals l, l + 64, ...: M = 2 is one interval, 17 fewer intervals than lanes, 65 exactly 64, 66 one lane
with two, 130 lanes with three and lanes with two.  Ragged: spans that end or begin inside the grid (ends that are NaN, pairs
without a common interval) and one satellite with a single node (its ephemeris is NaN throughout, status 9)."""
import numpy as np
import pytest

import conjunction_reference as R
import conjunction_cross_reference as X

pytestmark = pytest.mark.gpu

GRIDS = [2, 17, 65, 66, 130]
ALL = 1e12                                                           # metres: every pair with a valid interval is listed
S6 = np.array([(i, j) for i in range(6) for j in range(i + 1, 6)], dtype=np.float64)
S6X9 = np.array([(i, j) for i in range(6) for j in range(9)], dtype=np.float64)


def rows(ij):
    """(n, 2) index pairs -> an (n, 4) list whose last two columns must not be read"""
    return np.column_stack([ij, np.full((len(ij), 2), -7.0)])


def same_bits(out, status, listed, ij, swapped=False):
    """out / status for the pairs ij: the rows the screen listed carry its bytes, the others (+inf, NaN); every status OK.
    swapped: ij are the (j, i) of the all-pairs form, which the screen lists as (i, j)"""
    want = {(int(i), int(j)): (d, t) for i, j, d, t in listed}
    assert np.array_equal(out[:, :2], ij) and (status == 0).all()
    for (i, j), (d, t) in zip(ij.astype(int).tolist(), out[:, 2:]):
        key = (j, i) if swapped else (i, j)
        if key in want:
            assert np.array([d, t]).tobytes() == np.array(want[key]).tobytes(), (i, j, d, t, want[key])
        else:
            assert np.isposinf(d) and np.isnan(t), (i, j, d, t)


@pytest.mark.parametrize("M", GRIDS)
def test_all_pairs_form_has_the_screens_bits(M):
    from mpconstellation_amd import screen, screen_pairs
    c = R.case(6, M)
    grid = (c["T0"], c["T1"])
    r = screen(c["eph"], *grid, threshold=ALL)
    assert len(r.pairs) == 15
    out, status = screen_pairs(r, *grid, eph=c["eph"])
    assert out.tobytes() == r.pairs.tobytes() and status.tolist() == [0] * 15
    perm = np.random.default_rng(M).permutation(15)                  # list order, whatever it is
    out, status = screen_pairs(r.pairs[perm], *grid, eph=c["eph"])
    assert out.tobytes() == r.pairs[perm].tobytes()
    swapped = r.pairs[:, [1, 0, 2, 3]]                               # (j, i): the same operations on the same operands
    out, status = screen_pairs(swapped, *grid, eph=c["eph"])
    assert out.tobytes() == np.ascontiguousarray(swapped).tobytes() and (status == 0).all()
    traj = dict(Y=c["Y"], units=c["units"], span=c["span"], M=M)
    rt = screen(T0=c["T0"], T1=c["T1"], threshold=ALL, **traj)
    out, status, eph_status, cat_status = screen_pairs(rt, *grid, **traj)
    assert len(rt.pairs) == 15 and out.tobytes() == rt.pairs.tobytes()
    assert eph_status.tolist() == [0] * 6 and cat_status is None and (status == 0).all()
    out, status = screen_pairs(r, *grid, eph=c["eph"], devices=[0, 0])
    assert out.tobytes() == r.pairs.tobytes() and (status == 0).all()
    out, status, eph_status, cat_status = screen_pairs(rt, *grid, devices=[0, 0], **traj)
    assert out.tobytes() == rt.pairs.tobytes() and (eph_status == 0).all() and cat_status is None


@pytest.mark.parametrize("M", GRIDS)
def test_catalogue_form_has_the_screens_bits(M):
    from mpconstellation_amd import screen_against, screen_pairs
    c = X.case(6, 9, M)
    grid = (c["T0"], c["T1"])
    r = screen_against(c["eph"], c["cat_eph"], *grid, threshold=ALL)
    assert len(r.pairs) == 54
    out, status = screen_pairs(r, *grid, eph=c["eph"], cat_eph=c["cat_eph"])
    assert out.tobytes() == r.pairs.tobytes() and status.tolist() == [0] * 54
    perm = np.random.default_rng(M).permutation(54)
    out, status = screen_pairs(r.pairs[perm], *grid, eph=c["eph"], cat_eph=c["cat_eph"], devices=[0, 0])
    assert out.tobytes() == r.pairs[perm].tobytes() and (status == 0).all()
    traj = dict(M=M, **c["sat"], **c["cat"])
    rt = screen_against(T0=c["T0"], T1=c["T1"], threshold=ALL, **traj)
    out, status, eph_status, cat_status = screen_pairs(rt, *grid, **traj)
    assert len(rt.pairs) == 54 and out.tobytes() == rt.pairs.tobytes() and (status == 0).all()
    assert eph_status.tolist() == [0] * 6 and cat_status.tolist() == [0] * 9
    out, status, eph_status, cat_status = screen_pairs(rt, *grid, devices=[0, 0], **traj)
    assert out.tobytes() == rt.pairs.tobytes() and (eph_status == 0).all() and (cat_status == 0).all()


def ragged(M):
    """6 satellites and 9 objects with n = 40 nodes: spans that end or begin inside the grid, two that never meet, a satellite and an
    object with a single node in use, and node counts below n with garbage behind them"""
    orb = R.random_orbits(15, seed=31 + M)
    T0, T1 = 0.0, 2 * np.pi / R.orbit_rate(orb).max()
    span = np.tile([T0 - 1.0, T1 + 1.0], (15, 1))
    span[1] = (T0 - 1.0, 0.4 * T1)
    span[2] = (0.6 * T1, T1 + 1.0)                                   # never on the grid together with satellite 1
    span[4] = (0.3 * T1, 0.7 * T1)
    span[6 + 2] = (T0 - 1.0, 0.35 * T1)
    span[6 + 5] = (0.65 * T1, T1 + 1.0)
    span[6 + 7] = (T1 + 10.0, T1 + 500.0)                            # an object that is never on the grid
    Y, units, span = R.trajectories(orb, 40, span)
    ns = np.full(15, 40, dtype=np.int32)
    ns[3] = 1; ns[6 + 4] = 1                                         # a single node: no ephemeris, status 9
    ns[5] = 23; ns[6 + 1] = 31
    for s in (5, 6 + 1):                                             # the trajectory on its own count, garbage past it
        Yk, _, _ = R.trajectories({k: v[s:s + 1] for k, v in orb.items()}, int(ns[s]), span[s])
        Y[s] = 1e300; Y[s, :, :ns[s]] = Yk[0]
    sat = dict(Y=Y[:6], units=units[:6], span=span[:6], ns=ns[:6])
    cat = dict(cat_Y=Y[6:], cat_units=units[6:], cat_span=span[6:], cat_ns=ns[6:])
    return sat, cat, T0, T1


@pytest.mark.parametrize("M", GRIDS)
def test_ragged_spans_and_counts(M):
    from mpconstellation_amd import common_clock, screen, screen_against, screen_pairs
    sat, cat, T0, T1 = ragged(M)
    r = screen(T0=T0, T1=T1, threshold=ALL, M=M, **sat)
    out, status, eph_status, cat_status = screen_pairs(rows(S6), T0, T1, M=M, **sat)
    assert eph_status.tolist() == [0, 0, 0, 9, 0, 0] == r.status.tolist() and cat_status is None
    same_bits(out, status, r.pairs, S6)
    listed = {(int(i), int(j)) for i, j in r.pairs[:, :2]}
    assert (1, 2) not in listed and not any(3 in p for p in listed)
    if M >= 17:
        assert (0, 5) in listed and (0, 4) in listed and len(listed) >= 8
    out, status, _, _ = screen_pairs(rows(S6[:, ::-1]), T0, T1, M=M, **sat)
    same_bits(out, status, r.pairs, np.ascontiguousarray(S6[:, ::-1]), swapped=True)
    eph, st = common_clock(sat["Y"], sat["units"], sat["span"], M, T0, T1, ns=sat["ns"], return_status=True)
    assert st.tolist() == [0, 0, 0, 9, 0, 0] and np.isnan(eph[3]).all()
    out2, status2 = screen_pairs(rows(S6), T0, T1, eph=eph)
    same_bits(out2, status2, r.pairs, S6)
    # against the catalogue
    rx = screen_against(T0=T0, T1=T1, threshold=ALL, M=M, **sat, **cat)
    out, status, eph_status, cat_status = screen_pairs(rows(S6X9), T0, T1, M=M, **sat, **cat)
    assert eph_status.tolist() == rx.status.tolist() and cat_status.tolist() == rx.cat_status.tolist() == [0, 0, 0, 0, 9, 0, 0, 0, 0]
    same_bits(out, status, rx.pairs, S6X9)
    listed = {(int(i), int(j)) for i, j in rx.pairs[:, :2]}
    assert not any(i == 3 or j in (4, 7) for i, j in listed) and (1, 5) not in listed and (2, 2) not in listed
    if M >= 17:
        assert (0, 0) in listed and (0, 1) in listed and (5, 0) in listed and len(listed) >= 25
    out, status, _, _ = screen_pairs(rows(S6X9), T0, T1, M=M, devices=[0, 0, 0], **sat, **cat)
    same_bits(out, status, rx.pairs, S6X9)


def test_a_velocity_that_is_nan_alone_voids_the_end():
    """the screens read their ends behind the transpose kernel, which makes an end with a NaN in any of its six values NaN in all
    six; the list kernel reads the ephemeris itself and must apply the same rule"""
    from mpconstellation_amd import screen, screen_against, screen_pairs
    c = X.case(6, 9, 66)
    eph, cat = c["eph"].copy(), c["cat_eph"].copy()
    eph[2, 4, 10:30] = np.nan
    eph[4, 0, 64] = np.nan
    cat[3, 5, 0] = np.nan
    grid = (c["T0"], c["T1"])
    r = screen(eph, *grid, threshold=ALL)
    out, status = screen_pairs(r, *grid, eph=eph)
    assert len(r.pairs) == 15 and out.tobytes() == r.pairs.tobytes()
    rx = screen_against(eph, cat, *grid, threshold=ALL)
    out, status = screen_pairs(rx, *grid, eph=eph, cat_eph=cat)
    assert len(rx.pairs) == 54 and out.tobytes() == rx.pairs.tobytes()
    clean = screen_against(c["eph"], c["cat_eph"], *grid, threshold=ALL)
    assert rx.pairs.tobytes() != clean.pairs.tobytes()               # (the voided ends did hold some pair's minimum)


def test_bad_rows_are_reported_and_leave_their_neighbours_alone():
    from mpconstellation_amd import screen, screen_against, screen_pairs
    c = X.case(6, 9, 66)
    grid = (c["T0"], c["T1"])
    r = screen(c["eph"], *grid, threshold=ALL)
    want = {(int(i), int(j)): (d, t) for i, j, d, t in r.pairs}
    ij = np.array([(0, 1), (6, 1), (2, 2), (1, -1), (0.5, 1), (np.nan, 1), (1, np.inf), (3e9, 0), (3, 4)])
    out, status = screen_pairs(rows(ij), *grid, eph=c["eph"])
    assert status.tolist() == [0, 9, 9, 9, 9, 9, 9, 9, 0]
    assert np.isnan(out[1:8, 2:]).all() and np.array_equal(out[:, :2], ij, equal_nan=True)
    assert tuple(out[0, 2:]) == want[(0, 1)] and tuple(out[8, 2:]) == want[(3, 4)]
    rx = screen_against(c["eph"], c["cat_eph"], *grid, threshold=ALL)
    want = {(int(i), int(j)): (d, t) for i, j, d, t in rx.pairs}
    ij = np.array([(5, 8), (0, 9), (6, 0), (2, 2), (-1, 3), (0, 6)])
    out, status = screen_pairs(rows(ij), *grid, eph=c["eph"], cat_eph=c["cat_eph"])
    assert status.tolist() == [0, 9, 9, 0, 9, 0] and np.isnan(out[[1, 2, 4], 2:]).all()
    for k in (0, 3, 5):                                              # (against a catalogue i == j is a pair like any other)
        assert tuple(out[k, 2:]) == want[tuple(ij[k].astype(int))]


def test_c_abi_refuses_bad_arguments():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    eph = np.zeros((2, 6, 4)); cat = np.zeros((3, 6, 4)); pairs = np.zeros((2, 4)); pairs[:, 1] = 1
    out = np.zeros((2, 4)); st = np.zeros(2, dtype=np.int32)
    good = dict(n=2, S=2, D=3, M=4, T0=0.0, T1=1.0)

    def call(a, cat=cat, out=out):
        return lib.mpcx_conjunction_pairs(ctx, a["n"], _ffi.dptr(pairs), a["S"], a["D"], a["M"], _ffi.dptr(eph), _ffi.dptr_opt(cat), a["T0"], a["T1"],
                                          _ffi.dptr_opt(out), _ffi.iptr(st))
    assert call(good) == 0 and st.tolist() == [0, 0] and out[:, 2].tolist() == [0.0, 0.0]         # (all zeros: distance 0)
    assert call({**good, "D": 0}, cat=None) == 0 and st.tolist() == [0, 0]
    for bad in (dict(n=0), dict(S=0), dict(D=-1), dict(M=1), dict(T1=0.0), dict(T1=-1.0)):
        assert call({**good, **bad}) == -2, bad
        assert b"conjunction_pairs" in lib.mpcx_last_error(ctx)
    assert call(good, cat=None) == -2 and call({**good, "D": 0}) == -2 and call(good, out=None) == -2
    Y = np.zeros((2, 7, 5)); u = np.ones((2, 2)); sp = np.array([[0.0, 1.0]] * 2)
    for n, S, D, M, T1, nn in ((0, 2, 0, 4, 1.0, 5), (2, 0, 0, 4, 1.0, 5), (2, 2, 0, 1, 1.0, 5), (2, 2, 0, 4, 0.0, 5), (2, 2, 0, 4, 1.0, 0), (2, 2, 3, 4, 1.0, 5)):
        rc = lib.mpcx_conjunction_pairs_traj(ctx, n, _ffi.dptr(pairs), S, nn, None, _ffi.dptr(Y), _ffi.dptr(u), _ffi.dptr(sp), D, 0, None, None, None,
                                             None, M, 0.0, T1, _ffi.dptr(out), _ffi.iptr(st), None, None)
        assert rc == -2, (n, S, D, M, T1, nn)
    w = lib.mpcx_conjunction_pairs_workspace_bytes
    assert w(0, 0, 4) == 0 and w(2, -1, 4) == 0 and w(2, 3, 1) == 0 and w(2, 3, 4) > w(2, 0, 4) >= 2 * 6 * 4 * 8
