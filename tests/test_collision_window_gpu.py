"""The window collision probability on the device (csrc/collision_window.hip) against its numpy restatement
(collision_window_reference.py), through the screen and the short-encounter call for a planted fast encounter, for a planted slow
pair, and at its edges.

Tolerance against the restatement, from the arithmetic (collision_window_reference.rounding_bound): positions of 7e6 m through the
Hermite's few operations differ by about 2e-7 m, which moves the density by its logarithmic slope; the exponent is formed through the
Cholesky factor of a covariance that is two six-term products, so its rounding grows with cond(A) and with the largest exponent that
still counts.  test_collision_window_host.py checks on the CPU that the bound stays below 1e-6 on every row of the scenes and that
the restatement's own fp64 sensitivity is inside it."""
import numpy as np
import pytest

import collision_reference as C
import collision_window_reference as W

pytestmark = pytest.mark.gpu


def result_bits(r):
    return tuple(np.ascontiguousarray(x).tobytes() for x in (r.p, r.start, r.entries, r.rate_max, r.t_rate_max, r.window, r.status))


def assert_close_to_restated(res, out, status, bound, what):
    assert np.array_equal(res.status, status) and (status == 0).all()
    assert (bound <= 1e-6).all()
    p, start, entries, rmax, tmax, ta, tb = out.T
    print(f"{what}: worst |dp| / bound {np.max(np.abs(res.p - p) / (bound * p)):.3f}, largest bound {bound.max():.2e}")
    assert (np.abs(res.p - p) <= bound * p).all()
    assert (np.abs(res.start - start) <= bound * start).all() and (np.abs(res.entries - entries) <= bound * p).all()
    assert (np.abs(res.rate_max - rmax) <= bound * rmax).all()
    assert np.array_equal(res.window[:, 0], ta) and np.array_equal(res.window[:, 1], tb)
    same_node = np.abs(res.t_rate_max - tmax) <= 1e-9 * (tb - ta)           # (two nodes whose rates differ by less than the bound may swap)
    assert same_node.mean() >= 0.9 and (res.t_rate_max >= ta).all() and (res.t_rate_max <= tb).all()


@pytest.mark.parametrize("panels", W.SCENE_PANELS)
@pytest.mark.parametrize("K", W.SCENE_KS)
@pytest.mark.parametrize("n", [1, 63, 65])
def test_window_probability_against_the_restatement(n, K, panels):
    """catalogue form and all-pairs form of the first n rows of collision_window_reference.window_scene(K): km/s crossings and pairs
    below 1 m/s, one without any relative motion; ragged node counts; windows cut by the spans where K is small"""
    from mpconstellation_amd import collision_probability_window
    sc = W.window_scene(K)
    out, status, bound = (x[:n] for x in sc["ref"][panels])
    Y, units, span, P, radius, _ = sc["rows"]
    res = collision_probability_window(sc["pairs"][:n], radius, Y, units, span, P, sc["half"][:n], panels=panels, cat=sc["cat"])
    assert np.array_equal(res.pairs, sc["pairs"][:n])
    assert_close_to_restated(res, out, status, bound, f"n {n} K {K} panels {panels} catalogue")
    (uY, uunits, uspan, uP, uradius, uns), upairs = C.union_of(sc)
    res = collision_probability_window(upairs[:n], uradius, uY, uunits, uspan, uP, sc["half"][:n], panels=panels, ns=uns)
    assert_close_to_restated(res, out, status, bound, f"n {n} K {K} panels {panels} all-pairs")


def test_both_forms_and_two_contexts_give_the_same_bits():
    from mpconstellation_amd import collision_probability_window
    sc = W.window_scene(30)
    Y, units, span, P, radius, _ = sc["rows"]
    a = collision_probability_window(sc["pairs"], radius, Y, units, span, P, sc["half"], panels=3, cat=sc["cat"])
    (uY, uunits, uspan, uP, uradius, uns), upairs = C.union_of(sc)
    b = collision_probability_window(upairs, uradius, uY, uunits, uspan, uP, sc["half"], panels=3, ns=uns)
    c = collision_probability_window(sc["pairs"], radius, Y, units, span, P, sc["half"], panels=3, cat=sc["cat"], devices=[0, 0])
    assert (a.status == 0).all() and result_bits(a) == result_bits(b) == result_bits(c)


def planted_fast():
    """test_collision_gpu.py's planted encounter: circular orbits of radii R0 and R0 + 300 m, planes 1.2 rad apart, crossing at
    t_c = 1000 s, a node of both (101 nodes over 2000 s); isotropic position covariances of 200 m each, no velocity uncertainty"""
    R0, m, sig = 7.0e6, 300.0, 200.0
    tc, n, span = 1000.0, 101, (0.0, 2000.0)
    u = np.array([1.0, 0.0, 0.0])
    ya, ua = C.circular_through(R0 * u, np.array([0.0, 1.0, 0.0]), tc, n, span)
    yb, ub = C.circular_through((R0 + m) * u, np.array([0.0, np.cos(1.2), np.sin(1.2)]), tc, n, span)
    P = np.zeros((2, n, 6, 6)); P[:, :, 0, 0] = P[:, :, 1, 1] = P[:, :, 2, 2] = sig * sig
    return np.stack([ya, yb]), np.stack([ua, ub]), np.array([span, span]), P, np.array([8.0, 12.0])


def test_planted_fast_encounter_agrees_with_the_short_encounter_model():
    """screen -> collision_probability -> encounter_half_window -> collision_probability_window(panels=4) on test_collision_gpu.py's
    planted crossing (8 km/s, miss 300 m, combined sigma 283 m, R = 20 m, half window 0.268 s).  The two MODELS differ there, and by
    how much depends on where the screen puts the row's time t: the short-encounter model freezes the geometry and the covariance at
    t, the window follows both through +-0.268 s about it.  Evaluated with the restatements on the CPU when written
    (collision_window_reference against collision_reference on the row (0, 1, ., t)): relative difference 6.4e-10 at t = t_c -- where
    the screen puts it (profiles/collision_probability.txt) --, 5.7e-9 at t_c +- 0.05 s, 1.9e-7 at t_c +- 0.1 s, the residual the
    screen is held to here and in test_collision_gpu.py.  Asserted: 10 x the restatements' difference on the screen's own row (6.4e-9
    at t_c, at most 1.9e-6) plus the rounding bound of the device against its restatement (collision_window_reference.
    rounding_bound: 3e-9 here) -- far below the cap of 1e-4 that no unit or factor error passes."""
    from mpconstellation_amd import screen, collision_probability, collision_probability_window, encounter_half_window
    Y, units, spans, P, radius = planted_fast()
    scr = screen(Y=Y, units=units, span=spans, M=401, T0=0.0, T1=2000.0, threshold=1000.0)
    assert scr.pairs[:, :2].tolist() == [[0.0, 1.0]] and abs(scr.pairs[0, 3] - 1000.0) < 0.1
    col = collision_probability(scr, radius, Y, units, spans, P)
    h = encounter_half_window(col, radius.sum())
    win = collision_probability_window(scr, radius, Y, units, spans, P, h, panels=4)
    side = (Y, units, spans, P, radius, None)
    rounding = np.empty(1)
    ref_w, st_w = W.collision_probability_window(scr.pairs, side, h, 4, bounds=rounding)
    ref_c, st_c = C.collision_probability(scr.pairs, side)
    models = abs(ref_w[0, W.PW_P] - ref_c[0, 0]) / ref_c[0, 0]
    tol = 10.0 * models + rounding[0]
    print(f"tca - t_c {scr.pairs[0, 3] - 1000.0:.2e} s, half window {h[0]:.4f} s, window p {win.p[0]:.12e}, short-encounter pc {col.pc[0]:.12e}, relative difference "
          f"{abs(win.p[0] - col.pc[0]) / col.pc[0]:.2e}; the restatements' {models:.2e}; tolerance {tol:.1e}")
    assert models <= 1.9e-7 and rounding[0] <= 1e-6 and tol <= 1e-4 and st_w.tolist() == [0] and st_c.tolist() == [0]
    assert win.status.tolist() == [0] and col.status.tolist() == [0] and 0.0 < col.pc[0] < 1.0
    assert abs(h[0] - (8.0 * col.sigma[0, 0] + 20.0) / col.speed[0]) <= 1e-15 * h[0]
    assert abs(win.p[0] - col.pc[0]) <= tol * col.pc[0]
    assert win.start[0] <= 1e-12 * win.p[0] and abs(win.t_rate_max[0] - scr.pairs[0, 3]) <= 0.1 * h[0]
    assert np.array_equal(win.window[0], [scr.pairs[0, 3] - h[0], scr.pairs[0, 3] + h[0]])


def planted_slow(lag_m=150.0, drift=2.0e-5):
    """Two objects on ONE circular orbit (61 nodes over 6000 s): the second lags the first by lag_m metres along the track at
    t = 3000 s and closes at drift x the orbital speed (its radius is smaller by 2/3 drift R0: 0.15 m/s).  Covariances from
    collision_reference.random_covariances (sigma 100 .. 400 m, 0.05 .. 0.3 m/s, correlated)."""
    R0, n, span, tc = 7.0e6, 61, (0.0, 6000.0), 3000.0
    u, v = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    ya, ua = C.circular_through(R0 * u, v, tc, n, span)
    Rb = R0 * (1.0 - 2.0 / 3.0 * drift)
    th = -lag_m / R0
    yb, ub = C.circular_through(Rb * (np.cos(th) * u + np.sin(th) * v), -np.sin(th) * u + np.cos(th) * v, tc, n, span)
    P = C.random_covariances(np.random.default_rng(9), 2, n)
    return np.stack([ya, yb]), np.stack([ua, ub]), np.array([span, span]), P, np.array([10.0, 15.0])


def test_planted_slow_pair_and_no_relative_speed():
    """a pair on one orbit with a small along-track drift, window +-600 s: status 0 and 0 < p < 1, equal to the restatement within its
    rounding bound.  The short-encounter call on the same row returns the model include/mpcx.h documents as not valid there; nothing
    is asserted of it.  A row of an object against a copy of itself (speed exactly 0) fails there (MPCX_ST_NUMERIC) and does not
    fail here."""
    from mpconstellation_amd import collision_probability, collision_probability_window
    Y, units, spans, P, radius = planted_slow()
    Y, units, spans, P, radius = (np.concatenate([x, x[:1]]) for x in (Y, units, spans, P, radius))       # object 2 = object 0
    pairs = np.array([[0.0, 1.0, 150.0, 3000.0], [0.0, 2.0, 0.0, 3000.0]])
    side = (Y, units, spans, P, radius, None)
    bound = np.empty(2)
    ref, st = W.collision_probability_window(pairs, side, 600.0, 4, bounds=bound)
    win = collision_probability_window(pairs, radius, Y, units, spans, P, 600.0, panels=4)
    col = collision_probability(pairs, radius, Y, units, spans, P)
    print(f"slow pair: speed {col.speed[0]:.3f} m/s, short-encounter pc {col.pc[0]:.3e}; window p {win.p} start {win.start} entries {win.entries}, "
          f"restated {ref[:, 0]}, bound {bound}")
    assert st.tolist() == [0, 0] and win.status.tolist() == [0, 0] and (bound <= 1e-6).all()
    assert (win.p > 0.0).all() and (win.p < 1.0).all() and (np.abs(win.p - ref[:, 0]) <= bound * ref[:, 0]).all()
    assert col.speed[0] < 1.0 and col.status.tolist() == [0, C.ST_NUMERIC]
    assert np.array_equal(win.window, [[2400.0, 3600.0]] * 2)


def test_per_row_failures_leave_the_neighbours_alone():
    """a bad index, t outside a span, an empty cut window (the row's time is where one span ends and the other begins), h = 0, h < 0,
    h = NaN, h = inf, a radius that is not finite, an indefinite covariance, R = 0 (zeros, status 0): each failing row NaN in every
    column with its status, the good rows bit for bit what they are in a list of their own, the statuses the restatement's"""
    from mpconstellation_amd import collision_probability_window
    sc = W.window_scene(30)
    (Y, units, span, P, radius, ns), pairs = C.union_of(sc)
    S = 5
    P, radius, span, half = P.copy(), radius.copy(), span.copy(), sc["half"][:22].copy()
    rows = pairs[:22].copy()
    P[S + 15] = -100.0 * P[S + 15]                                       # object 15: negative variances, larger than any satellite's
    radius[S + 17] = np.inf
    i19 = int(rows[19, 0])
    radius[S + 19] = -radius[i19]                                        # R = 0 exactly
    rows[1, 1] = len(Y)                                                  # no such object
    rows[3, 0] = -1.0
    rows[5, 3] = 1.0e6                                                   # outside both spans
    half[9], half[11], half[13], half[21] = 0.0, -5.0, np.nan, np.inf
    good = [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20]
    # row 7: object 7's span begins at the row's time, and the row's satellite is replaced by a copy of it whose span ends there
    t7, i7 = rows[7, 3], int(rows[7, 0])
    span[S + 7, 0] = t7
    Y, units, P, radius, ns = (np.concatenate([x, x[i7:i7 + 1]]) for x in (Y, units, P, radius, ns))
    span = np.concatenate([span, [[t7 - (span[i7, 1] - span[i7, 0]), t7]]])
    rows[7, 0] = len(Y) - 1
    side = (Y, units, span, P, radius, ns)
    res = collision_probability_window(rows, radius, Y, units, span, P, half, panels=3, ns=ns)
    ref, ref_status = W.collision_probability_window(rows, side, half, 3)
    B, N = C.ST_BADK, C.ST_NUMERIC
    assert ref_status.tolist() == [0, B, 0, B, 0, B, 0, B, 0, B, 0, B, 0, B, 0, N, 0, N, 0, 0, 0, B]
    assert np.array_equal(res.status, ref_status)
    bad = res.status != 0
    for a in (res.p, res.start, res.entries, res.rate_max, res.t_rate_max, res.window[:, 0], res.window[:, 1]):
        assert np.isnan(a[bad]).all() and np.isfinite(a[~bad]).all()
    assert (res.p[19], res.start[19], res.entries[19], res.rate_max[19]) == (0.0, 0.0, 0.0, 0.0) and res.window[19, 1] > res.window[19, 0]
    assert (res.p[good] > 0.0).all()
    alone = collision_probability_window(rows[good], radius, Y, units, span, P, half[good], panels=3, ns=ns)
    assert result_bits(alone) == tuple(np.ascontiguousarray(x[good]).tobytes() for x in
                                       (res.p, res.start, res.entries, res.rate_max, res.t_rate_max, res.window, res.status))


def test_c_abi_refuses_bad_sizes_and_panels():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    S, K, n = 2, 5, 3
    Y, units, span = np.zeros((S, 7, K)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S)
    P, radius, pairs, half = np.zeros((S, K, 6, 6)), np.ones(S), np.zeros((n, 4)), np.ones(n)
    out, pst = np.zeros((n, _ffi.NPW)), np.zeros(n, dtype=np.int32)
    d, i = _ffi.dptr, _ffi.iptr
    row = lambda S, K: (S, K, None, d(Y), d(units), d(span), d(P), d(radius))
    none = (0, 0, None, None, None, None, None, None)

    def pw(n=n, rows=None, cols=none, mu=C.MU_EARTH, half=d(half), panels=4):
        return lib.mpcx_collision_probability_window(ctx, n, d(pairs), *(rows or row(S, K)), *cols, mu, half, panels, d(out), i(pst))
    for bad in (dict(n=0), dict(rows=row(0, K)), dict(rows=row(S, 1)), dict(mu=0.0), dict(mu=-1.0), dict(cols=row(0, K)), dict(cols=row(S, 1)),
                dict(cols=(S, K, None, d(Y), d(units), d(span), None, d(radius))), dict(half=None), dict(panels=0), dict(panels=-3),
                dict(panels=_ffi.PW_MAX_PANELS + 1)):
        out[:] = 7.0
        assert pw(**bad) == -2, bad
        assert b"collision_probability_window" in lib.mpcx_last_error(ctx) and (out == 7.0).all()
    assert pw(panels=_ffi.PW_MAX_PANELS) == 0 and pw(panels=1) == 0
    assert (pst == C.ST_NUMERIC).all() and np.isnan(out).all()             # (all zeros: no covariance to factor)


def test_constellation_mpc_collision_probability_window():
    """test_collision_gpu.py's three-satellite plan with satellite 0 moved to pass 500 m from satellite 1: the method returns, bit for
    bit, collision_probability's two results and the module-level window call on the plan"""
    from mpconstellation_amd import Satellite, ConstellationMPC, conjunction as cj
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(3)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5)
    mpc.update()
    (w,) = mpc._screen_windows("plan", samples_per_node=4)
    X = mpc._plan[0]
    m = w["M"] // 3
    tb = w["T0"] + m * ((w["T1"] - w["T0"]) / (w["M"] - 1))
    side = (X, w["units"], w["span"], np.zeros((3, X.shape[2], 6, 6)), np.zeros(3), w["ns"])
    _, pa, va, _, _ = C.state_and_cov_at(side, 0, tb, C.MU_EARTH)
    _, pb, vb, _, _ = C.state_and_cov_at(side, 1, tb, C.MU_EARTH)
    e = np.cross(vb - va, [0.0, 0.0, 1.0]); e /= np.linalg.norm(e)
    X[0, 0:3, :] += ((pb - pa + 500.0 * e) / w["units"][0, 0])[:, None]
    P0 = np.diag([100.0 ** 2] * 3 + [0.1 ** 2] * 3)
    scr, col, win = mpc.collision_probability_window(1000.0, P0, 5.0, 60.0, panels=2, q=1e-8)
    print("planted pair:", scr.pairs, "pc", col.pc, "window p", win.p, "start", win.start, "entries", win.entries, "window", win.window)
    assert scr.pairs[:, :2].tolist() == [[0, 1]] and win.status.tolist() == [0] and 0.0 < win.p[0] < 1.0
    scr2, col2 = mpc.collision_probability(1000.0, P0, 5.0, q=1e-8)
    P = cj.covariance(X, w["units"], w["span"], mpc.consts, P0, U=mpc._plan[1], ns=w["ns"], q=1e-8)
    win2 = cj.collision_probability_window(scr2, 5.0, X, w["units"], w["span"], P, 60.0, panels=2, ns=w["ns"])
    assert scr.pairs.tobytes() == scr2.pairs.tobytes() and col.pc.tobytes() == col2.pc.tobytes() and result_bits(win) == result_bits(win2)
