"""The mathematics of avoidance for slow encounters (avoidance_window_reference.py, the restatement of include/mpcx.h:
mpcx_collision_window_sensitivity and mpcx_avoidance_window) without a GPU and independently of the kernels: the state gradient c_q
against central differences of collision_window_reference's own rate and ball term, the thrust gradient against central differences
of the window probability along arcs the CPU oracle propagates, the manoeuvre's contract, and the wrappers' argument checks.  The
measured figures quoted below are in profiles/avoidance_window.txt."""
import functools

import numpy as np
import pytest

import avoidance_reference as AR
import avoidance_window_reference as AW
import collision_reference as C
import collision_window_reference as CW

# (b) measured on the scene when this file was written: largest |sens - central difference| over largest |central difference|
SENS_MEASURED = 2.548e-3
SENS_BOUND = 2.0 * SENS_MEASURED


# ---------------------------------------------------------------- (a) the state gradient
def slow_state():
    """test_collision_window_host.slow_case: 0.25 m/s, R = 30 m, sigma 40 .. 120 m, velocity uncertainty with 30 % correlation"""
    from test_collision_window_host import slow_case
    R, d0, w, A0, B0, D0, T = slow_case()

    def state(tau, dd=np.zeros(3), dw=np.zeros(3)):
        A = A0[:, :, None] + tau * (B0 + B0.T)[:, :, None] + (tau * tau) * D0[:, :, None]
        return ((d0 + dd)[:, None] + w[:, None] * tau, np.repeat((w + dw)[:, None], len(tau), 1), A, B0[:, :, None] + tau * D0[:, :, None],
                np.repeat(D0[:, :, None], len(tau), 2))
    lw = np.sqrt(np.linalg.eigvalsh(D0 - B0 @ np.linalg.inv(A0) @ B0.T).min())      # the conditional velocity's smallest sigma
    return R, 0.0, T, state, 40.0, lw


def fast_state():
    """test_collision_window_host.fast_case at R / sigma_min = 1: 7 km/s, sigma 100 .. 500 m, no velocity uncertainty"""
    from test_collision_window_host import fast_case
    R, d0, w, A, h = fast_case(np.random.default_rng(12), 1.0)
    Z = np.zeros((3, 3, 1))

    def state(tau, dd=np.zeros(3), dw=np.zeros(3)):
        return ((d0 + dd)[:, None] + w[:, None] * tau, np.repeat((w + dw)[:, None], len(tau), 1), np.repeat(A[:, :, None], len(tau), 2),
                np.repeat(Z, len(tau), 2), np.repeat(Z, len(tau), 2))
    return R, -h, h, state, 100.0, float(np.linalg.norm(w))


@pytest.mark.parametrize("scene", [slow_state, fast_state])
def test_state_gradient_against_central_differences(scene):
    """c_q / omega_q = d rate / d (d, w) at the 64 time nodes of one panel, and d START / dd, against central differences of
    collision_window_reference.entry_rate and ball_probability under shifted means.
    Step and bound.  The integrands are Gaussians in d of width l_d = the smallest position sigma (40 m slow, 100 m fast) and, in w,
    error functions of width l_w = the smallest conditional velocity sigma (slow) or linear in w, scale |w| (fast: no velocity
    uncertainty, and the kink n . w = 0 stays on the rule's equator because the pole follows w).  A central difference with step
    eps = 1e-4 l has the truncation error eps^2 / 6 |f'''| -- the third derivative of a Gaussian-like f is at most 1.38 max|f| / l^3
    (the largest |He_3(x)| exp(-x^2 / 2)), taken ten times over for the three dimensions and the factor E: 2.5 (eps / l)^2 max|f| / l
    -- and the rounding error eta max|f| / eps with eta = 1e-13 for a sum of 512 terms of exp and erfc: together (2.5e-8 + 1e-9)
    max|f| / l, max|f| the largest rate over the window; for the ball term max|f| is the density's peak times the ball's volume.
    The velocity components have one more term.  entry_rate places the sphere rule's pole along the w it is given, so its difference
    quotient also holds the change of the rule's quadrature error with the pole -- nothing in the continuum, and not differentiated
    (include/mpcx.h).  That share is the reference's own error: it is measured here from the rate alone, as the difference between
    the quotient with the pole following w and the quotient of the same expressions with the pole held (rate_and_gradient(wf=...),
    whose rate has entry_rate's bits), and added to the bound node by node; against the held pole the bound stands as it is."""
    R, ta, tb, state, ld, lw = scene()
    ok, tau, c, _, start, entries = AW.state_gradient(R, ta, tb, 1, state)
    assert ok and c.shape == (65, 6)
    om = (0.5 * (tb - ta)) * CW.GL_W
    tq = tau[:64]
    _, rate = CW.entry_rate(R, *state(tq))
    w0 = state(tq)[1]
    assert np.array_equal(rate, AW.rate_and_gradient(R, *state(tq), grad=False)[1])
    rel = 2.5 * 1e-8 + 1e-13 / 1e-4
    worst = 0.0
    for e in range(6):
        l = ld if e < 3 else lw
        eps = 1e-4 * l
        sh = np.zeros(3); sh[e % 3] = eps
        plus = state(tq, sh, np.zeros(3)) if e < 3 else state(tq, np.zeros(3), sh)
        minus = state(tq, -sh, np.zeros(3)) if e < 3 else state(tq, np.zeros(3), -sh)
        fd = (CW.entry_rate(R, *plus)[1] - CW.entry_rate(R, *minus)[1]) / (2.0 * eps)
        bound = rel * rate.max() / l
        own = np.zeros(64)
        if e >= 3:                                                       # the reference's own error: its pole follows the shifted w
            held = (AW.rate_and_gradient(R, *plus, wf=w0, grad=False)[1] - AW.rate_and_gradient(R, *minus, wf=w0, grad=False)[1]) / (2.0 * eps)
            own = np.abs(fd - held)
            print(f"{scene.__name__} component {e}: error against the pole held {np.abs(c[:64, e] / om - held).max():.3e}")
            assert np.abs(c[:64, e] / om - held).max() <= bound
        err = np.abs(c[:64, e] / om - fd)
        print(f"{scene.__name__} component {e}: largest |c/omega| {np.abs(fd).max():.3e}, error {err.max():.3e}, bound {bound:.3e}, "
              f"the moving pole's share of the difference quotient {own.max():.3e}")
        worst = max(worst, (err / (bound + own)).max())
        assert np.abs(fd).max() > 100.0 * bound and (err <= bound + own).all()
    d, w, A, _, _ = state(np.array([ta]))
    cden = CW.INV_2PI_32 / np.sqrt(np.linalg.det(A[:, :, 0]))
    for e in range(3):
        eps = 1e-4 * ld
        sh = np.zeros(3); sh[e] = eps
        fd = (CW.ball_probability(R, d[:, 0] + sh, w[:, 0], A[:, :, 0])[1] - CW.ball_probability(R, d[:, 0] - sh, w[:, 0], A[:, :, 0])[1]) / (2.0 * eps)
        bound = rel * (cden * 4.0 / 3.0 * np.pi * R ** 3) / ld
        print(f"{scene.__name__} ball component {e}: start {start:.3e}, d start / dd {fd:.3e}, error {abs(c[64, e] - fd):.3e}, bound {bound:.3e}")
        assert abs(c[64, e] - fd) <= bound
    assert not c[64, 3:].any()
    print(f"{scene.__name__}: worst error / bound {worst:.3f}")


def test_coincident_means_have_no_gradient():
    """d = w = 0 exactly: the integrand is odd in n and c_q is 0, not the rounding of the rule's antipodal points"""
    R, ta, tb, state, _, _ = slow_state()
    still = lambda tau: tuple(np.zeros_like(x) if i < 2 else x for i, x in enumerate(state(tau)))
    ok, _, c, Ec, start, _ = AW.state_gradient(R, ta, tb, 1, still)
    assert ok and start > 0.0 and not c.any()


# ---------------------------------------------------------------- (b) the thrust gradient
HALF, PANELS = 150.0, 1


@functools.lru_cache(maxsize=None)
def slow_pair(at=20.37):
    """avoidance_reference.thrusting_arc() and an object planted to pass it slowly at `at` node intervals: 120 m away, on the circular
    orbit through that point along the arc's own direction turned by 1e-4 rad (as collision_window_reference.window_scene plants its
    slow rows).  Random covariances at the nodes of both, radii 10 + 20 m, a half window of 150 s (about one node interval each way).
    -> sc, t, rows, cat, pairs, stage (the oracle's A, B_kn, B_kp).  Treat as read-only."""
    sc = AR.thrusting_arc()
    return (sc,) + pair_on_arc(sc["x"], sc, at) + ((sc["A"][None], sc["Bn"][None], sc["Bp"][None]),)


def pair_on_arc(x, sc, at):
    """the object planted on the arc x (7, K) of avoidance_reference's scene, covariances and radii -> t, rows, cat, pairs"""
    K = AR.SCENE["K"]
    rng = np.random.default_rng(41)
    hn = (sc["span"][1] - sc["span"][0]) / (K - 1)
    t = sc["span"][0] + at * hn
    p, v = AR.arc_position(x, sc, t)
    e = rng.normal(size=3); e /= np.linalg.norm(e)
    q = p + 120.0 * e
    qh = q / np.linalg.norm(q)
    vh = v - (v @ qh) * qh; vh /= np.linalg.norm(vh)
    vhat = np.cos(1e-4) * vh + np.sin(1e-4) * np.cross(qh, vh)
    cspan = np.array([sc["span"][0] - 10.0, sc["span"][1] + 10.0])
    cy, cunits = C.circular_through(q, vhat, t, 41, cspan)
    rows = (x[None], sc["units"][None], sc["span"][None], C.random_covariances(rng, 1, K), np.array([10.0]), None)
    cat = (cy[None], cunits[None], cspan[None], C.random_covariances(rng, 1, 41), np.array([20.0]), None)
    return t, rows, cat, np.array([[0.0, 0.0, 120.0, t]])


def window_q(rows, cat, pairs):
    out, st = CW.collision_probability_window(pairs, rows, HALF, PANELS, cat)
    assert st.tolist() == [0]
    return out[0, CW.PW_START] + out[0, CW.PW_ENTRIES]


def test_thrust_gradient_against_central_differences():
    """sens of the restatement from the oracle's A, B_kn, B_kp against central differences of the restated window probability along
    oracle-propagated arcs U +- eps e, P at the nodes held fixed, for every thrust node and component.
    Step: the probability is a Gaussian of width sigma >= 100 m in the position, and a unit of normalised thrust moves the arc by
    up to 3e5 m at t; eps = 3e-7 moves it by 0.087 m (printed below, asserted below 2 m = sigma / 50): the difference quotient's
    truncation (shift / sigma)^2 is below 1e-6 relative and its rounding, 1e-13 Q / (eps |dQ/du|) = 1.5e-9, likewise.  What is left is
    the linearisation against the nonlinear flow (mpcx_avoidance's own sensitivities miss it by 0.24 to 0.35 % of the largest entry).
    The arc thrusts, so its speed is not the circular one: the pair passes at 6.2 m/s, 900 m either way inside the window.
    Measured when written: Q = 2.856e-3, the window reaches node 22, largest |dQ/du| 0.6187 per unit, mismatch 2.548e-3 of the
    largest entry (SENS_MEASURED).  Asserted: twice that, since eps and the oracle's step limit move it."""
    sc, t, rows, cat, pairs, stage = slow_pair()
    K = AR.SCENE["K"]
    grads = AW.row_gradients(pairs, rows, HALF, PANELS, cat)
    sens, Es, st = AW.window_sensitivity(grads, rows, stage, "i", cat)
    assert st.tolist() == [0] and grads[0]["st"] == 0
    g = sens[0, 0]
    ke = int(np.flatnonzero(np.abs(g).sum(axis=0))[-1]) - 1
    eps, shift = 3e-7, 0.0
    fd = np.zeros((3, K))
    for m in range(ke + 3):
        for c in range(3):
            Up, Um = sc["U"].copy(), sc["U"].copy()
            Up[c, m] += eps; Um[c, m] -= eps
            xp, xm = AR.propagate_arc(Up, sc), AR.propagate_arc(Um, sc)
            shift = max(shift, 0.5 * float(np.linalg.norm(AR.arc_position(xp, sc, t)[0] - AR.arc_position(xm, sc, t)[0])))
            qp, qm = window_q((xp[None],) + rows[1:], cat, pairs), window_q((xm[None],) + rows[1:], cat, pairs)
            fd[c, m] = (qp - qm) / (2.0 * eps)
    d, w, _, _, _ = CW.relative_state(rows, cat, 0, 0, np.array([t]), CW.MU_EARTH)
    err = np.abs(g - fd).max() / np.abs(fd).max()
    print(f"largest shift of the arc at t {shift:.3f} m, relative speed {np.linalg.norm(w):.3f} m/s, distance {np.linalg.norm(d):.1f} m, Q {grads[0]['start'] + grads[0]['entries']:.4e}, "
          f"last node reached {ke + 1}, largest |dQ/du| {np.abs(fd).max():.4e}, mismatch {err:.3e} of it (bound {SENS_BOUND:.3e}), "
          f"largest rounding bound over largest entry {Es.max() / np.abs(g).max():.1e}")
    assert np.linalg.norm(w) < 10.0 and shift < 2.0
    assert (g[:, ke + 2:] == 0.0).all() and np.abs(fd[:, ke + 2]).max() <= 1e-3 * np.abs(fd).max()
    assert err <= SENS_BOUND


# ---------------------------------------------------------------- (c) the manoeuvre
def manoeuvre(target_p, tol=1e-6, max_eval=40, pairs=None, cat=True, at=20.37):
    sc, t, rows, cat_, pr, stage = slow_pair(at)
    pr = pr if pairs is None else pairs
    cols = cat_ if cat else None
    grads = AW.row_gradients(pr, rows, HALF, PANELS, cols)
    sens, Es, st = AW.window_sensitivity(grads, rows, stage, "i", cols)
    out, du, status, _ = AW.avoidance_window(grads, sens, Es, st, rows, stage, target_p, tol, max_eval, PANELS, "i", cols)
    return grads, sens, out, du, status


def test_manoeuvre_reaches_the_target():
    """two decades down: Q at the returned alpha, evaluated again through the restated response, is within tol of the target in ln;
    the window rule of collision_window_reference on the moved means, whose pole follows the moved w, is printed beside it (3.4e-5
    apart in ln when written: the rule's own dependence on its pole, two and a half decades down the tail) and only held to 1e-3,
    where a wrong response would begin; the first-order prediction has the sign and the order of the change"""
    sc, t, rows, cat, pairs, stage = slow_pair()
    tol = 1e-6
    grads, sens, out, du, status = manoeuvre(1.0e-5, tol)
    o = out[0]
    assert status.tolist() == [0] and o[AW.P0] > 1e-3 and o[AW.ALPHA] > 0.0 and 1 <= o[AW.EVALS] <= 40
    du1, Gam, dv, um = AW.direction(rows, sens[0], (0, 0), (True, False), AR.SCENE["K"])
    dx = AW.response(stage[0][0], stage[1][0], stage[2][0], du1[0], AR.SCENE["K"])
    Q = AW.shifted_window(grads[0], rows, cat, [(rows, 0, -1.0, dx)], PANELS)
    again = Q(o[AW.ALPHA])
    assert again == o[AW.P1] and abs(np.log(again / 1.0e-5)) <= tol
    assert Q(0.0) == o[AW.P0] == grads[0]["start"] + grads[0]["entries"]

    def moved(tau):
        d, w, A, B, D = CW.relative_state(rows, cat, 0, 0, tau, CW.MU_EARTH)
        k, bp, bv = AW.bases(rows, 0, tau)
        x0, x1 = dx[k].T, dx[k + 1].T
        dd = -(bp[0] * x0[0:3] + bp[1] * x0[3:6] + bp[2] * x1[0:3] + bp[3] * x1[3:6])
        dw = -(bv[0] * x0[0:3] + bv[1] * x0[3:6] + bv[2] * x1[0:3] + bv[3] * x1[3:6])
        return d + o[AW.ALPHA] * dd, w + o[AW.ALPHA] * dw, A, B, D
    st, wo = CW.window_probability(grads[0]["R"], grads[0]["ta"], grads[0]["tb"], PANELS, moved)
    free = wo[CW.PW_START] + wo[CW.PW_ENTRIES]
    print(f"P0 {o[AW.P0]:.4e} -> P1 {o[AW.P1]:.6e} (target 1e-5) at alpha {o[AW.ALPHA]:.4e} after {int(o[AW.EVALS])} evaluations; the pole on the moved w: "
          f"{free:.6e}; first-order change {o[AW.DQ_LINEAR]:.3e} against {o[AW.P1] - o[AW.P0]:.3e}; dv {o[AW.DV_I]:.4f} m/s, umax {o[AW.UMAX_I]:.3e}")
    assert st == 0 and abs(np.log(free / 1.0e-5)) <= 1e-3
    assert o[AW.DQ_LINEAR] < 0.0 and o[AW.DV_J] == 0.0 and o[AW.UMAX_J] == 0.0 and o[AW.DV_I] > 0.0
    assert np.array_equal(du[0], o[AW.ALPHA] * du1) and abs(o[AW.DQ_LINEAR] + o[AW.ALPHA] * Gam) <= 1e-15 * o[AW.ALPHA] * Gam


def test_manoeuvre_edges():
    """at or below the target: zeros; the same object twice: SINGULAR; a target below the floor the window's start leaves, with six
    evaluations: INFEASIBLE; a reachable one with too few to close the bracket: MAXITER"""
    sc, t, rows, cat, pairs, stage = slow_pair()
    grads, sens, out, du, status = manoeuvre(0.5)
    assert status.tolist() == [0] and not du.any() and out[0, AW.P0] == out[0, AW.P1] == grads[0]["start"] + grads[0]["entries"]
    assert not out[0, AW.ALPHA:].any() and sens.any()
    grads, sens, out, du, status = manoeuvre(1e-5, pairs=np.array([[0.0, 0.0, 0.0, t]]), cat=False)
    assert grads[0]["st"] == 0 and grads[0]["start"] > 1e-5 and not sens.any()
    assert status.tolist() == [AW.ST_SINGULAR] and np.isnan(out).all() and np.isnan(du).all()
    # a window cut at the arc's first node: dx_0 = 0, no thrust moves the mean there, START is a floor under Q
    grads, sens, out, du, status = manoeuvre(1e-9, max_eval=6, at=0.3)
    assert grads[0]["ta"] == sc["span"][0] and grads[0]["start"] > 1e-7 and sens.any()
    assert status.tolist() == [AW.ST_INFEASIBLE] and np.isnan(out).all() and np.isnan(du).all()
    grads, sens, out, du, status = manoeuvre(1e-5, tol=1e-12, max_eval=3)
    assert status.tolist() == [AW.ST_MAXITER] and np.isnan(out).all() and np.isnan(du).all()


# ---------------------------------------------------------------- (d) the wrappers without a device
S, N = 2, 5
Y, U, UNITS, SPAN, P = np.zeros((S, 7, N)), np.zeros((S, 3, N)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S), np.zeros((S, N, 6, 6))
GOOD = dict(pairs=np.array([[0.0, 1.0, 100.0, 0.5]]), radius=5.0, Y=Y, U=U, units=UNITS, span=SPAN, consts=np.ones((S, 8)), P=P, half_window=10.0)
CAT = (Y, UNITS, SPAN, P, 1.0)


def test_wrapper_argument_checks():
    from mpconstellation_amd import conjunction as cj, _ffi
    bad = [dict(pairs=np.zeros((1, 3))), dict(radius=[1.0, 2.0, 3.0]), dict(P=None), dict(P=np.zeros((S, N, 6, 5))), dict(U=np.zeros((S, 3, N + 1))),
           dict(consts=np.ones((S, 7))), dict(Y=np.zeros((S, 7, 1)), U=np.zeros((S, 3, 1)), P=np.zeros((S, 1, 6, 6))), dict(mu=0.0), dict(ns=[5]),
           dict(max_step=0.0), dict(who="k"), dict(cat=CAT, who="j"), dict(cat=CAT, who="both"), dict(cat=(Y, UNITS, SPAN, P)),
           dict(cat=(Y, UNITS, SPAN, np.zeros((S, N, 6)), 1.0)), dict(cat=(Y, UNITS, SPAN, P, [1.0, 2.0, 3.0])),
           dict(half_window=None), dict(half_window=[1.0, 2.0]), dict(panels=0), dict(panels=1.5), dict(panels=_ffi.PW_MAX_PANELS + 1)]
    for kw in bad:
        with pytest.raises(ValueError):
            cj.collision_window_sensitivity(**{**GOOD, **kw})
        with pytest.raises(ValueError):
            cj.avoidance_window(target_p=1e-4, **{**GOOD, **kw})
    for kw in (dict(target_p=0.0), dict(target_p=1.0), dict(target_p=np.nan), dict(target_p=[0.1]), dict(tol=0.0), dict(tol=np.inf), dict(max_eval=0),
               dict(max_eval=2.5)):
        with pytest.raises(ValueError):
            cj.avoidance_window(**{**dict(target_p=1e-4), **GOOD, **kw})
    with pytest.raises(ValueError, match="target_p.*strictly between 0 and 1"):
        cj.avoidance_window(target_p=1.5, **GOOD)
    with pytest.raises(ValueError, match="only the satellite can manoeuvre"):
        cj.avoidance_window(target_p=0.5, **{**GOOD, "cat": CAT, "who": "both"})


def test_the_empty_list_makes_no_library_call(monkeypatch):
    from mpconstellation_amd import conjunction as cj, _ffi

    def no_call(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(_ffi, "call", no_call)
    monkeypatch.setattr(_ffi, "context", no_call)
    monkeypatch.setattr(_ffi, "atmosphere_context", no_call)
    empty_ev = cj.EncounterEvents(np.zeros((3, 2, 4)), np.zeros((3, 2, 2), dtype=np.int32), np.zeros(3, dtype=np.int32), np.zeros(3, dtype=np.int32))
    for kw in (dict(), dict(cat=CAT), dict(devices=[0, 0]), dict(pairs=empty_ev), dict(who="both")):
        args = {**GOOD, "pairs": np.zeros((0, 4)), **kw}
        NS = 1 if "cat" in kw else 2
        r = cj.collision_window_sensitivity(return_state_gradient=True, panels=2, **args)
        assert isinstance(r, cj.WindowSensitivityResult) and r.sens.shape == (0, NS, 3, N) and r.state_grad.shape == (0, 129, 6) and r.p.shape == (0,)
        a = cj.avoidance_window(target_p=1e-4, return_sensitivities=True, **args)
        assert isinstance(a, cj.AvoidanceWindowResult) and a.du.shape == a.sens.shape == (0, NS, 3, N) and a.p0.shape == a.evals.shape == (0,)
        assert a.dv.shape == a.umax.shape == (0, 2) and a.status.dtype == np.int32
    with pytest.raises(AssertionError, match="the library was called"):
        cj.avoidance_window(target_p=1e-4, **GOOD)


def test_result_columns_and_apply(monkeypatch):
    """the wrapper hands the library one row per stored event of an EncounterEvents, maps the columns by name, and apply adds a row's
    du to its satellites"""
    from mpconstellation_amd import conjunction as cj, _ffi
    seen = {}

    def fake_call(name, ctx, n, *args):
        seen.update(name=name, n=n, target=args[-7], tol=args[-6], max_eval=args[-5], who=args[-8], panels=args[-9])
        out = np.ctypeslib.as_array(args[-4], shape=(n * _ffi.NAW,)).reshape(n, _ffi.NAW)
        out[:] = np.arange(_ffi.NAW)[None, :] + 10.0 * np.arange(n)[:, None]
        np.ctypeslib.as_array(args[-3], shape=(n * 2 * 3 * N,))[:] = 1.0
    monkeypatch.setattr(_ffi, "call", fake_call)
    monkeypatch.setattr(_ffi, "atmosphere_context", lambda *a: None)
    ev = np.zeros((2, 3, 4)); ev[0, :2, 3] = (0.25, 0.75); ev[1, 0, 3] = 0.5; ev[:, :, 1] = 1.0
    events = cj.EncounterEvents(ev, np.zeros((2, 3, 2), dtype=np.int32), np.array([2, 1], dtype=np.int32), np.zeros(2, dtype=np.int32))
    r = cj.avoidance_window(target_p=1e-3, **{**GOOD, "pairs": events, "half_window": [1.0, 2.0, 3.0], "panels": 3, "who": "both", "tol": 1e-4, "max_eval": 7})
    assert seen == dict(name="mpcx_avoidance_window", n=3, target=1e-3, tol=1e-4, max_eval=7, who=2, panels=3)
    assert r.pairs[:, 3].tolist() == [0.25, 0.75, 0.5] and r.sens is None
    assert r.p0.tolist() == [0.0, 10.0, 20.0] and r.p1.tolist() == [1.0, 11.0, 21.0] and r.alpha.tolist() == [2.0, 12.0, 22.0]
    assert r.dq_linear.tolist() == [3.0, 13.0, 23.0] and r.dv.tolist() == [[4.0, 5.0], [14.0, 15.0], [24.0, 25.0]]
    assert r.umax.tolist() == [[6.0, 7.0], [16.0, 17.0], [26.0, 27.0]] and r.evals.tolist() == [8.0, 18.0, 28.0]
    U2 = r.apply(U, 1)
    assert U2.shape == U.shape and (U2 == 1.0).all() and not U.any()
    r.status[2] = 4
    with pytest.raises(ValueError, match="no manoeuvre"):
        r.apply(U, 2)


def test_constellation_avoidance_window_needs_a_plan():
    from test_conjunction_host import hand_made_mpc
    mpc, _ = hand_made_mpc()
    with pytest.raises(ValueError, match="no plan"):
        mpc.avoidance_window(1000.0, np.eye(6), 5.0, 60.0, 1e-6)
