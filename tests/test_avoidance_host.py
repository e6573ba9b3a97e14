"""The avoidance manoeuvre's formulas (avoidance_reference.py, the restatement of include/mpcx.h: mpcx_avoidance) against the
nonlinear dynamics of the CPU oracle, without a GPU: the thrust sensitivities against central differences, the manoeuvre against
a second propagation, the steepest direction against a scan of the target ellipse; and the wrapper's argument checks.

The scene (avoidance_reference.thrusting_arc): a 7000 km orbit, tf = 0.8, K = 30, U = 0.02 standard_normal, propagated with
max_step 1e-3 and linearised with max_step 1e-2 by the oracle.  The measured figures quoted below are in profiles/avoidance.txt."""
import numpy as np
import pytest
from scipy.optimize import minimize_scalar

import avoidance_reference as AR
import collision_reference as C

# Measured on the scene when this file was written (each test prints its figures).
# Sensitivities, largest entry error over largest entry, per time of closest approach.  At the three times with a history behind them
# it is the discretiser's rtol 1e-3 quadrature, 3e-3.  Inside the FIRST interval every entry of g is one interval's B_kn or B_kp entry
# on its own, and the discretiser splits an interval's input influence between its two nodes by the trapezoid rule over the n = 4
# integrator steps that max_step = 1e-2 leaves in an interval of 1 / 29: the position rows of B_kn are off by 1 / (2 n^2) = 3 % and
# those of B_kp by 1 / n^2 = 6 % of themselves (their sum is right to 3e-4); later that error is still there, under 1e-3 of the entries
# that have grown by then.  It is the linearisation's, the reference's included, not the sweep's: the bound of that case is its own.
SENS_MEASURED = {"node 17": 3.04e-3, "mid-interval 11": 3.46e-3, "first interval": 6.35e-2, "last node": 2.43e-3}
SENS_BOUND = {name: 3.0 * v for name, v in SENS_MEASURED.items()}
MISS_WORST = 1.43e-4                # |nonlinear miss - MISS1| / MISS1 after the 200 m -> 1000 m manoeuvre (the second-order term of a 980 m change)
MISS_BOUND = min(10.0 * MISS_WORST, 1e-2)      # never looser than 1e-2, where an error in L, Tu or c_m begins


def encounter_times(sc):
    """at a node, mid-interval, inside the first interval, at the last node"""
    hn = (sc["span"][1] - sc["span"][0]) / (AR.SCENE["K"] - 1)
    return {"node 17": sc["span"][0] + 17 * hn, "mid-interval 11": sc["span"][0] + 11.5 * hn, "first interval": sc["span"][0] + 0.4 * hn,
            "last node": sc["span"][1]}


def frame_at(sc, t):
    """the frame of the planted encounter at t: R = [e_1 e_2 e_w]^T, |m|, |w| and the object"""
    y, units, span = AR.planted_object(sc, t)
    pa, va = AR.arc_position(sc["x"], sc, t)
    st, pb, vb, _, _ = C.state_and_cov_at((y[None], units[None], span[None], np.zeros((1, y.shape[1], 6, 6)), np.zeros(1), None), 0.0, t, C.MU_EARTH)
    assert st == 0
    ew, e1, e2, mn, wn = AR.frame(pb - pa, vb - va)
    return np.stack([e1, e2, ew]), mn, wn, (y, units, span)


def restated_sens(sc, t, Rf, swapped=False):
    L, Tu = sc["units"]
    k, basis, hn, nn = AR.node_of(sc["x"][None], sc["units"][None], sc["span"][None], None, 0, t)
    hi, lo = AR.seeds(-Rf, L, AR.SCENE["tf"] / (nn - 1), basis)
    Bn, Bp = (sc["Bp"], sc["Bn"]) if swapped else (sc["Bn"], sc["Bp"])
    return AR.sweep(sc["A"], Bn, Bp, k, hi, lo, AR.SCENE["K"]), k


@pytest.fixture(scope="module")
def central_differences():
    """d p(t) / d U[c, m] of the nonlinear arc for the four times: {name: (3, 3, K)} (space component, thrust component, node), m/unit"""
    sc = AR.thrusting_arc()
    K, h = AR.SCENE["K"], 1e-3
    times = encounter_times(sc)
    out = {name: np.zeros((3, 3, K)) for name in times}
    for m in range(K):
        for c in range(3):
            Up, Um = sc["U"].copy(), sc["U"].copy()
            Up[c, m] += h; Um[c, m] -= h
            xp, xm = AR.propagate_arc(Up, sc), AR.propagate_arc(Um, sc)
            for name, t in times.items():
                out[name][:, c, m] = (AR.arc_position(xp, sc, t)[0] - AR.arc_position(xm, sc, t)[0]) / (2.0 * h)
    return out


def test_sensitivities_against_central_differences(central_differences):
    """g_m of the restatement from the oracle's A, B_kn, B_kp against central differences of the oracle's nonlinear propagation with
    respect to every thrust node, at four times of closest approach.  Measure: largest entry error over largest entry, per time.
    Asserted at 3 x the figure measured for that time (SENS_MEASURED); with B_kn and B_kp swapped the same measure is 4e-2 or more
    (0.9 in the first interval) and must exceed that same bound at every one of the four times: the test tells the conventions apart."""
    sc = AR.thrusting_arc()
    for name, t in encounter_times(sc).items():
        Rf, _, _, _ = frame_at(sc, t)
        fd = -np.einsum("ra,acm->rcm", Rf, central_differences[name])            # object i: d = p_b - p_a
        g, k = restated_sens(sc, t, Rf)
        gs, _ = restated_sens(sc, t, Rf, swapped=True)
        err, err_s = np.abs(g - fd).max() / np.abs(fd).max(), np.abs(gs - fd).max() / np.abs(fd).max()
        print(f"{name}: k {k}, largest |g| {np.abs(fd).max():.4e} m/unit, error {err:.3e} (bound {SENS_BOUND[name]:.3e}), "
              f"with B_kn / B_kp swapped {err_s:.3e}")
        assert (g[:, :, k + 2:] == 0.0).all() and (g[:, :, :k + 2] != 0.0).any()
        assert np.abs(fd[:, :, k + 2:]).max(initial=0.0) <= 1e-4 * np.abs(fd).max()         # later nodes do not move p(t) (but for the integrator's step across node k + 1)
        assert err <= SENS_BOUND[name], (name, err)
        assert err_s > SENS_BOUND[name], (name, err_s)


def scene_manoeuvre(W=None, target=1000.0):
    """the planted encounter 200 m from the arc at a mid-interval time, and the restated manoeuvre of the arc alone"""
    sc = AR.thrusting_arc()
    hn = (sc["span"][1] - sc["span"][0]) / (AR.SCENE["K"] - 1)
    t = sc["span"][0] + 20.37 * hn
    y, units, span = AR.planted_object(sc, t)
    rows = (sc["x"][None], sc["units"][None], sc["span"][None], None)
    stage = (sc["A"][None], sc["Bn"][None], sc["Bp"][None])
    cat = (y[None], units[None], span[None], None, None)
    out, du, sens, status = AR.avoidance(np.array([[0.0, 0.0, 200.0, t]]), rows, stage, target, "i", cat=cat)
    assert status.tolist() == [0]
    return sc, t, (y, units, span), out[0], du[0, 0], sens[0, 0]


def test_manoeuvre_under_the_nonlinear_dynamics():
    """200 m -> 1000 m (W = I): apply du, propagate again with the oracle, recompute the encounter-plane miss at t + DT.  The linear
    prediction MISS1 is the reference; measured 1.2e-4 relative (the second-order term of a 800 m change), asserted at 10 x that
    and never looser than 1e-2."""
    sc, t, (y, units, span), out, du, _ = scene_manoeuvre()
    assert abs(out[AR.D0] - 200.0) < 1.0 and abs(out[AR.D1] - 1000.0) < 1e-6 and abs(out[AR.MISS1] - 1000.0) < 1e-6
    assert (du[:, 22:] == 0.0).all() and np.abs(du).max() == pytest.approx(out[AR.UMAX_I], rel=0.5)
    x2 = AR.propagate_arc(sc["U"] + du, sc)
    t2 = t + out[AR.DT]
    pa, va = AR.arc_position(x2, sc, t2)
    st, pb, vb, _, _ = C.state_and_cov_at((y[None], units[None], span[None], np.zeros((1, y.shape[1], 6, 6)), np.zeros(1), None), 0.0, t2, C.MU_EARTH)
    _, _, _, miss, wn = AR.frame(pb - pa, vb - va)
    along = (pb - pa) @ (vb - va) / wn
    p0, _ = AR.arc_position(sc["x"], sc, t)
    rel = abs(miss - out[AR.MISS1]) / out[AR.MISS1]
    print(f"position change {np.linalg.norm(AR.arc_position(x2, sc, t)[0] - p0):.1f} m, dv {out[AR.DV_I]:.4f} m/s, umax {out[AR.UMAX_I]:.3e}, "
          f"DT {out[AR.DT]:.4f} s, nonlinear miss {miss:.3f} m against MISS1 {out[AR.MISS1]:.3f} m: {rel:.3e} relative; "
          f"offset left along the relative velocity {along:.2f} m")
    assert st == 0 and rel <= MISS_BOUND
    assert abs(along) <= 1e-2 * miss                                         # t + DT is the new time of closest approach


def test_steepest_direction_against_the_scan_of_the_target_ellipse():
    """Anisotropic W (axis ratio 10, the miss at 45 degrees to the axes), target 4 sigma: the effort dm^T M^-1 dm of the steepest
    direction against the minimum over the target ellipse by a scan of 3600 angles (the grid passes through the W-radial point, so
    that the isotropic case below is on it).  No bound on the excess -- it is printed and recorded -- except that the scan cannot
    find less than nothing better than itself: steepest >= minimum; and when M W is a multiple of the identity the two agree to 1e-9."""
    _, _, _, out, _, sens = scene_manoeuvre()
    mn = out[AR.D0]
    k = 20
    sc = AR.thrusting_arc()
    L, Tu = sc["units"]
    hn = (sc["span"][1] - sc["span"][0]) / (AR.SCENE["K"] - 1)
    gh = sens[0:2, :, :k + 2] / ((L / (Tu * Tu)) / sc["x"][6, :k + 2])
    M = np.einsum("acm,bcm->ab", gh / AR.node_weights(hn, AR.SCENE["K"], AR.SCENE["K"])[:k + 2], gh)
    c45 = np.sqrt(0.5)
    Q = np.array([[c45, -c45], [c45, c45]])
    W = Q @ np.diag([1.0 / 1000.0 ** 2, 1.0 / 100.0 ** 2]) @ Q.T
    target = 4.0

    def efforts(W, M):
        d0, dm, lam, d1, _ = AR.solve_manoeuvre(mn, W, M, target)
        assert d0 < target and abs(d1 - target) <= 1e-9 * target
        m = np.array([mn, 0.0])
        Wh = np.linalg.cholesky(W).T                                         # x^T W x = |Wh x|^2
        th0 = np.arctan2(*(Wh @ m)[::-1])
        th = th0 + 2.0 * np.pi * np.arange(3600) / 3600.0

        def effort(th):
            D = np.linalg.solve(Wh, target * np.stack([np.cos(th), np.sin(th)])) - (m[:, None] if np.ndim(th) else m)      # ellipse - m
            return np.einsum("a...,a...->...", D, np.linalg.solve(M, D))
        scan = effort(th)
        j = int(np.argmin(scan))
        fine = minimize_scalar(effort, bounds=(th[j] - 2.0 * np.pi / 3600.0, th[j] + 2.0 * np.pi / 3600.0), method="bounded", options=dict(xatol=1e-13))
        return dm @ np.linalg.solve(M, dm), min(scan[j], float(fine.fun)), scan[j]
    steep, best, coarse = efforts(W, M)
    print(f"effort of the steepest direction {steep:.9e}, minimum over the ellipse {best:.9e} (3600 angles: {coarse:.9e}): excess {steep / best - 1.0:.3e}")
    assert steep >= best * (1.0 - 1e-9)
    steep_i, best_i, coarse_i = efforts(W, 3.0e5 * np.linalg.inv(W))
    print(f"M W = 3e5 I: steepest {steep_i:.12e}, scan {coarse_i:.12e}")
    assert abs(steep_i - coarse_i) <= 1e-9 * coarse_i and abs(steep_i - best_i) <= 1e-9 * best_i


def test_wrapper_argument_checks():
    """shapes, who='j' with a catalogue, one-sided P, a bad target: ValueError before any library call (there is no device here to call)"""
    from mpconstellation_amd import avoidance, AvoidanceResult, conjunction
    S, K, D, Kc = 2, 5, 3, 4
    Y, U, units, span, consts = np.ones((S, 7, K)), np.zeros((S, 3, K)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S), np.ones((S, 8))
    pairs = np.array([[0.0, 1.0, 10.0, 0.5]])
    cat = (np.ones((D, 7, Kc)), np.ones((D, 2)), np.array([[0.0, 1.0]] * D))
    P, cP = np.zeros((S, K, 6, 6)), np.zeros((D, Kc, 6, 6))
    good = dict(pairs=pairs, target=100.0, Y=Y, U=U, units=units, span=span, consts=consts)
    for bad in (dict(pairs=np.zeros((1, 3))), dict(target=0.0), dict(target=-1.0), dict(target=np.inf), dict(target=np.nan), dict(who="k"),
                dict(Y=np.ones((S, 6, K))), dict(Y=np.ones((S, 7, 1)), U=np.zeros((S, 3, 1))), dict(U=np.zeros((S, 3, K + 1))),
                dict(units=np.ones((S, 3))), dict(span=np.ones((S + 1, 2))), dict(consts=np.ones((S, 7))), dict(ns=np.array([5])),
                dict(P=np.zeros((S, K, 6, 5))), dict(cat=cat, who="j"), dict(cat=cat, who="both"), dict(cat=cat, P=P), dict(cat=cat + (cP,)),
                dict(cat=cat[:2]), dict(cat=cat + (np.zeros((D, Kc, 6, 5)),), P=P), dict(cat=cat + (cP, np.array([4, 4]))), dict(max_step=0.0),
                dict(mu=0.0)):
        with pytest.raises(ValueError):
            avoidance(**{**good, **bad})
    res = avoidance(np.zeros((0, 4)), 100.0, Y, U, units, span, consts, return_sensitivities=True)        # an empty list: no library call
    assert isinstance(res, AvoidanceResult) and res.du.shape == (0, 2, 3, K) and res.sens.shape == (0, 2, 3, 3, K) and res.d0.shape == (0,)
    assert conjunction.avoidance(np.zeros((0, 4)), 100.0, Y, U, units, span, consts, cat=cat).du.shape == (0, 1, 3, K)
    # apply: the pair's du lands on its satellites, the given table is left alone
    out = np.zeros((1, AR.NAV)); du = np.arange(2 * 3 * K, dtype=np.float64).reshape(1, 2, 3, K)
    r = AvoidanceResult(np.array([[1.0, 0.0, 5.0, 0.5]]), out, du, None, np.zeros(1, dtype=np.int32))
    U2 = r.apply(U, 0)
    assert np.array_equal(U2[1], du[0, 0]) and np.array_equal(U2[0], du[0, 1]) and not U.any()
    with pytest.raises(ValueError):
        r.apply(np.zeros((S, 3, K + 1)), 0)
