"""The window collision probability without a device: the numpy restatement (collision_window_reference) against independent truths
-- the short-encounter probability in the fast limit, a Monte Carlo count of straight sample paths for a slow encounter, the
non-central chi-square for the ball term, a finite-difference two-body transition for the 6 x 6 carry."""
import warnings

import numpy as np
import pytest

import collision_reference as C
import collision_window_reference as W


def random_rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return Q


def fast_case(rng, ratio):
    """|w| = 7 km/s along a random direction, A = Q diag(100^2, s^2, s'^2) Q^T with s, s' in 100 .. 500 m, B = D = 0, R = ratio x
    100 m, the closest approach at tau = 0 with a miss of up to 2 sigma (a random direction of length <= 2 in the metric of A, its
    component along w removed) -> R, d0, w, A, the half window (8 sigma_max + R) / |w|"""
    sig = np.array([100.0, rng.uniform(100.0, 500.0), rng.uniform(100.0, 500.0)])
    Q = random_rotation(rng)
    A = Q @ np.diag(sig * sig) @ Q.T
    A = 0.5 * (A + A.T)
    e = rng.normal(size=3); e /= np.linalg.norm(e)
    w = 7000.0 * e
    g = rng.normal(size=3); g *= rng.uniform(0.0, 2.0) / np.linalg.norm(g)
    d0 = Q @ (sig * g)
    d0 = d0 - (d0 @ e) * e
    R = ratio * 100.0
    return R, d0, w, A, (8.0 * sig.max() + R) / 7000.0


def plane_truth(R, d0, w, A, adaptive):
    """the short-encounter probability of the same case: the restated 64-point rule inside its 1e-13 domain (R / sigma_2 <= 2), or
    scipy's adaptive double integral over the disc (epsrel 1e-11) in the principal frame of the plane covariance"""
    st, o = C.encounter(np.zeros(3), np.zeros(3), A, d0, w, np.zeros((3, 3)), R)
    assert st == 0
    if not adaptive:
        assert R / o[4] <= 2.0
        return o[0]
    from scipy.integrate import dblquad
    ew = w / np.linalg.norm(w)
    E = np.linalg.svd(np.eye(3) - np.outer(ew, ew))[0][:, :2]
    lam, V = np.linalg.eigh(E.T @ A @ E)
    m = V.T @ (E.T @ d0)

    def f(th, r):
        x, y = r * np.cos(th), r * np.sin(th)
        return r * np.exp(-0.5 * ((x - m[0]) ** 2 / lam[0] + (y - m[1]) ** 2 / lam[1])) / (2.0 * np.pi * np.sqrt(lam[0] * lam[1]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        val, _ = dblquad(f, 0.0, R, 0.0, 2.0 * np.pi, epsabs=1e-300, epsrel=1e-11)
    assert abs(val - o[0]) <= 1e-7 * val                                  # (the fixed rule at R / sigma_2 <= 4: 3e-9)
    return val


def fast_window(R, d0, w, A, h, panels):
    Z = np.zeros((3, 3, 1))
    state = lambda tau: (d0[:, None] + w[:, None] * tau[None, :], np.repeat(w[:, None], len(tau), 1), np.repeat(A[:, :, None], len(tau), 2),
                         np.repeat(Z, len(tau), 2), np.repeat(Z, len(tau), 2))
    st, o = W.window_probability(R, -h, h, panels, state)
    assert st == 0
    return o


@pytest.mark.parametrize("panels,ratios,bound", [(4, (0.05, 0.5, 1.0, 2.0), 1e-9), (4, (4.0,) * 4, 1e-6), (1, (0.05, 0.5, 1.0, 2.0), 1e-5)])
def test_fast_limit_is_the_short_encounter_probability(panels, ratios, bound):
    """No velocity uncertainty, a constant position covariance and a straight line at 7 km/s: start + entries over a window of
    +-(8 sigma_max + R) / |w| is the Gaussian's integral over the disc in the plane across w.  Four random anisotropic cases per
    line, smallest sigma 100 m, misses up to 2 sigma.  Measured when written (worst relative error): 4 panels R / sigma_min <= 2:
    1.3e-14; 4 panels R / sigma_min = 4: 8.8e-7 (3.8e-9 .. 8.8e-7: largest where the smallest sigma lies along w); 1 panel R /
    sigma_min <= 2: 4.7e-7.  Asserted: 1e-9, 1e-6, 1e-5."""
    rng = np.random.default_rng(31 + panels + int(ratios[0] * 100))
    worst = 0.0
    for ratio in ratios:
        R, d0, w, A, h = fast_case(rng, ratio)
        o = fast_window(R, d0, w, A, h, panels)
        ref = plane_truth(R, d0, w, A, adaptive=ratio > 2.0)
        err = abs(o[W.PW_P] - ref) / ref
        print(f"panels {panels} R/sigma_min {ratio}: window {o[W.PW_P]:.12e} plane {ref:.12e} relative {err:.2e} start {o[W.PW_START]:.1e}")
        worst = max(worst, err)
        assert o[W.PW_START] <= 1e-12 * ref                               # (the window opens 8 sigma out)
        assert abs(o[W.PW_T_RATE_MAX]) <= 0.5 * h                         # the rate peaks near the closest approach, not at an end
    print(f"worst relative error {worst:.2e} (bound {bound:.0e})")
    assert worst <= bound


def slow_case():
    sr, sv = np.array([40.0, 120.0, 60.0]), np.array([0.02, 0.05, 0.03])
    A0, D0, B0 = np.diag(sr * sr), np.diag(sv * sv), np.diag(0.3 * sr * sv)      # 30 % correlation of position and velocity per axis
    return 30.0, np.array([-150.0, 40.0, 20.0]), np.array([0.25, -0.02, 0.01]), A0, B0, D0, 1200.0


def test_slow_encounter_against_monte_carlo():
    """Force-free relative motion with velocity uncertainty: rho(tau) = rho_0 + nu tau with (rho_0, nu) Gaussian, so A(tau) = A0 +
    tau (B0 + B0^T) + tau^2 D0, B(tau) = B0 + tau D0, D = D0.  A sample path is a straight line: it enters the sphere at most once,
    and start + entries IS the probability of a hit in [0, T].  400 000 samples (seed 7), each decided in closed form (the closest
    point of its line over [0, T]).  sigma_r = (40, 120, 60) m, sigma_v = (0.02, 0.05, 0.03) m/s, 30 % correlation between position
    and velocity on every axis, R = 30 m, d0 = (-150, 40, 20) m, w = (0.25, -0.02, 0.01) m/s, T = 1200 s.  Measured when written:
    the rule 0.045460 at 1, 2 and 4 panels alike; Monte Carlo 0.045207 +- 0.00033.  Asserted: |rule - MC| <= 4 sqrt(p (1 -
    p) / N), the sampling error and nothing else; the panel counts agree to 1e-6 relative."""
    R, d0, w, A0, B0, D0, T = slow_case()

    def state(tau):
        A = A0[:, :, None] + tau * (B0 + B0.T)[:, :, None] + (tau * tau) * D0[:, :, None]
        return (d0[:, None] + w[:, None] * tau, np.repeat(w[:, None], len(tau), 1), A, B0[:, :, None] + tau * D0[:, :, None],
                np.repeat(D0[:, :, None], len(tau), 2))
    p = []
    for panels in (1, 2, 4):
        st, o = W.window_probability(R, 0.0, T, panels, state)
        assert st == 0 and o[W.PW_TA] == 0.0 and o[W.PW_TB] == T and 0.0 < o[W.PW_T_RATE_MAX] < T
        p.append(o[W.PW_P])
    rng = np.random.default_rng(7)
    N = 400000
    cov = np.block([[A0, B0.T], [B0, D0]])
    x = rng.multivariate_normal(np.concatenate([d0, w]), cov, size=N, method="cholesky")
    r0, nu = x[:, 0:3], x[:, 3:6]
    ts = np.clip(-(r0 * nu).sum(1) / (nu * nu).sum(1), 0.0, T)
    hit = (np.linalg.norm(r0 + nu * ts[:, None], axis=1) <= R).mean()
    se = np.sqrt(hit * (1.0 - hit) / N)
    print(f"rule {p[0]:.6f} {p[1]:.6f} {p[2]:.6f}, Monte Carlo {hit:.6f} +- {se:.5f}")
    assert abs(p[0] - p[2]) <= 1e-6 * p[2] and abs(p[1] - p[2]) <= 1e-6 * p[2]
    for q in p:
        assert abs(q - hit) <= 4.0 * se


def test_ball_term_against_the_noncentral_chi_square():
    """isotropic A = sigma^2 I: P(|rho| <= R) = ncx2.cdf(R^2 / sigma^2, 3, |d|^2 / sigma^2).  R / sigma in {0.1, 0.5, 1, 2}, |d| /
    sigma in {0, 0.5, 1, 2, 3} in random directions with random poles.  Measured when written (worst relative error): 1.2e-15 for R /
    sigma <= 1, 2.1e-11 at 2.  Asserted: 1e-10."""
    from scipy.stats import ncx2
    rng = np.random.default_rng(5)
    worst = {}
    for ratio in (0.1, 0.5, 1.0, 2.0):
        for miss in (0.0, 0.5, 1.0, 2.0, 3.0):
            sig = 10.0 ** rng.uniform(0.0, 3.0)
            e = rng.normal(size=3); e /= np.linalg.norm(e)
            ok, p = W.ball_probability(ratio * sig, miss * sig * e, rng.normal(size=3), sig * sig * np.eye(3))
            ref = ncx2.cdf(ratio * ratio, 3, miss * miss)
            assert ok
            worst[ratio] = max(worst.get(ratio, 0.0), abs(p - ref) / ref)
    print("worst relative error per R / sigma:", {k: f"{v:.1e}" for k, v in worst.items()})
    assert max(worst.values()) <= 1e-10
    ok, _ = W.ball_probability(1.0, np.zeros(3), np.ones(3), np.diag([1.0, 1.0, -1.0]))
    assert not ok


@pytest.mark.parametrize("nodes", [31, 101])
def test_carry_against_finite_difference_truth(nodes):
    """The 6 x 6 short-arc transition at dt = half a node interval of `nodes` nodes per revolution, forwards and backwards, against
    the finite-difference transition over dt, as test_collision_host.py holds the position rows: relative Frobenius difference with
    velocity in units of the mean motion n (rows and columns: D Phi D^-1, D = diag(1, 1, 1, 1/n, 1/n, 1/n), every block of order
    one), bound (n dt)^3 for the whole matrix and for the position rows alone, which are collision_reference.short_arc_rows to the
    bit.  Measured when written (worst orbit, e = 0.15): whole matrix 7.3e-4 at n dt = 0.105 where (n dt)^3 is 1.15e-3 (position rows
    1.04e-3, velocity rows 1.4e-4), 2.0e-5 at n dt = 0.031 where it is 3.10e-5 (position rows 2.8e-5, velocity rows 1.2e-6).
    Velocity rows G dt | I + G dt^2/2 with the node's gradient alone miss this bound 18 and 61 times (2.08e-2, 1.90e-3): G dt neglects
    G' dt^2 / 2, order (n dt)^2.  That is why the velocity rows are Simpson's rule on the gradient along the arc."""
    worst = 0.0
    for which in range(len(C.ORBITS)):
        c = C.orbit_case(which, 30)
        L, Tu = c["units"]
        dt_n = 0.5 / (nodes - 1)
        ndt = 2.0 * np.pi * dt_n
        n = 2.0 * np.pi / Tu
        s = np.array([1.0] * 3 + [1.0 / n] * 3)
        scale = s[:, None] / s[None, :]
        for sign in (1.0, -1.0):
            truth = C.to_physical(C.fd_transition(c["y0"], sign * dt_n), c["units"])
            F = W.short_arc_transition((c["y0"][0:3] * L)[:, None], (c["y0"][3:6] * (L / Tu))[:, None], np.array([sign * dt_n * Tu]), C.MU_EARTH)[0]
            assert np.array_equal(F[0:3], C.short_arc_rows(c["y0"][0:3] * L, sign * dt_n * Tu, C.MU_EARTH))
            err = np.linalg.norm((F - truth) * scale) / np.linalg.norm(truth * scale)
            rows = [np.linalg.norm(((F - truth) * scale)[r]) / np.linalg.norm((truth * scale)[r]) for r in (slice(0, 3), slice(3, 6))]
            print(f"orbit {which} nodes {nodes}: n dt = {sign * ndt:.3f}, error {err:.2e} (position rows {rows[0]:.2e}, velocity rows {rows[1]:.2e}), "
                  f"(n dt)^3 = {ndt ** 3:.2e}")
            assert rows[0] <= ndt ** 3
            worst = max(worst, err / ndt ** 3)
    assert worst <= 1.0


@pytest.mark.parametrize("K", W.SCENE_KS)
def test_rounding_bound_of_the_device_scenes_on_the_cpu(K):
    """The scenes test_collision_window_gpu.py holds the device to: every row good, its rounding bound (collision_window_reference.
    rounding_bound: cond(A), the smallest sigma and the Mahalanobis distance of the sphere points that count) at most 1e-6 relative,
    and the restatement's own fp64 sensitivity inside it -- the first 16 rows evaluated again with every trajectory entry and every
    covariance entry moved by up to one unit in the last place (what another order of the same operations does to them)."""
    sc = W.window_scene(K)
    rng = np.random.default_rng(K)
    eps = np.finfo(np.float64).eps

    def moved(side):
        Y, units, span, P, radius, ns = side
        dP = 1.0 + eps * rng.uniform(-1.0, 1.0, P.shape)
        return (Y * (1.0 + eps * rng.uniform(-1.0, 1.0, Y.shape)), units, span, P * (0.5 * (dP + np.swapaxes(dP, 2, 3))), radius, ns)
    for panels in W.SCENE_PANELS:
        out, status, bound = sc["ref"][panels]
        assert (status == 0).all() and (out[:, W.PW_P] > 0.0).all() and (out[:, W.PW_P] < 1.0).all()
        assert np.isfinite(bound).all() and bound.max() <= 1e-6
    out, _, bound = sc["ref"][1]
    again, st = W.collision_probability_window(sc["pairs"][:16], moved(sc["rows"]), sc["half"][:16], 1, moved(sc["cat"]))
    ratio = np.abs(again[:, W.PW_P] - out[:16, W.PW_P]) / (bound[:16] * out[:16, W.PW_P])
    print(f"K {K}: largest bound {bound.max():.2e}; inputs moved by an ulp: worst |dp| / bound {ratio.max():.3f}")
    assert (st == 0).all() and (ratio <= 1.0).all()
    w = np.linalg.norm(out[:, W.PW_RATE_MAX])                                 # (the scene has what it promises)
    speeds = [np.linalg.norm(W.relative_state(sc["rows"], sc["cat"], int(i), int(j), np.array([t]), W.MU_EARTH)[1]) for i, j, _, t in sc["pairs"]]
    slow = np.arange(W.SCENE_N) % 4 >= 2
    assert w > 0.0 and speeds[3] == 0.0 and max(s for s, f in zip(speeds, slow) if f) < 1.0 and min(s for s, f in zip(speeds, slow) if not f) > 1000.0
