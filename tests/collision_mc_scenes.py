"""The planted scenes of the Monte Carlo collision probability's truth checks, shared by tests/test_collision_mc_gpu.py and
profiles/tools/collision_mc_timing.py (which measures the models' own gaps that the tests assert against).  Every scene is a dict
of collision_probability_mc's arguments: pairs, radius, Y, U, units, span, consts, P0, half_window, and `panels` for the window rule
beside it.  slow_pair and fast_pair are host arithmetic; reentry_pair and thrust_arc fly their nominal trajectories on the device."""
import numpy as np

import collision_reference as C

# The models' own gaps, measured once at N = 2^20 by profiles/tools/collision_mc_timing.py (profiles/collision_mc.txt): the
# difference between the sampled figure and the linearised one where the large run resolves one beyond its own 4 standard errors,
# else 0.  The tests assert at 3 x these.  Measured: the slow pair's START + ENTRIES +1.12 SE_BOUND (+3.1e-4 on 0.0824) and START
# +0.24 SE, the fast pair's P_HIT -0.31 SE (-5.0e-5 on 0.02795), the re-entry pair's START + ENTRIES +0.31 SE_BOUND (+2.8e-4 on
# 0.6877): no gap resolved on any of them.
GAP_SLOW_BOUND, GAP_SLOW_START, GAP_FAST, GAP_REENTRY_BOUND = 0.0, 0.0, 0.0, 0.0


def scale_constants(lengths):
    from mpconstellation_amd.satellite_scale import SatelliteScale
    return np.stack([SatelliteScale(x=np.array([L, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])).get_normalized_constants().as_vector() for L in lengths])


def rtn_covariance(y_first, sigmas):
    """diag(sigmas^2) in the radial / along-track / cross-track frame of a circular orbit's first node (positions, then velocities), in
    the inertial axes"""
    r, v = y_first[0:3] / np.linalg.norm(y_first[0:3]), y_first[3:6] / np.linalg.norm(y_first[3:6])
    Q = np.zeros((6, 6))
    Q[0:3, 0:3] = Q[3:6, 3:6] = np.stack([r, v, np.cross(r, v)], axis=1)
    P0 = Q @ np.diag(np.asarray(sigmas, dtype=np.float64) ** 2) @ Q.T
    return 0.5 * (P0 + P0.T)


SLOW_SIGMAS = (5.0, 30.0, 15.0, 0.03, 0.001, 0.015)


def slow_pair(sigmas=SLOW_SIGMAS, drift=0.25e-5):
    """test_collision_window_gpu.planted_slow's geometry (two objects on one circular orbit of 7000 km, 61 nodes over 6000 s) with a
    lag of 50 m at t = 3000 s closing at 0.25e-5 of the orbital speed (0.019 m/s; the second orbit is 12 m lower), radii 10 and 15 m,
    window 3000 +- 2000 s.  P0 is diagonal in each object's radial / along-track / cross-track frame at the first node, sigmas (5, 30,
    15) m and (0.03, 0.001, 0.015) m/s: what changes the semi-major axis -- the radial position, the along-track velocity -- is known
    best, as after an orbit determination, so that the along-track uncertainty at the encounter stays near 150 m and the window
    figure is 0.08, in the range the check asks for (an isotropic 40 m grows to 500 m along the track in 0.6 revolutions; with the
    second orbit 47 m lower that gave 0.008)."""
    from test_collision_window_gpu import planted_slow
    Y, units, spans, _, radius = planted_slow(lag_m=50.0, drift=drift)
    P0 = np.stack([rtn_covariance(Y[o, :, 0], sigmas) for o in range(2)])
    return dict(pairs=np.array([[0.0, 1.0, 50.0, 3000.0]]), radius=radius, Y=Y, U=None, units=units, span=spans, consts=scale_constants(units[:, 0]),
                P0=P0, half_window=2000.0, panels=4)


def fast_pair():
    """test_collision_window_gpu.planted_fast's geometry (circular orbits 300 m apart in radius, planes 1.2 rad apart, crossing at
    t = 1000 s at 8 km/s, 101 nodes over 2000 s) with radii summing to 100 m and its position-only P0: 200 m isotropic, no velocity
    uncertainty -- a positive SEMI-definite matrix.  The half window is the caller's (encounter_half_window)."""
    from test_collision_window_gpu import planted_fast
    Y, units, spans, P, _ = planted_fast()
    return dict(pairs=np.array([[0.0, 1.0, 300.0, 1000.0]]), radius=np.array([40.0, 60.0]), Y=Y, U=None, units=units, span=spans,
                consts=scale_constants(units[:, 0]), P0=P[0, 0].copy(), half_window=None, panels=4)


def reentry_pair(K=201, sig_r=10.0, sig_v=0.005):
    """Two objects on one orbit of 7000 km with a small relative eccentricity: the second has the same semi-major axis and e = 40 m / a,
    so that it circles the first on the 1 : 2 relative ellipse -- 40 m radially, 80 m along the track -- once per revolution, inside
    R = 50 m within 25.7 degrees of its perigee and apogee and outside in between.  K nodes over two revolutions from the second
    object's perigee, flown on the device; the window runs from a quarter to seven quarters of a revolution, from one along-track
    extreme to another: the nominal path enters three times.  Position sigmas 10 m, velocity sigmas 0.005 m/s: R / sigma of the
    relative position is 3.5 at the first node, inside what the window rule's sphere quadrature resolves, and the along-track drift of
    a sample is up to hundreds of metres per revolution, so that samples enter zero to three times.  (At 2 m and 0.002 m/s, R / sigma =
    18, the rule gives 1.683 where 2^20 samples give 1.937 +- 0.001: its quadrature, not its model -- profiles/collision_mc.txt.)"""
    from mpconstellation_amd import propagate_batch, _ffi
    a = 7.0e6
    n = np.sqrt(C.MU_EARTH / a ** 3)
    Tp = 2.0 * np.pi / n
    e = 40.0 / a
    s0 = np.array([a, 0.0, 0.0, 0.0, a * n, 0.0, 1.0])
    rp = a * (1.0 - e)
    s1 = np.array([rp, 0.0, 0.0, 0.0, np.sqrt(C.MU_EARTH * (2.0 / rp - 1.0 / a)), 0.0, 1.0])
    units = np.array([[a, Tp]] * 2)
    D = np.array([a] * 3 + [a / Tp] * 3 + [1.0])
    consts = scale_constants(units[:, 0])
    span = np.array([[0.0, 2.0 * Tp]] * 2)
    Y, st, _ = propagate_batch(np.stack([s0, s1]) / D, np.array([2.0, 2.0]), consts, (_ffi.CTRL_ZERO, None, 0, 1.0), K, max_step=1e-3)
    assert (st == 0).all()
    P0 = np.diag([sig_r ** 2] * 3 + [sig_v ** 2] * 3)
    return dict(pairs=np.array([[0.0, 1.0, 40.0, Tp]]), radius=np.array([20.0, 30.0]), Y=np.ascontiguousarray(Y), U=None, units=units, span=span,
                consts=consts, P0=P0, half_window=0.75 * Tp, panels=8)


EXEC = np.array([1e-4, 0.02, 1e-4, 0.01745, 1e-3])                          # test_covariance_thrust_host.py's: 2 % and 1 degree, small fixed parts


def thrust_arc(K=8):
    """covariance_thrust_reference.eccentric_arc's recipe with the device's flight in place of the oracle's: a 100 kg satellite from the
    perigee of an a = 7400 km, e = 0.1 orbit over 0.6 of its time unit, thrusting 0.02 standard_normal at K nodes, node 2 and the last
    one off; P0 = test_covariance_thrust_host.py's P0_SMALL"""
    import covariance_thrust_reference as T
    from mpconstellation_amd import propagate_batch, _ffi
    from mpconstellation_amd.satellite_scale import SatelliteScale
    A = T.ARC
    state = np.concatenate([C.eccentric_orbit(A["a"], A["e"], A["inc"], A["raan"], A["argp"]), [A["mass"]]])
    scale = SatelliteScale(x=state)
    units = np.array([[scale.units["length"], scale.units["time"]]])
    U = A["u_scale"] * np.random.default_rng(A["seed"] + K).standard_normal((3, K))
    U[:, min(2, K - 1)] = 0.0; U[:, K - 1] = 0.0
    consts = scale.get_normalized_constants().as_vector()[None]
    y0 = np.asarray(scale.normalize_state(state), dtype=np.float64)[None]
    Y, st, _ = propagate_batch(y0, [A["tf"]], consts, (_ffi.CTRL_SEQUENCE, U[None], K, 1.0), K, max_step=A["prop_max_step"])
    assert (st == 0).all()
    return dict(Y=np.ascontiguousarray(Y), U=U[None].copy(), units=units, span=np.array([[0.0, A["tf"] * units[0, 1]]]), consts=consts,
                P0=1e-2 * C.P0_TEST)
