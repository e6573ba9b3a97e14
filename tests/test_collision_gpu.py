"""Covariance propagation and collision probability on the device (csrc/collision.hip) against their numpy restatement
(collision_reference.py), against the restatement's own truths, and against closed forms.

Tolerances, from the arithmetic.  Covariance chain: the standard product bound run along the chain with gamma = 32 eps
(collision_reference.chain_error_bound), computed from the test's own inputs.  Probability: positions of 7e6 m through the same few
operations differ by about 2e-7 m (test_conjunction_gpu.py), which moves the miss by as much and the probability by its
logarithmic slope mahal / sigma_2 times that; the quadrature's 64 terms and the special functions add 1e-11 (1 + mahal^2)."""
import numpy as np
import pytest

import collision_reference as C
import conjunction_reference as R

pytestmark = pytest.mark.gpu


def scale_constants(lengths):
    from mpconstellation_amd.satellite_scale import SatelliteScale
    return np.stack([SatelliteScale(x=np.array([L, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])).get_normalized_constants().as_vector() for L in lengths])


def device_A(X, tf, consts, flags=0, max_step=1e-2):
    """the device's own A (S, K-1, 7, 7) from the existing mpcx_discretize_batch, zero thrust"""
    from mpconstellation_amd import _ffi
    X = _ffi.as_f64(X)
    S, _, K = X.shape
    U, tf, consts = np.zeros((S, 3, K)), _ffi.as_f64(tf), _ffi.as_f64(consts)
    n = S * (K - 1)
    A, Bp, Bn, Sg, xi = np.empty((S, K - 1, 7, 7)), np.empty(n * 21), np.empty(n * 21), np.empty(n * 7), np.empty(n * 7)
    st = np.zeros(S, dtype=np.int32)
    _ffi.call("mpcx_discretize_batch", _ffi.context(0), S, K, K, _ffi.dptr(X), _ffi.dptr(U), _ffi.dptr(tf), _ffi.dptr(consts), flags, max_step,
              _ffi.dptr(A), _ffi.dptr(Bp), _ffi.dptr(Bn), _ffi.dptr(Sg), _ffi.dptr(xi), _ffi.iptr(st))
    assert (st == 0).all()
    return A


def chain_case(S, K, ragged):
    """S circular LEO orbits over 2000 s at K nodes; ragged: counts between 2 and K (the first is 2), garbage behind them"""
    orb = R.random_orbits(S, seed=11 + S + K)
    Y, units, span = R.trajectories(orb, K, (10.0, 2010.0))
    ns = None
    if ragged:
        ns = np.random.default_rng(S).integers(2, K + 1, S).astype(np.int32)
        ns[0] = 2
        for s in range(S):
            Ys, _, _ = R.trajectories({k: v[s:s + 1] for k, v in orb.items()}, int(ns[s]), (10.0, 2010.0))
            Y[s] = 1e300
            Y[s, :, :ns[s]] = Ys[0]
    return Y, units, span, ns, scale_constants(units[:, 0])


def restated_chain(Y, units, span, ns, consts, P0, q, flags):
    """the restatement fed the device's own A; a ragged batch takes every count's satellites through a plain launch of that length"""
    S, _, K = Y.shape
    tf = (span[:, 1] - span[:, 0]) / units[:, 1]
    A = np.zeros((S, K - 1, 7, 7))
    counts = np.full(S, K) if ns is None else ns
    for nn in np.unique(counts):
        at = np.flatnonzero(counts == nn)
        A[at, :nn - 1] = device_A(Y[at][:, :, :nn], tf[at], consts[at], flags)
    P, status = C.covariance_chain(A, units, span, P0, q, ns)
    return A, P, status


@pytest.mark.parametrize("q", [0.0, 1e-6])
@pytest.mark.parametrize("K,ragged", [(2, False), (3, False), (30, False), (30, True)])
@pytest.mark.parametrize("S", [1, 3, 65])
def test_chain_against_the_restatement(S, K, ragged, q):
    """|P - restated| <= E entrywise, E the product bound along the chain; P symmetric to the bit; nodes past ns zero"""
    from mpconstellation_amd import covariance, _ffi
    Y, units, span, ns, consts = chain_case(S, K, ragged)
    flags = _ffi.FLAG_J2 if S == 3 else 0
    A, ref, ref_status = restated_chain(Y, units, span, ns, consts, C.P0_TEST, q, flags)
    P, status = covariance(Y, units, span, consts, C.P0_TEST, ns=ns, q=q if q else None, include_J2=S == 3, return_status=True)
    assert (status == 0).all() and (ref_status == 0).all()
    E = C.chain_error_bound(A, units, span, ref, ns)
    worst = (np.abs(P - ref) / np.where(E > 0.0, E, 1.0)).max()
    print(f"S {S} K {K} ragged {ragged} q {q}: worst |P - restated| / bound = {worst:.3f}")
    assert (np.abs(P - ref) <= E).all()
    assert np.array_equal(P, np.transpose(P, (0, 1, 3, 2)))
    assert np.array_equal(P[:, 0], np.broadcast_to(C.P0_TEST, (S, 6, 6)))
    if ns is not None:
        for s in range(S):
            assert (P[s, ns[s]:] == 0.0).all() and (P[s, ns[s] - 1] != 0.0).any()


def test_covariance_end_to_end_against_finite_difference_truth():
    """The host test's eccentric orbits, K in {2, 3, 30}, all five in one call, in metres: P at the last node against Phi~ P0 Phi~^T of
    the finite-difference transition, the same truth and the same bound as test_collision_host.py holds the oracle's chain to
    (collision_reference.CHAIN_BOUND_P = min(10 x the worst measured there, 1e-6) = 1e-6).  A wrong unit conversion is orders of magnitude away."""
    from mpconstellation_amd import covariance
    worst = 0.0
    for K in C.CHAIN_KS:
        cases = [C.orbit_case(w, K) for w in range(len(C.ORBITS))]
        X, units, span = np.stack([c["x"] for c in cases]), np.stack([c["units"] for c in cases]), np.stack([c["span"] for c in cases])
        P, status = covariance(X, units, span, np.stack([c["consts"] for c in cases]), C.P0_TEST, return_status=True)
        assert (status == 0).all()
        for c, p in zip(cases, P):
            truth = C.to_physical(c["Phi"], c["units"])
            d = C.scaled_difference(p[-1], truth @ C.P0_TEST @ truth.T, c["units"])
            worst = max(worst, d)
            assert d <= C.CHAIN_BOUND_P, (K, d)
    print(f"worst difference from the finite-difference truth: {worst:.3e} (bound {C.CHAIN_BOUND_P:.3e})")


def assert_close_to_restated(res, out, status):
    assert np.array_equal(res.status, status) and (status == 0).all()
    pc, miss, speed, s1, s2, mah = out.T
    assert (mah <= 6.0).all() and (speed >= 1.0).all()                  # what gives the bounds their meaning (R / sigma_2: the callers)
    bound = pc * (2e-7 * mah / s2 + 1e-11 * (1.0 + mah * mah))
    print(f"n {len(pc)}: worst |dpc| / bound {np.max(np.abs(res.pc - pc) / bound):.3f}, |dmiss| {np.abs(res.miss - miss).max():.2e} m")
    assert (np.abs(res.pc - pc) <= bound).all()
    assert (np.abs(res.miss - miss) <= 1e-6).all()
    assert (np.abs(res.speed - speed) <= 1e-10 * speed).all()
    assert (np.abs(res.sigma[:, 0] - s1) <= 1e-10 * s1).all() and (np.abs(res.sigma[:, 1] - s2) <= 1e-10 * s2).all()
    assert (np.abs(res.mahalanobis - mah) <= 1e-6 / s2 + 1e-10 * mah).all()


@pytest.mark.parametrize("n", [1, 63, 65, 300])
def test_probability_against_the_restatement(n):
    """catalogue form and all-pairs form of collision_reference.encounter_scene(n): times on a node (even rows) and between nodes"""
    from mpconstellation_amd import collision_probability
    sc = C.encounter_scene(n)
    Y, units, span, P, radius, _ = sc["rows"]
    R_sum = radius[sc["pairs"][:, 0].astype(int)] + sc["cat"][4]
    assert (R_sum / sc["out"][:, 4] <= 2.0).all()
    res = collision_probability(sc["pairs"], radius, Y, units, span, P, cat=sc["cat"])
    assert res.pairs is not None and np.array_equal(res.pairs, sc["pairs"])
    assert_close_to_restated(res, sc["out"], sc["status"])
    (uY, uunits, uspan, uP, uradius, uns), upairs = C.union_of(sc)
    assert_close_to_restated(collision_probability(upairs, uradius, uY, uunits, uspan, uP, ns=uns), sc["out"], sc["status"])


def result_bits(r):
    return (r.pc.tobytes(), r.miss.tobytes(), r.speed.tobytes(), r.sigma.tobytes(), r.mahalanobis.tobytes(), r.status.tobytes())


def test_both_forms_and_two_contexts_give_the_same_bits():
    """the all-pairs form of [satellites; catalogue] and the catalogue form are the same arithmetic; devices=[0, 0] deals the list's
    rows (the satellites, for covariance) to two contexts and returns the bits of one"""
    from mpconstellation_amd import collision_probability, covariance
    sc = C.encounter_scene(65)
    Y, units, span, P, radius, _ = sc["rows"]
    a = collision_probability(sc["pairs"], radius, Y, units, span, P, cat=sc["cat"])
    (uY, uunits, uspan, uP, uradius, uns), upairs = C.union_of(sc)
    b = collision_probability(upairs, uradius, uY, uunits, uspan, uP, ns=uns)
    c = collision_probability(sc["pairs"], radius, Y, units, span, P, cat=sc["cat"], devices=[0, 0])
    assert (a.status == 0).all() and result_bits(a) == result_bits(b) == result_bits(c)
    Yc, cunits, cspan, cns, consts = chain_case(65, 30, True)
    one = covariance(Yc, cunits, cspan, consts, C.P0_TEST, ns=cns, q=1e-6, return_status=True)
    two = covariance(Yc, cunits, cspan, consts, C.P0_TEST, ns=cns, q=1e-6, return_status=True, devices=[0, 0])
    assert one[0].tobytes() == two[0].tobytes() and np.array_equal(one[1], two[1]) and (one[1] == 0).all()


def test_planted_encounter_against_the_closed_form():
    """Two circular orbits (radii R0 and R0 + 300 m, planes 1.2 rad apart) cross at t_c = 1000 s, a node of both (101 nodes over
    2000 s: h_n = 20 s), the upper one exactly 300 m above the lower: the offset is radial, the relative velocity tangential, so
    300 m is the miss in the encounter plane.  Position covariances isotropic, sigma = 200 m each, no velocity uncertainty, given
    directly as P: the combined Gaussian is isotropic with sigma_c^2 = 2 sigma^2 and the probability is the non-central chi-square
    ncx2.cdf(R^2 / sigma_c^2, 2, m^2 / sigma_c^2).  screen -> collision_probability.
    Tolerance: the screen's time differs from t_c by a residual dt, |dt| < 0.1 s (asserted).  At s = |dt| / h_n < 0.005 of a node
    interval an interpolated position is off its circle by at most s^2 (1 - s)^2 h_n^4 / 24 w^4 R0 = 1.6e-6 m (nothing at dt = 0);
    across the relative velocity a residual dt moves the offset only through the curvature, w^2 m dt^2 / 2 = 2e-6 m.  So
    |miss - 300| <= 1e-5 m, which with d ln Pc / d m = m / sigma_c^2 = 3.75e-3 / m is 4e-8 relative in Pc; the carried covariance
    differs from P by (w dt)^2 = 1.2e-8 relative, and Pc moves by at most as much.  Asserted: |Pc - closed form| <= 1e-7 Pc."""
    from scipy.stats import ncx2
    from mpconstellation_amd import screen, collision_probability
    R0, m, sig, Rb = 7.0e6, 300.0, 200.0, (8.0, 12.0)
    tc, n, span = 1000.0, 101, (0.0, 2000.0)
    u = np.array([1.0, 0.0, 0.0])
    va = np.array([0.0, 1.0, 0.0]); vb = np.array([0.0, np.cos(1.2), np.sin(1.2)])
    ya, ua = C.circular_through(R0 * u, va, tc, n, span)
    yb, ub = C.circular_through((R0 + m) * u, vb, tc, n, span)
    Y, units, spans = np.stack([ya, yb]), np.stack([ua, ub]), np.array([span, span])
    P = np.zeros((2, n, 6, 6)); P[:, :, 0, 0] = P[:, :, 1, 1] = P[:, :, 2, 2] = sig * sig
    scr = screen(Y=Y, units=units, span=spans, M=401, T0=span[0], T1=span[1], threshold=1000.0)
    assert scr.pairs[:, :2].tolist() == [[0.0, 1.0]] and abs(scr.pairs[0, 3] - tc) < 0.1
    res = collision_probability(scr, np.array(Rb), Y, units, spans, P)
    sc2 = 2.0 * sig * sig
    exact = ncx2.cdf(sum(Rb) ** 2 / sc2, 2, m * m / sc2)
    print(f"tca - t_c = {scr.pairs[0, 3] - tc:.2e} s, miss {res.miss[0]:.6f} m, Pc {res.pc[0]:.9e}, closed form {exact:.9e}, "
          f"relative difference {abs(res.pc[0] - exact) / exact:.2e}")
    assert res.status.tolist() == [0] and np.array_equal(res.pairs, scr.pairs)
    assert abs(res.miss[0] - m) <= 1e-5
    assert abs(res.pc[0] - exact) <= 1e-7 * exact
    assert abs(res.sigma[0, 0] - np.sqrt(sc2)) <= 1e-5 and abs(res.sigma[0, 1] - np.sqrt(sc2)) <= 1e-5
    assert abs(res.mahalanobis[0] - m / np.sqrt(sc2)) <= 1e-5


def test_per_row_failures_leave_the_neighbours_alone():
    """a time outside a span (BADK), an index outside its side (BADK), a negative variance (NUMERIC), identical velocities (NUMERIC),
    a radius that is not a number (NUMERIC): each NaN with its status, the rows between them bit for bit what they are in a list of
    their own; the same for covariance with a non-finite P0 (NUMERIC), a count of 1 (BADK), an empty span and a negative time unit
    (BADK)"""
    from mpconstellation_amd import collision_probability, covariance
    sc = C.encounter_scene(63)
    (Y, units, span, P, radius, ns), pairs = C.union_of(sc)
    S = 5
    P = P.copy(); P[S + 7] = -P[S + 7]                                  # object 7 of the catalogue: negative variances, larger than any satellite's
    P[S + 7] *= 100.0
    good = [0, 2, 4, 6, 8]
    rows = pairs[[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]].copy()
    radius = radius.copy(); radius[S + 10] = np.nan
    rows[1, 3] = 1.0e6                                                   # outside both spans
    rows[3, 1] = len(Y)                                                  # no such object
    rows[5, 1] = rows[5, 0]                                              # a satellite against itself: no relative velocity
    rows[9, 0] = -1.0
    res = collision_probability(rows, radius, Y, units, span, P, ns=ns)
    assert res.status.tolist() == [0, C.ST_BADK, 0, C.ST_BADK, 0, C.ST_NUMERIC, 0, C.ST_NUMERIC, 0, C.ST_BADK, C.ST_NUMERIC]
    bad = res.status != 0
    for a in (res.pc, res.miss, res.speed, res.sigma[:, 0], res.sigma[:, 1], res.mahalanobis):
        assert np.isnan(a[bad]).all() and np.isfinite(a[~bad]).all()
    alone = collision_probability(rows[good], radius, Y, units, span, P, ns=ns)
    assert result_bits(alone) == tuple(np.ascontiguousarray(x[good]).tobytes() for x in
                                       (res.pc, res.miss, res.speed, res.sigma, res.mahalanobis, res.status))
    ref_out, ref_status = C.collision_probability(rows, (Y, units, span, P, radius, ns))
    assert np.array_equal(ref_status, res.status)
    # covariance
    Yc, cunits, cspan, _, consts = chain_case(5, 30, False)
    P0 = np.broadcast_to(C.P0_TEST, (5, 6, 6)).copy(); P0[1, 0, 3] = np.inf; P0[2, 5, 0] = np.nan      # (2: below the diagonal, never read)
    cns = np.array([30, 30, 30, 1, 31], dtype=np.int32)
    sp = cspan.copy()
    Pc, st = covariance(Yc, cunits, sp, consts, P0, ns=cns, return_status=True)
    assert st.tolist() == [0, C.ST_NUMERIC, 0, C.ST_BADK, C.ST_BADK]
    assert np.isnan(Pc[[1, 3, 4]]).all() and np.isfinite(Pc[[0, 2]]).all()
    Pa, sta = covariance(Yc[[0, 2]], cunits[[0, 2]], sp[[0, 2]], consts[[0, 2]], C.P0_TEST, return_status=True)
    assert (sta == 0).all() and np.array_equal(Pa, Pc[[0, 2]])
    sp[0] = (5.0, 5.0)                                                   # an empty span
    bad_units = cunits.copy(); bad_units[1, 1] = -bad_units[1, 1]        # a negative time unit: no positive tf to linearise over
    Pb, st = covariance(Yc, bad_units, sp, consts, C.P0_TEST, return_status=True)
    assert st.tolist() == [C.ST_BADK, C.ST_BADK, 0, 0, 0] and np.isnan(Pb[:2]).all() and np.array_equal(Pb[2], Pc[2])


def test_c_abi_refuses_bad_sizes():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    S, K, n = 2, 5, 3
    Y, units, span, consts = np.zeros((S, 7, K)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S), np.ones((S, 8))
    P0, P, st = np.zeros((S, 6, 6)), np.zeros((S, K, 6, 6)), np.zeros(S, dtype=np.int32)
    d, i = _ffi.dptr, _ffi.iptr

    def cov(S=S, K=K, flags=0, max_step=1e-2):
        return lib.mpcx_covariance_batch(ctx, S, K, None, d(Y), None, d(units), d(span), d(consts), flags, max_step, d(P0), None, d(P), i(st))
    for bad in (dict(S=0), dict(K=1), dict(max_step=0.0), dict(flags=4), dict(flags=_ffi.FLAG_ATMO)):
        assert cov(**bad) == -2, bad
        assert b"covariance" in lib.mpcx_last_error(ctx) or b"ATMO" in lib.mpcx_last_error(ctx)
    w = lib.mpcx_covariance_workspace_bytes
    assert w(0, 5) == 0 and w(2, 1) == 0 and w(2, 5) >= 2 * 4 * _ffi.STAGE_DOUBLES * 8
    pairs, radius = np.zeros((n, 4)), np.ones(S)
    out, pst = np.zeros((n, _ffi.NPC)), np.zeros(n, dtype=np.int32)
    row = lambda S, K: (S, K, None, d(Y), d(units), d(span), d(P), d(radius))
    none = (0, 0, None, None, None, None, None, None)

    def pc(n=n, rows=None, cols=none, mu=C.MU_EARTH):
        return lib.mpcx_collision_probability(ctx, n, d(pairs), *(rows or row(S, K)), *cols, mu, d(out), i(pst))
    for bad in (dict(n=0), dict(rows=row(0, K)), dict(rows=row(S, 1)), dict(mu=0.0), dict(mu=-1.0), dict(cols=row(0, K)), dict(cols=row(S, 1)),
                dict(cols=(S, K, None, d(Y), d(units), d(span), None, d(radius)))):
        assert pc(**bad) == -2, bad
        assert b"collision_probability" in lib.mpcx_last_error(ctx)
    assert pc() == 0 and (pst == C.ST_NUMERIC).all() and np.isnan(out).all()          # (all zeros: no relative velocity anywhere)


def test_constellation_mpc_collision_probability():
    """Three satellites, one update; satellite 0's planned positions are moved so that it passes 500 m from satellite 1, across the
    relative motion, at an instant of the screen's common grid (as test_conjunction_gpu.py plants one in the flown segments: the screen's
    ephemeris at a grid instant is the cubic Hermite on the nodes that plants the offset here, so that end of a grid interval is exactly
    500 m apart and the listed distance cannot be larger; between grid instants the screen interpolates a second time).
    ConstellationMPC.collision_probability lists exactly that pair and returns, bit for bit, what the module-level calls return on
    the plan: screen, covariance along (plan X, plan U, plan_tf, plan_K), collision_probability."""
    from mpconstellation_amd import Satellite, ConstellationMPC, conjunction as cj
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(3)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5)
    mpc.update()
    (w,) = mpc._screen_windows("plan", samples_per_node=4)
    a, b = 0, 1
    X = mpc._plan[0]
    m = w["M"] // 3
    tb = w["T0"] + m * ((w["T1"] - w["T0"]) / (w["M"] - 1))               # the grid's instant m, as the screen computes it
    assert 0 < m < w["M"] - 1
    side = (X, w["units"], w["span"], np.zeros((3, X.shape[2], 6, 6)), np.zeros(3), w["ns"])
    _, pa, va, _, _ = C.state_and_cov_at(side, a, tb, C.MU_EARTH)
    _, pb, vb, _, _ = C.state_and_cov_at(side, b, tb, C.MU_EARTH)
    rel = vb - va
    e = np.cross(rel, [0.0, 0.0, 1.0]); e /= np.linalg.norm(e)
    assert np.linalg.norm(rel) >= 1.0
    X[a, 0:3, :] += ((pb - pa + 500.0 * e) / w["units"][a, 0])[:, None]
    P0 = np.diag([100.0 ** 2] * 3 + [0.1 ** 2] * 3)
    scr, col = mpc.collision_probability(1000.0, P0, 5.0, q=1e-8)
    print("planted pair:", scr.pairs, "Pc", col.pc, "miss", col.miss, "sigma", col.sigma)
    assert scr.n_pairs_total == 1 and scr.pairs[:, :2].tolist() == [[a, b]] and 400.0 < scr.pairs[0, 2] <= 500.001
    assert col.status.tolist() == [0] and 0.0 < col.pc[0] < 1.0 and abs(col.miss[0] - scr.pairs[0, 2]) < 1.0
    scr2 = cj.screen(threshold=1000.0, **w)
    P, pst = cj.covariance(X, w["units"], w["span"], mpc.consts, P0, U=mpc._plan[1], ns=w["ns"], q=1e-8, return_status=True)
    col2 = cj.collision_probability(scr2, 5.0, X, w["units"], w["span"], P, ns=w["ns"])
    assert (pst == 0).all() and scr.pairs.tobytes() == scr2.pairs.tobytes() and result_bits(col) == result_bits(col2)


def test_catalogue_covariance_is_trajectories_then_covariance():
    """catalogue_covariance pairs every object with the constants of ITS OWN scale: the same bits as catalogue_trajectories followed by
    covariance with constants built here from the units it returns, and not those of constants shifted by one object"""
    from mpconstellation_amd import catalogue_covariance, catalogue_trajectories, covariance
    orb = R.random_orbits(4, seed=21, r_lo=6.8e6, r_hi=9.0e6)
    p, v = R.kepler_state(orb, np.zeros(4))
    T0, T1, n, q = 100.0, 2100.0, 25, np.array([1e-8, 0.0, 2e-8, 1e-9])
    Y, units, span, P = catalogue_covariance(p, v, C.P0_TEST, T0, T1, n, q=q)
    Y2, units2, span2 = catalogue_trajectories(p, v, T0, T1, n)
    assert np.array_equal(Y, Y2) and np.array_equal(units, units2) and np.array_equal(span, span2)
    assert np.array_equal(units[:, 0], np.linalg.norm(p, axis=1))
    consts = scale_constants(units[:, 0])
    P2, st = covariance(Y, units, span, consts, C.P0_TEST, q=q, include_J2=True, return_status=True)
    assert (st == 0).all() and np.isfinite(P).all() and P.shape == (4, n, 6, 6) and np.array_equal(P, P2)
    assert not np.array_equal(P, covariance(Y, units, span, np.roll(consts, 1, axis=0), C.P0_TEST, q=q, include_J2=True))
    assert not np.array_equal(P, covariance(Y, units, span, consts, C.P0_TEST, q=q, include_J2=False))


def test_constellation_mpc_collision_probability_against_a_catalogue_under_the_planning_model():
    """ConstellationMPC(plan_drag, plan_J2, atmosphere) and catalogue=: one foreign object on a circular orbit that passes 500 m from
    satellite 0's plan at an instant of the screen's grid (its position there is the node Hermite's, so the listed distance cannot be
    larger).  The method returns, bit for bit, screen_against, covariance under the planning model's flags and atmosphere, and
    collision_probability with cat= on the plan; the covariance without those flags is a different one, so the forwarding counts."""
    from mpconstellation_amd import Satellite, ConstellationMPC, Atmosphere, conjunction as cj
    from mpconstellation_amd.constellation import constellation_states
    atm = Atmosphere.power_law()
    st = constellation_states(3)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5,
                           plan_drag=True, plan_J2=True, atmosphere=atm)
    mpc.update()
    (w,) = mpc._screen_windows("plan", samples_per_node=4)
    X, U = mpc._plan[0], mpc._plan[1]
    m = w["M"] // 3
    tb = w["T0"] + m * ((w["T1"] - w["T0"]) / (w["M"] - 1))
    side = (X, w["units"], w["span"], np.zeros((3, X.shape[2], 6, 6)), np.zeros(3), w["ns"])
    _, pa, va, _, _ = C.state_and_cov_at(side, 0, tb, C.MU_EARTH)
    qh = pa / np.linalg.norm(pa)
    vh = va - (va @ qh) * qh; vh /= np.linalg.norm(vh)
    vhat = np.cos(1.0) * vh + np.sin(1.0) * np.cross(qh, vh)            # crossing at 1 rad
    n, cspan = 31, np.array([[w["T0"], w["T1"]]])
    h = (cspan[0, 1] - cspan[0, 0]) / (n - 1)
    # a node of the object at the grid instant: move its span so that tb falls on node 10 (the span still covers the grid's middle)
    cspan = cspan + (tb - (cspan[0, 0] + 10 * h))
    cy, cu = C.circular_through(pa + 500.0 * qh, vhat, tb, n, cspan[0])
    cat = (cy[None], cu[None], cspan, C.random_covariances(np.random.default_rng(5), 1, n), np.array([3.0]))
    P0 = np.diag([100.0 ** 2] * 3 + [0.1 ** 2] * 3)
    scr, col = mpc.collision_probability(1000.0, P0, 5.0, q=1e-8, catalogue=cat)
    print("planted pair:", scr.pairs, "Pc", col.pc, "miss", col.miss, "sigma", col.sigma)
    assert scr.n_pairs_total == 1 and scr.pairs[:, :2].tolist() == [[0, 0]] and 400.0 < scr.pairs[0, 2] <= 500.001
    assert col.status.tolist() == [0] and 0.0 < col.pc[0] < 1.0 and abs(col.miss[0] - scr.pairs[0, 2]) < 1.0
    scr2 = cj.screen_against(threshold=1000.0, cat_Y=cat[0], cat_units=cat[1], cat_span=cat[2], **w)
    model = dict(U=U, ns=w["ns"], q=1e-8, return_status=True)
    P, pst = cj.covariance(X, w["units"], w["span"], mpc.consts, P0, include_drag=True, include_J2=True, atmosphere=atm, **model)
    col2 = cj.collision_probability(scr2, 5.0, X, w["units"], w["span"], P, ns=w["ns"], cat=cat)
    assert (pst == 0).all() and scr.pairs.tobytes() == scr2.pairs.tobytes() and result_bits(col) == result_bits(col2)
    for other in (dict(), dict(include_J2=True), dict(include_drag=True, include_J2=True)):
        P_other, _ = cj.covariance(X, w["units"], w["span"], mpc.consts, P0, **other, **model)
        assert not np.array_equal(P_other, P), other
