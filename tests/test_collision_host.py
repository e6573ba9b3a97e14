"""Collision probability without a device: the numpy restatement (collision_reference) against independent truths -- the chain of
the oracle's transition matrices against a finite-difference transition of a tightly integrated two-body flow, the quadrature
against scipy's adaptive double integral and the non-central chi-square, the short-arc block against the same finite differences --
and the wrappers' argument checks."""
import numpy as np
import pytest

import collision_reference as C
import oracle_lib as O
from mpconstellation_amd import conjunction as cj

CHAIN_KS = C.CHAIN_KS
CHAIN_BOUND_PHI, CHAIN_BOUND_P = C.CHAIN_BOUND_PHI, C.CHAIN_BOUND_P


def oracle_chain(which, K):
    c = C.orbit_case(which, K)
    d = O.discretize(c["x"], np.zeros((3, K)), c["tf"], c["consts"], flags=0, max_step=1e-2)
    assert d["status"] == 0
    P, status = C.covariance_chain(d["A"][None], c["units"][None], c["span"][None], C.P0_TEST)
    assert status.tolist() == [0]
    return c, d["A"], P[0]


def test_mass_row_of_A_is_zero_in_position_and_velocity():
    """what makes the 6 x 6 chain exact: the 7 x 7 chain restricted to position and velocity is the chain of the 6 x 6 blocks"""
    _, A, _ = oracle_chain(0, 30)
    assert np.abs(A[:, 6, :6]).max() == 0.0


def test_restated_chain_against_finite_difference_truth():
    """Eccentric inclined two-body orbits (e = 0.01 .. 0.15, five of them) over one revolution, K in {2, 3, 30} nodes, A from the CPU
    oracle at the default max_step: P_K of the restated chain from P0_TEST against Phi~ P0 Phi~^T with Phi~ the fourth-order
    central-difference transition of a flow integrated to 1e-13, and the product of the 6 x 6 blocks against that transition
    itself, both as relative Frobenius differences.  Measured when written: transition worst 1.52e-7 (orbit 3, e = 0.15,
    K = 3), covariance worst 1.74e-7 (same case); the same at every K to a factor of two: the discretiser integrates at rtol 1e-3
    with max_step 1e-2, and that step limit, not the chain, sets the difference (it grows with the eccentricity: 1e-8 at e = 0.04).
    Asserted: the measured worst values against min(10 x the recorded worst, 1e-6) = 1e-6 for both: the factor covers adaptive
    steps landing differently elsewhere, the cap is where noise ends and a units or indexing error begins."""
    worst_p = worst_phi = 0.0
    for which in range(len(C.ORBITS)):
        for K in CHAIN_KS:
            c, A, P = oracle_chain(which, K)
            truth = C.to_physical(c["Phi"], c["units"])
            dp = C.scaled_difference(P[-1], truth @ C.P0_TEST @ truth.T, c["units"])
            prod = np.eye(6)
            for k in range(K - 1):
                prod = A[k][:6, :6] @ prod
            dphi = np.linalg.norm(prod - c["Phi"]) / np.linalg.norm(c["Phi"])
            print(f"orbit {which} K {K}: covariance {dp:.2e} transition {dphi:.2e}")
            worst_p, worst_phi = max(worst_p, dp), max(worst_phi, dphi)
            assert np.array_equal(P, np.transpose(P, (0, 2, 1)))
    print(f"worst: covariance {worst_p:.3e} transition {worst_phi:.3e}")
    assert CHAIN_BOUND_PHI <= 1e-6 and CHAIN_BOUND_P <= 1e-6
    assert worst_phi <= CHAIN_BOUND_PHI and worst_p <= CHAIN_BOUND_P


def test_chain_noise_term_and_ragged_counts():
    """q Q(h) against the closed form for a free particle (Phi = [[I, h I], [0, I]]): after n steps of h the noise is q Q(n h);
    nodes past ns are zero, a count of 1, an empty span and a non-finite P0 are NaN with their status"""
    K, h, q = 5, 7.0, 0.3
    A = np.zeros((4, K - 1, 7, 7))
    A[:] = np.eye(7)
    A[:, :, 0:3, 3:6] = np.eye(3) * 0.25                                  # normalised step 1/4 of a span of one time unit
    units = np.tile([1000.0, h * (K - 1)], (4, 1))
    span = np.array([[0.0, h * (K - 1)], [0.0, h * 2], [5.0, 5.0], [0.0, h * (K - 1)]])
    P0 = np.zeros((4, 6, 6)); P0[3, 2, 2] = np.inf
    P, status = C.covariance_chain(A, units, span, P0, q=q, ns=[K, 3, K, K])
    assert status.tolist() == [0, 0, C.ST_BADK, C.ST_NUMERIC]
    assert np.allclose(P[0, -1], q * C.q_matrix(h * (K - 1)), rtol=1e-13, atol=0.0)
    assert np.isnan(P[2]).all() and np.isnan(P[3]).all() and (P[1, 3:] == 0.0).all() and (P[1, 2] != 0.0).any()
    _, st = C.covariance_chain(A, units, span, np.zeros((6, 6)), ns=[K, 1, K, K + 1])
    assert st.tolist() == [0, C.ST_BADK, C.ST_BADK, C.ST_BADK]
    for Tu in (-28.0, 0.0, np.inf, np.nan):                             # a time unit that gives no positive finite tf
        bad_units = units.copy(); bad_units[0, 1] = Tu
        Pb, st = C.covariance_chain(A, bad_units, span, np.zeros((6, 6)), ns=[K, 3, K, K])
        assert st.tolist() == [C.ST_BADK, 0, C.ST_BADK, 0] and np.isnan(Pb[0]).all()


def dblquad_disc(xm, ym, s1, s2, R):
    """the same integral by scipy's adaptive double quadrature, in polar coordinates about the disc's centre"""
    from scipy.integrate import dblquad

    def f(th, r):
        x, y = r * np.cos(th), r * np.sin(th)
        return r * np.exp(-0.5 * (((x - xm) / s1) ** 2 + ((y - ym) / s2) ** 2)) / (2.0 * np.pi * s1 * s2)
    val, _ = dblquad(f, 0.0, R, 0.0, 2.0 * np.pi, epsabs=1e-300, epsrel=1e-12)
    return val


def quadrature_cases():
    """40 random encounters: R / sigma_2 log-uniform in [0.02, 2], axis ratio in [1, 10], Mahalanobis distance in [0, 5], any
    direction; every fourth one isotropic"""
    rng = np.random.default_rng(20)
    out = []
    for n in range(40):
        s2 = 10.0 ** rng.uniform(0.5, 3.0)
        s1 = s2 * (1.0 if n % 4 == 0 else rng.uniform(1.0, 10.0))
        R = s2 * 10.0 ** rng.uniform(np.log10(0.02), np.log10(2.0))
        mah, ang = rng.uniform(0.0, 5.0), rng.uniform(0.0, 2.0 * np.pi)
        out.append((mah * s1 * np.cos(ang), mah * s2 * np.sin(ang), s1, s2, R))
    return out


def test_restated_probability_against_adaptive_double_integral():
    """40 random cases (R / sigma_2 <= 2, axis ratio <= 10, Mahalanobis distance <= 5) against scipy.integrate.dblquad at epsrel
    1e-12, whose own tolerance sets the bound 1e-10 relative; the isotropic ones also against the non-central chi-square
    distribution ncx2.cdf(R^2 / sigma^2, 2, m^2 / sigma^2).  Measured when written: worst 3.5e-15 against dblquad, worst
    1.8e-15 against ncx2."""
    import warnings
    from scipy.stats import ncx2
    worst = worst_iso = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # (dblquad reports that epsabs = 1e-300 is not reached)
        for xm, ym, s1, s2, R in quadrature_cases():
            assert R / s2 <= 2.0 and s1 / s2 <= 10.0 and np.hypot(xm / s1, ym / s2) <= 5.0
            pc = C.disc_probability(xm, ym, s1, s2, R)
            ref = dblquad_disc(xm, ym, s1, s2, R)
            err = abs(pc - ref) / ref
            worst = max(worst, err)
            if s1 == s2:
                iso = ncx2.cdf(R * R / (s1 * s1), 2, (xm * xm + ym * ym) / (s1 * s1))
                worst_iso = max(worst_iso, abs(pc - iso) / iso)
                assert abs(pc - iso) <= 1e-10 * iso, (xm, ym, s1, s2, R, pc, iso)
            assert err <= 1e-10, (xm, ym, s1, s2, R, pc, ref)
    print(f"worst relative error: dblquad {worst:.2e}, ncx2 {worst_iso:.2e}")


def test_probability_edges():
    assert C.disc_probability(10.0, 5.0, 100.0, 50.0, 0.0) == 0.0 and C.disc_probability(10.0, 5.0, 100.0, 50.0, -1.0) == 0.0
    assert abs(C.disc_probability(0.0, 0.0, 1.0, 1.0, 1.0) - (1.0 - np.exp(-0.5))) <= 1e-15        # Rayleigh
    # the miss along the larger axis and along the smaller one are different numbers, and the frame's angle decides which
    pa, va, pb = np.zeros(3), np.zeros(3), np.array([0.0, 300.0, 0.0])
    Ca, Cb = np.diag([1.0, 400.0 ** 2, 100.0 ** 2]), np.zeros((3, 3))
    st, o = C.encounter(pa, va, Ca, pb, np.array([7000.0, 0.0, 0.0]), Cb, 20.0)
    assert st == 0 and abs(o[1] - 300.0) < 1e-9 and abs(o[3] - 400.0) < 1e-9 and abs(o[4] - 100.0) < 1e-9 and abs(o[5] - 0.75) < 1e-12
    assert abs(o[0] - C.disc_probability(300.0, 0.0, 400.0, 100.0, 20.0)) <= 1e-15 * o[0]
    st, o = C.encounter(pa, va, Ca, pb, np.zeros(3), Cb, 20.0)
    assert st == C.ST_NUMERIC and np.isnan(o).all()
    for R in (np.nan, np.inf):                                           # a radius that is not finite is no probability at all
        st, o = C.encounter(pa, va, Ca, pb, np.array([7000.0, 0.0, 0.0]), Cb, R)
        assert st == C.ST_NUMERIC and np.isnan(o).all()
    st, o = C.encounter(pa, va, Ca, np.zeros(3), np.array([0.0, 0.0, 7000.0]), Cb, 20.0)      # zero miss: e_1 from the x axis
    assert st == 0 and o[1] == 0.0 and abs(o[3] - 400.0) < 1e-9 and abs(o[4] - 1.0) < 1e-12


@pytest.mark.parametrize("nodes", [31, 101])
def test_short_arc_block_against_finite_difference_truth(nodes):
    """Phi_r at dt = half a node interval of `nodes` nodes per revolution against the position rows of the finite-difference
    transition over dt, relative Frobenius difference with the velocity columns in units of the mean motion (Phi_r's two blocks
    are then both of order one): <= (n dt)^3, the order of the first neglected term.  Measured when written (worst orbit, e = 0.15; from perigee, where
    the gradient is largest): 1.04e-3 at n dt = 0.105 where (n dt)^3 is 1.15e-3, 2.8e-5 at 0.031 where it is 3.1e-5; 5.7e-4 and
    1.6e-5 at e = 0.04."""
    for which in range(len(C.ORBITS)):
        c = C.orbit_case(which, 30)
        L, Tu = c["units"]
        dt_n = 0.5 / (nodes - 1)                                          # in periods
        ndt = 2.0 * np.pi * dt_n
        truth = C.to_physical(C.fd_transition(c["y0"], dt_n), c["units"])[0:3]
        state = c["y0"][0:3] * L
        F = C.short_arc_rows(state, dt_n * Tu, C.MU_EARTH)
        n = 2.0 * np.pi / Tu
        w = np.array([1.0] * 3 + [n] * 3)
        err = np.linalg.norm((F - truth) * w) / np.linalg.norm(truth * w)
        print(f"orbit {which} nodes {nodes}: n dt = {ndt:.3f}, error {err:.2e}, (n dt)^3 = {ndt ** 3:.2e}")
        assert err <= ndt ** 3


def test_wrapper_argument_checks_and_the_empty_list():
    """every bad argument is a ValueError before the library (which needs a device) is touched; an empty list never reaches it"""
    S, n = 2, 5
    Y, units, span = np.zeros((S, 7, n)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S)
    consts, P0, P = np.ones((S, 8)), np.eye(6), np.zeros((S, n, 6, 6))
    good = dict(Y=Y, units=units, span=span, consts=consts, P0=P0)
    bad_cov = [dict(Y=np.zeros((S, 6, n))), dict(Y=np.zeros((S, 7, 1))), dict(units=np.ones((3, 2))), dict(span=np.ones((S, 3))),
               dict(consts=np.ones((S, 7))), dict(P0=np.eye(5)), dict(P0=np.zeros((3, 6, 6))), dict(U=np.zeros((S, 3, n + 1))),
               dict(ns=[5, 5, 5]), dict(q=[1.0, 2.0, 3.0]), dict(q=-1.0), dict(max_step=0.0)]
    for kw in bad_cov:
        with pytest.raises(ValueError):
            cj.covariance(**{**good, **kw})
    pairs = np.array([[0.0, 1.0, 100.0, 0.5]])
    good = dict(pairs=pairs, radius=5.0, Y=Y, units=units, span=span, P=P)
    cat = (Y, units, span, P, 1.0)
    bad_pc = [dict(pairs=np.zeros((1, 3))), dict(pairs=np.zeros(4)), dict(radius=[1.0, 2.0, 3.0]), dict(P=np.zeros((S, n, 6, 5))),
              dict(P=np.zeros((S, n + 1, 6, 6))), dict(Y=np.zeros((S, 7, 1)), P=np.zeros((S, 1, 6, 6))), dict(mu=0.0), dict(ns=[5]),
              dict(cat=(Y, units, span, P)), dict(cat=(Y, units, span, np.zeros((S, n, 6)), 1.0)), dict(cat=(Y, units, np.ones((S, 3)), P, 1.0)),
              dict(cat=(Y, units, span, P, [1.0, 2.0, 3.0]))]
    for kw in bad_pc:
        with pytest.raises(ValueError):
            cj.collision_probability(**{**good, **kw})
    with pytest.raises(ValueError, match=r"cat_P.*\(2, 5, 6, 6\)"):
        cj.collision_probability(**{**good, "cat": (Y, units, span, np.zeros((S, n, 6)), 1.0)})
    for kw in (dict(), dict(cat=cat), dict(devices=[0, 0])):
        r = cj.collision_probability(**{**good, "pairs": np.zeros((0, 4)), **kw})
        assert isinstance(r, cj.CollisionResult)
        assert r.pc.shape == r.miss.shape == r.speed.shape == r.mahalanobis.shape == r.status.shape == (0,)
        assert r.sigma.shape == (0, 2) and r.pairs.shape == (0, 4) and r.status.dtype == np.int32
    empty = cj.ConjunctionResult(np.zeros(S), np.zeros(S, dtype=np.int32), np.zeros(S), cj.sort_pairs([]), 0)
    assert len(cj.collision_probability(**{**good, "pairs": empty}).pc) == 0


def test_constellation_collision_probability_needs_a_plan():
    from test_conjunction_host import hand_made_mpc
    mpc, _ = hand_made_mpc()
    with pytest.raises(ValueError, match="no plan"):
        mpc.collision_probability(1000.0, np.eye(6), 5.0)
