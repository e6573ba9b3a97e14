"""Inputs of the rollout comparisons where max_step does not clip the steps: the one list that tests/test_rollout_unclipped_host.py
(the oracle against scipy's solve_ivp) and tests/test_rollout_unclipped_gpu.py (propagate_kernel against the oracle) share, with
the oracle's results for them, its step and attempt counts, and the tolerance each case is held to.

The tolerance is measured on the oracle, never on what is compared with it.  kappa is the oracle's own amplification of a
relative change of 1e-10 in y0 (eight seeded draws, the step counts unchanged under them); the two sides evaluate the same
right-hand side with other roundings (reciprocals and rsqrt by Newton steps, sums in another order): at most `ulps` units in the last
place per evaluation, six evaluations per attempted step, each amplified by at most kappa:

    tol = ulps 2^-52 6 (accepted + rejected) kappa max(1, |y|_inf)         ulps = 4 for the device, 2 for scipy

per case: the largest kappa, attempt count and |y| of its satellites (case_tolerance says why).

Two conditions keep that bound from hiding a failure (case_tolerance): it is below 1e-8, and it is at least 1e3 times smaller
than what the oracle's output moves by when its steps are clipped at a twentieth of the case's max_step -- a flight on
another step sequence cannot pass.  (A max_step above the interval's length, inf included, clips nothing the length does not:
its twentieth is taken of the length 1.  A flight with one output point returns its start state and is held to it exactly.)  Everything is deterministic (seeded) and computed once per process."""
import functools

import numpy as np

import drag_cases as D
import oracle_lib as O

# normalised constants of tests/test_discretize_step_factor_gpu.py (MU = 4 pi^2: one orbit of radius 1 per unit of tf)
CST = np.array([39.47841760435743, 0.92, 1.08262668E-3, 46.5, 0.0873, 1e-12, 6.9e6, 3.7e-17])
DRAG, J2 = O.FLAG_DRAG, O.FLAG_J2
DJ = DRAG | J2
END_TAUS = (1.0, 0.6, 0.37)
KU = 5
EPS = 2.0 ** -52
DEVICE_ULPS, SCIPY_ULPS = 4, 2
KAPPA_REL, KAPPA_DRAWS = 1e-10, 8
EDGE_REL, EDGE_DRAWS = 1e-13, 8


def orbit_y0(e, nu, inc=0.4):
    """normalised state at true anomaly nu of the orbit with perigee radius 1 and eccentricity e, inclined by inc (J2 sees z)"""
    p = 1.0 + e
    r = p / (1.0 + e * np.cos(nu))
    h = np.sqrt(CST[0] * p)
    rv = np.array([r * np.cos(nu), r * np.sin(nu), 0.0]), CST[0] / h * np.array([-np.sin(nu), e + np.cos(nu), 0.0])
    c, s = np.cos(inc), np.sin(inc)
    R = np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    return np.concatenate([R @ rv[0], R @ rv[1], [1.0]])


def make_case(name, law, y0, tf, max_step, n_eval, flags=DJ, atmosphere=None, **params):
    """law: one of drag_cases.LAWS; params: table (S,3,Ku) and end_tau (S,), constant (S,3) or tangential (S,);
    n_eval: an int or per-satellite counts (S,)"""
    y0 = np.atleast_2d(np.asarray(y0, dtype=np.float64))
    S = y0.shape[0]
    c = dict(name=name, law=law, y0=y0, tf=np.broadcast_to(np.asarray(tf, dtype=np.float64), (S,)).copy(), S=S, max_step=float(max_step),
             n_eval=n_eval, flags=flags, atmosphere=atmosphere, const=np.tile(CST, (S, 1)), _ref={})
    c.update(params)
    return c


def n_eval_of(case, s):
    return int(case["n_eval"] if np.ndim(case["n_eval"]) == 0 else case["n_eval"][s])


def oracle_ctrl(case, s):
    law = case["law"]
    if law == "zero":
        return O.make_ctrl(O.CTRL_ZERO)
    if law == "constant":
        return O.make_ctrl(O.CTRL_CONSTANT, case["constant"][s])
    if law == "tangential":
        return O.make_ctrl(O.CTRL_TANGENTIAL, (case["tangential"][s], 0, 0))
    return O.make_ctrl(O.CTRL_SEQUENCE, useq=case["table"][s], end_tau=case["end_tau"][s])


def oracle_flight(case, s, y0=None, max_step=None):
    """-> (y (7, n_eval), status, accepted steps, rejected attempts, nfev) of satellite s"""
    return O.propagate_counts(case["y0"][s] if y0 is None else y0, float(case["tf"][s]), case["const"][s], oracle_ctrl(case, s), n_eval_of(case, s),
                              case["flags"], max_step=case["max_step"] if max_step is None else max_step, atmosphere=case["atmosphere"])


def _moved(case, s, rel, draws, seed):
    """the oracle's flights from y0 (1 + rel d), d standard normal: seeded per satellite"""
    rng = np.random.default_rng([seed, s])
    return [oracle_flight(case, s, case["y0"][s] * (1.0 + rel * rng.standard_normal(7))) for _ in range(draws)]


def reference(case):
    """per satellite: dict(y, accepted, rejected, nfev, kappa, gap, counts_stable); computed once per case.
    counts_stable: the step and attempt counts are those of every draw at 1e-13 (no acceptance knife edge) and at 1e-10 (kappa is
    the amplification of one step sequence); gap: |y - y(max_step / 20)|_inf"""
    ref = case["_ref"]
    if not ref:
        out = []
        for s in range(case["S"]):
            y, rc, acc, rej, nfev = oracle_flight(case, s)
            assert rc == 0, (case["name"], s, rc)
            wide = _moved(case, s, KAPPA_REL, KAPPA_DRAWS, 1)
            edge = _moved(case, s, EDGE_REL, EDGE_DRAWS, 2)
            stable = all(m[1] == 0 and m[2:4] == (acc, rej) for m in wide + edge)
            kappa = max(np.abs(m[0] - y).max() for m in wide) / KAPPA_REL
            fine = oracle_flight(case, s, max_step=min(case["max_step"], 1.0) / 20)
            assert fine[1] == 0
            out.append(dict(y=y, accepted=acc, rejected=rej, nfev=nfev, kappa=kappa, gap=np.abs(fine[0] - y).max(), counts_stable=stable))
        ref["sats"] = out
    return ref["sats"]


def own_bound(r, ulps):
    """the bound from one satellite's own counts and amplification: for the record only (see case_tolerance)"""
    return ulps * EPS * 6 * (r["accepted"] + r["rejected"]) * r["kappa"] * max(1.0, np.abs(r["y"]).max())


def case_tolerance(case, ulps):
    """the bound of a case, after the conditions that keep it meaningful: kappa, the attempts and |y| are the largest of the case's
    satellites.  A satellite with one output point is left out of it: that point is tau = 0, the interpolant of the first step
    at x = 0, h 0 + y0 -- the start state itself on any step sequence, and held to it exactly (tolerance_of: 0).

    One bound per case, not one per satellite: a short flight's own figure (own_bound; three steps, kappa 40: 4e-12) is below what
    rounding does to it.  The error norm of a small step is a sum over the stages that cancels to 1e-5 .. 1e-3 of its terms, so an
    ulp in a stage is 1e-13 .. 1e-11 of the norm and a fifth of that of the next step's length, and the samples follow the step
    lengths about one to one -- a channel kappa, which moves y0 smoothly, does not see.  scipy and the oracle, the same arithmetic
    in another order, differ by up to seven times such a figure on the mixed waves (test_rollout_unclipped_host.py prints them),
    the device and the oracle by up to 4.7 times; against the case's bound that is 0.11 and 0.028
    (profiles/rollout_unclipped.txt)."""
    ref = reference(case)
    for s, r in enumerate(ref):
        assert r["counts_stable"], (case["name"], s, "step counts move with y0: an acceptance knife edge")
        if n_eval_of(case, s) == 1:
            assert np.array_equal(r["y"][:, 0], case["y0"][s])
    many = [r for s, r in enumerate(ref) if n_eval_of(case, s) > 1]
    if not many:
        return 0.0
    tol = (ulps * EPS * 6 * max(r["accepted"] + r["rejected"] for r in many) * max(r["kappa"] for r in many)
           * max(1.0, max(np.abs(r["y"]).max() for r in many)))
    assert 0.0 < tol < 1e-8, (case["name"], tol)
    assert 1e3 * tol <= min(r["gap"] for r in many), (case["name"], tol, [r["gap"] for r in many])
    return tol


def tolerance_of(case, s, tol):
    return tol if n_eval_of(case, s) > 1 else 0.0


def counts(case):
    r = reference(case)
    return np.array([x["accepted"] for x in r]), np.array([x["rejected"] for x in r])


# (a) mixed waves: S = 21 sequence flights (one full wave of 16 quads and five live quads in the next), tables ~ N(0, 0.8^2) of five
# columns, end_tau and tf cycling, start states on orbits of eccentricity 0 .. 0.6 at different phases
MIXED_S, MIXED_SEED, MIXED_TFS = 21, 1, (0.4, 1.0, 2.0, 3.0)


@functools.lru_cache(None)
def mixed_waves(max_step=1.0, seed=MIXED_SEED):
    S = MIXED_S
    rng = np.random.default_rng(seed)
    y0 = np.array([orbit_y0(0.6 * s / (S - 1), 2.4 * s) for s in range(S)])
    return make_case(f"mixed waves, max_step {max_step:g}", "sequence", y0, [MIXED_TFS[s % 4] for s in range(S)], max_step, 9,
                     table=rng.normal(size=(S, 3, KU)) * 0.8, end_tau=np.array([END_TAUS[s % 3] for s in range(S)]))


def check_mixed_waves(case):
    """the conditions of (a) on the oracle's counts: the flights do take the paths the case is there for"""
    acc, rej = counts(case)
    assert (rej > 0).sum() >= 6 and (rej == 0).sum() >= 3, rej
    assert (rej[:16] > 0).any() and (rej[:16] == 0).any(), rej
    assert acc[:16].max() >= 2 * acc[:16].min(), acc
    assert all(r["counts_stable"] for r in reference(case))
    return acc, rej


# (f) a failing satellite among the mixed waves: this quad of the first wave starts from a NaN velocity component
BAD_SAT, BAD_COMPONENT = 5, 4

# (b) many output points per step: three sequence flights, tf = 1e-4 (two steps: every output point in one or the other, and the
# tables of satellite 1 and 2 end inside one) and tf = 0.5 (40 points in at most eight steps)
Y0_POLAR = np.array([1.0, 0, 0, 0, 0, 2 * np.pi * 1.1, 1.0])
SHORT_SEED = 3
SHORT_TF = 1e-4
SHORT_N_EVALS = (1, 2, 3, 40, (1, 40, 3))


def _three(seed=SHORT_SEED):
    rng = np.random.default_rng(seed)
    y0 = np.array([Y0_POLAR, orbit_y0(0.3, 1.0), orbit_y0(0.1, 4.0)])
    return y0, rng.normal(size=(3, 3, KU)) * 0.8


@functools.lru_cache(None)
def dense_points(tf, n_eval, law="sequence", end_tau=END_TAUS):
    """S = 3, max_step = 1; n_eval: an int, or a tuple of per-satellite counts (a ragged launch)"""
    y0, table = _three()
    n = n_eval if np.ndim(n_eval) == 0 else np.array(n_eval, dtype=np.int32)
    return make_case(f"{law}, tf {tf:g}, n_eval {n_eval}", law, y0, tf, 1.0, n, table=table, end_tau=np.array(end_tau, dtype=np.float64),
                     tangential=np.array([0.5, 0.25, 0.1]))


# (d) between the regimes: max_step = 0.05, S = 3, tables that end at 0.37
@functools.lru_cache(None)
def between_regimes():
    y0, table = _three()
    return make_case("between the regimes", "sequence", y0, [2.0, 1.0, 3.0], 0.05, 9, table=table, end_tau=np.full(3, 0.37))


# (e) the other instantiations: S = 3 at max_step = 1
OTHER_LAWS = ("constant", "tangential", "zero")
OTHER_FLAGS_TF = (0.5, 1.0, 0.8)        # (two orbits at 320 km under the atmosphere amplify 2e4 times: beyond what 1e-8 holds)
OTHER_FLAGS = {"none": 0, "J2": J2, "drag": DRAG, "drag+atmosphere+J2": DJ}


@functools.lru_cache(None)
def other_law(law):
    y0, _ = _three()
    rng = np.random.default_rng(11)
    return make_case(f"law {law}", law, y0, [2.5, 1.0, 0.5], 1.0, 9, constant=rng.normal(size=(3, 3)) * 0.3, tangential=np.array([0.5, 0.25, 0.1]))


@functools.lru_cache(None)
def other_flags(which):
    """sequence flights of the low orbits of tests/drag_cases.py (the only ones its atmosphere is anything on), in their own units"""
    c = D.rollout_case()
    atmo = D.models()["general"] if "atmosphere" in which else None
    case = make_case(f"flags {which}", "sequence", c["y0"], OTHER_FLAGS_TF, 1.0, 9, flags=OTHER_FLAGS[which], atmosphere=atmo,
                     table=np.random.default_rng(12).normal(size=(3, 3, KU)) * 0.3, end_tau=np.array(END_TAUS))
    case["const"] = c["const"].copy()
    return case


# host anchor: one satellite per thrust law against scipy, at every combination of the max_step, end_tau and n_eval below
HOST_MAX_STEPS = (1.0, float("inf"), 0.05)
HOST_N_EVALS = (1, 2, 9)


@functools.lru_cache(None)
def host_case(law, max_step, end_tau, n_eval):
    y0, table = _three()
    s = {"sequence": 0, "tangential": 1, "zero": 1, "constant": 2}[law]
    tf = {"sequence": 2.0, "tangential": 2.5, "zero": 2.5, "constant": 1.0}[law]
    return make_case(f"host {law} max_step {max_step:g} end_tau {end_tau:g} n_eval {n_eval}", law, y0[s], tf, max_step, n_eval, table=table[s:s + 1],
                     end_tau=np.array([end_tau]), constant=np.array([[0.2, -0.3, 0.1]]), tangential=np.array([0.3]))


def host_cases():
    for law in D.LAWS:
        for ms in HOST_MAX_STEPS:
            for et in (END_TAUS if law == "sequence" else END_TAUS[:1]):
                for n in HOST_N_EVALS:
                    yield law, ms, et, n


def device_cases():
    """every case the device's values are compared on, under the bound at DEVICE_ULPS"""
    yield mixed_waves()
    for n in SHORT_N_EVALS:
        yield dense_points(SHORT_TF, n)
    yield dense_points(0.5, 40)
    yield dense_points(0.5, 40, "tangential")
    yield between_regimes()
    for law in OTHER_LAWS:
        yield other_law(law)
    for which in OTHER_FLAGS:
        yield other_flags(which)
