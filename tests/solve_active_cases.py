"""Solves chosen for the inequality constraints that are ACTIVE at their solution: the one list that
tests/test_solve_active_host.py (the list held to its own criteria on the CPU oracle) and tests/test_solve_active_gpu.py (every
solve kernel against the oracle on it) share, with the census that says which constraints a solution sits on.

A case = a committed fixture (tests/golden/disc_*.npz: reference trajectory and the reference's own A / B matrices), the
variant of the tangential-velocity condition, an option set written in the fixture's own quantities (umax = largest node
thrust, m0 / mK = first / last mass, rK = final radius, tf = reference final time; r_des = rK throughout) and the constraint
families the case is there for.  The oracle's solves are computed once per process and shared; nobody changes them.

Families (census): u, rmax, rmin (stage constraints, indices as in MpcProblem.ineq), term0 .. term7 (rows of the terminal
block: 0 final radius from below, 1 / 2 +-Vr, 3 / 4 +-Vn, 5 final-mass floor, 6 / 7 +-Vt linearised, variant linvt only),
rfmax (terminal ball (r_des + eps_r)^2), tf_hi (tf <= tf_max) and nu (virtual control in use)."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import oracle_lib as O
import nlp_ipm as N

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STAGE_KEYS = ("A", "Bp", "Bn", "Sigma", "xi")
STAGE_FAMILIES = ("u", "rmax", "rmin")
FAMILIES = STAGE_FAMILIES + tuple(f"term{j}" for j in range(8)) + ("rfmax", "tf_hi", "nu")
ACTIVE_SLACK, ACTIVE_MULT, ACTIVE_NU = 1e-6, 1e-2, 1e-3
TP_MIN_K = 24                  # row length from which MPCX_SOLVE_TIME_PARALLEL is honoured
TP_SEGMENTS = 4                # csrc/solve_tp.hpp: four segments
TP_TIGHT = 1e-12               # the CPU's partitioned algebra within this of its sequential solve: the device is held to 1e-9


def census(P, result):
    """Which inequalities the oracle's final iterate sits on: per family the set of active indices (positions in the arrays
    of MpcProblem.ineq; {0} for the single-row families).  Active: slack <= 1e-6 and multiplier >= 1e-2; nu: max |NU| >= 1e-3."""
    it = result["iterate"]
    on = lambda k: (it.s[k] <= ACTIVE_SLACK) & (it.z[k] >= ACTIVE_MULT)
    idx = lambda mask: set(int(i) for i in np.flatnonzero(mask))
    c = {f: idx(on(f)) for f in STAGE_FAMILIES}
    term = on("term")
    for j in range(8):
        c[f"term{j}"] = {0} if j < len(term) and term[j] else set()
    c["rfmax"] = idx(on("rfmax"))
    c["tf_hi"] = {0} if "tf" in it.s and on("tf")[1] else set()
    c["nu"] = {0} if np.abs(result["NU"]).max() >= ACTIVE_NU else set()
    return c


def family_values(g, family):
    """the entries of family `family` in a dict g of MpcProblem.ineq"""
    if family.startswith("term"): return g["term"][int(family[4:]):int(family[4:]) + 1]
    if family == "tf_hi": return g["tf"][1:2]
    return g[family]


# ---- option sets, in the fixture's own quantities q = dict(umax, m0, mK, rK, tf) ----
def u_lim(f): return lambda q: {"u_lim": [0, f * q["umax"]]}
def mass_floor(f): return lambda q: {"min_mass": q["mK"] + f * (q["m0"] - q["mK"])}
r_ball = lambda q: {"r_lim": [0.99, 1.0005 * q["rK"]], "eps_r": 1e-3}
tf_short = lambda q: {"tf_max": 0.9 * q["tf"]}
vn_tight = lambda q: {"eps_vn": 1e-9}
controller = lambda q: {"eps_r": 1e-6, "eps_vr": 1e-16, "tf_max": q["tf"]}          # OptimalController's set (control.py:192-197)
def r_floor(r_min): return lambda q: {"r_lim": [r_min, 5]}


def _case(fixture, variant, what, options, declares):
    return dict(id=f"{fixture}-{variant}-{what}", fixture=fixture, variant=variant, options=options, declares=tuple(declares),
                K=int(fixture.split("_K")[1].split("_")[0]))


CASES = [
    _case("tan_K30_tf1", "linvt", "u_lim_0.98", u_lim(0.98), ("u", "term0", "term1", "term4", "term6")),
    _case("tan_K60_tf2", "linvt", "u_lim_0.9", u_lim(0.9), ("u", "rfmax", "nu")),
    _case("const_K30_tf1", "linvt", "u_lim_0.98", u_lim(0.98), ("u", "term2", "term3", "term7", "rfmax", "nu")),
    _case("tan_K30_tf1", "exact", "r_max", r_ball, ("rmax",)),
    _case("tan_K30_tf1", "linvt", "r_max", r_ball, ("rmax",)),
    _case("tan_K60_tf2", "exact", "r_max", r_ball, ("rmax",)),
    _case("tan_K30_tf1", "exact", "tf_max", tf_short, ("tf_hi", "rfmax", "rmin")),
    _case("tan_K30_tf1", "linvt", "tf_max", tf_short, ("tf_hi", "rfmax", "rmin")),
    _case("tan_K30_tf1", "linvt", "min_mass_0.3", mass_floor(0.3), ("term5", "rfmax")),
    _case("tan_K60_tf2", "exact", "min_mass_0.05", mass_floor(0.05), ("term5", "rfmax")),
    _case("tan_K30_tf1", "exact", "eps_vn", vn_tight, ("term3", "term4")),
    _case("tanJ2_K30_tf1", "exact", "controller", controller, ("term2", "rfmax")),
    _case("tan_K60_tf2", "exact", "controller", controller, ("term2", "rfmax")),
    _case("tan_K30_tf1", "exact", "r_min_0.99995", r_floor(0.99995), ("rmin",)),
    _case("tan_K60_tf2", "exact", "r_min_0.99999", r_floor(0.99999), ("rmin",)),
    _case("tan_K20_tf2", "linvt", "u_lim_0.9", u_lim(0.9), ("u", "term6", "nu")),       # K < 24: sequential builds only
]
BY_ID = {c["id"]: c for c in CASES}
IDS = [c["id"] for c in CASES]
TP_IDS = [c["id"] for c in CASES if c["K"] >= TP_MIN_K]
assert len(BY_ID) == len(CASES)


@functools.lru_cache(maxsize=None)
def fixture(name):
    d = np.load(os.path.join(GOLDEN, f"disc_{name}.npz"))
    return {k: d[k] for k in STAGE_KEYS + ("x", "u", "tf", "const")}


def quantities(d):
    x, u = d["x"], d["u"]
    return dict(umax=float(np.sqrt((u ** 2).sum(0).max())), m0=float(x[6, 0]), mK=float(x[6, -1]),
                rK=float(np.linalg.norm(x[:3, -1])), tf=float(d["tf"]))


def options_of(case):
    return case["options"](quantities(fixture(case["fixture"])))


def problem(case, u_scale=1.0):
    """the case's MpcProblem on the fixture's own stage data; u_scale multiplies the reference thrust (the knife-edge probe)"""
    d = fixture(case["fixture"]); q = quantities(d)
    x, u, cst = d["x"], d["u"] * u_scale, d["const"]
    return N.MpcProblem(x, u, q["tf"], cst[0], {k: d[k] for k in STAGE_KEYS}, O.constraint_terms(x, u, cst[0]),
                        {"r_des": q["rK"], **case["options"](q)}, variant=case["variant"])


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """(problem, the oracle's solve, its census): computed once, shared by every test, left unchanged"""
    P = problem(BY_ID[case_id])
    ref = N.solve(P)
    return P, ref, census(P, ref)


@functools.lru_cache(maxsize=None)
def reference_half_way(case_id):
    """the oracle stopped after half of its iterations (no case has a regularised iteration): the common path, half way"""
    P, ref, _ = reference(case_id)
    return N.solve(P, max_iter=ref["iters"] // 2)


def delta(a, b):
    """max(|dX|, |dU|, |dtf|) of two oracle results"""
    return max(np.abs(a["X"] - b["X"]).max(), np.abs(a["U"] - b["U"]).max(), abs(a["tf"] - b["tf"]))


@functools.lru_cache(maxsize=None)
def partitioned(case_id):
    """the oracle run again with the partitioned (time-parallel) algebra of tests/tools/partitioned_riccati.py at four segments,
    as tests/test_partitioned_riccati.py patches it in -> (its result, delta_part against the sequential solve)"""
    import partitioned_riccati as PR
    P, ref, _ = reference(case_id)
    old = PR.SEGMENTS
    PR.SEGMENTS = TP_SEGMENTS; PR._cache.clear()
    N.riccati_channel = PR.partitioned_channel
    try:
        part = N.solve(P)
    finally:
        N.riccati_channel = PR.SEQ_CHANNEL
        PR.SEGMENTS = old; PR._cache.clear()
    return part, delta(part, ref)


def tp_tight(case_id):
    """the CPU's partitioned algebra reproduces its sequential solve to 1e-12 on this case: the device's time-parallel kernel
    is then held to 1e-9 (computed, never typed in)"""
    return bool(partitioned(case_id)[1] <= TP_TIGHT)


# ---- two satellites that share ONE final time (solve_shared_tf) ----
# The shared-tf solve takes one option set for all its satellites: both get the thrust limit of the first case AND the mass
# floor of the min_mass case; the second satellite flies the fixture with its reference thrust raised by a hundredth.
SHARED_TF = dict(fixture="tan_K30_tf1", variant="linvt", u_scales=(1.0, 1.01), declares=("u", "term5", "rfmax"),
                 options=lambda q: {**u_lim(0.98)(q), **mass_floor(0.3)(q)})


def shared_tf_problems():
    return [problem(SHARED_TF, u_scale=f) for f in SHARED_TF["u_scales"]]
