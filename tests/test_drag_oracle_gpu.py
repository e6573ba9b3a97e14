"""The drag and atmosphere kernels against the CPU oracle (oracle/dynamics.c: the reference's drag branch and density model,
pinned against the reference's own arrays by tests/test_oracle_drag.py) on the inputs of tests/drag_cases.py: everything the
three fixtures with the Hubble's tangential climb do not reach -- thrust in random directions, tf != 1, other R0 / RHO, the
all-zero table, c1 and c2 both non-zero, the floor crossed inside an interval, K = 2 and 3, the stage layout, every thrust law
through the atmosphere with and without J2, the fused step.  Every input is sensitive by >= 1e-7 to the term it is there for and
on no step-acceptance knife edge (test_oracle_drag.py); the tolerance is 1e-10 relative to each array's magnitude
(tests/test_discretize_gpu.py), 1e-10 absolute for rollouts (tests/test_propagate_gpu.py).  Each test prints its worst error
(profiles/drag_oracle_checks.txt)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import drag_cases as D
import oracle_lib as O
import nlp_ipm as N

pytestmark = pytest.mark.gpu
RTOL = 1e-10                     # tests/test_discretize_gpu.py
ATOL_ROLLOUT = 1e-10             # tests/test_propagate_gpu.py, tests/test_atmosphere_gpu.py
TOL, TOL_SOL = 1e-9, 5e-6        # tests/test_solve_gpu.py
KEYS = D.KEYS
relerr = D.relerr


class _Const:
    def __init__(self, v):
        self.v = np.asarray(v, dtype=np.float64)

    def as_vector(self):
        return self.v


def discretizer(cst, model, solver, j2):
    from mpconstellation_amd import Discretizer
    d = Discretizer(_Const(cst), include_drag=True, include_J2=j2, atmosphere=D.models()[model] if isinstance(model, str) else model)
    if solver == "rk23":
        d.ivp_solver = "RK23"
    if solver == "uni11":
        d.use_uniform_steps = True; d.integrator_steps = 11
    return d


def worst_against_oracle(got, x, u, tf, cst, model, solver, j2, what):
    """got: the five arrays of one satellite; -> the largest relative error over them (asserted < RTOL)"""
    ref = D.oracle_discretize(x, u, tf, cst, model, solver, j2)
    assert ref["status"] == 0
    worst = 0.0
    for k in KEYS:
        assert got[k].shape == ref[k].shape, (what, k)
        e = relerr(got[k], ref[k])
        worst = max(worst, e)
        assert e < RTOL, (what, k, e)
    return worst


@pytest.mark.parametrize("model,solver,j2", D.BATCH_CONFIGS, ids=lambda v: str(v))
def test_random_batch_vs_oracle(model, solver, j2):
    """(a) five satellites in one launch, K = 12 (55 interval groups: not a multiple of the 8 per wave): per-satellite tf in
    [0.5, 1.5], u ~ N(0, 0.5^2) with one all-zero table, S x 1e4 on four, different R0 and RHO, inclined orbits of 300-450 km;
    the fixed density and the power-law, exponential and general (c1, c2 != 0) models; RK45, RK23, 11 uniform steps; J2 off, on"""
    b = D.batch()
    out = discretizer(b["const"][0], model, solver, j2).discretize_batch(b["x"], b["u"], b["tf"], b["const"])
    assert (out[5] == 0).all(), out[5]
    worst = max(worst_against_oracle({k: out[i][s] for i, k in enumerate(KEYS)}, b["x"][s], b["u"][s], b["tf"][s], b["const"][s], model, solver, j2, s)
                for s in range(b["x"].shape[0]))
    print(f"batch {model} {solver} j2={j2}: worst relative error {worst:.3g}")


@pytest.mark.parametrize("solver", ["rk45", "rk23"])
@pytest.mark.parametrize("tf", D.FLOOR_TFS)
def test_floor_crossing_discretize_vs_oracle(tf, solver):
    """(b) 350 x 700 km with the floor at 500 km, K = 6: intervals wholly on the floor, wholly above it, and crossing it -- the
    density's branch switches between the stages of a step"""
    c, atm = D.floor_case(tf), D.floor_model()
    ref = D.oracle_discretize(c["x"], c["u"], tf, c["const"], atm, solver, True, dump_nodes=True)
    assert set(D.interval_kinds(ref, c["const"], D.FLOOR_K)) == {"on", "cross", "above"}
    out = discretizer(c["const"], atm, solver, True).discretize_batch(c["x"][None], c["u"][None], [tf], c["const"][None])
    assert out[5][0] == 0
    worst = worst_against_oracle({k: out[i][0] for i, k in enumerate(KEYS)}, c["x"], c["u"], tf, c["const"], atm, solver, True, "floor")
    print(f"floor tf={tf} {solver}: worst relative error {worst:.3g}")


@pytest.mark.parametrize("tf", D.FLOOR_TFS)
def test_floor_crossing_rollout_vs_oracle(tf):
    """(b) the rollout of the same thrust table through the floor and back, 20 output points, the oracle's step count"""
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.simulator import propagate_batch
    c, atm = D.floor_case(tf), D.floor_model()
    ref, rc, ns_ref = O.propagate(c["y0"], tf, c["const"], O.make_ctrl(O.CTRL_SEQUENCE, useq=c["u"], end_tau=1.0), 20, O.FLAG_DRAG | O.FLAG_J2, atmosphere=atm)
    alt = D.altitude(ref, c["const"])
    assert rc == 0 and alt.min() < D.H_FLOOR < alt.max()
    y, st, ns = propagate_batch(c["y0"][None], [tf], c["const"][None], (_ffi.CTRL_SEQUENCE, c["u"], D.FLOOR_K, 1.0), 20, include_drag=True,
                                include_J2=True, atmosphere=atm)
    err = np.abs(y[0] - ref).max()
    print(f"floor rollout tf={tf}: max |device - oracle| = {err:.3g}, steps {ns[0]} / {ns_ref}")
    assert st[0] == 0 and ns[0] == ns_ref and err < ATOL_ROLLOUT


def test_smallest_horizons_vs_oracle():
    """(c) K = 2 and K = 3 with drag, the general atmosphere and J2: one satellite per launch in the reference layout, then both
    in one ragged stage launch"""
    import dev_solve
    from mpconstellation_amd import _ffi
    atm = D.models()["general"]
    cases = [D.short_case(s, K) for s, K in D.SMALL]
    worst = 0.0
    for c, (_, K) in zip(cases, D.SMALL):
        out = discretizer(c["const"], atm, "rk45", True).discretize_batch(c["x"][None], c["u"][None], [c["tf"]], c["const"][None])
        assert out[5][0] == 0 and out[0].shape == (1, K - 1, 7, 7)
        worst = max(worst, worst_against_oracle({k: out[i][0] for i, k in enumerate(KEYS)}, c["x"], c["u"], c["tf"], c["const"], atm, "rk45", True, K))
    Ks = np.array([K for _, K in D.SMALL], dtype=np.int32)
    x, u = np.full((2, 7, 3), np.nan), np.full((2, 3, 3), np.nan)
    for i, (c, K) in enumerate(zip(cases, Ks)):
        x[i, :, :K], u[i, :, :K] = c["x"], c["u"]
    _ffi.set_atmosphere(_ffi.context(0), atm)
    stage, st = dev_solve.discretize_stages(x, u, np.array([c["tf"] for c in cases]), np.array([c["const"] for c in cases]), Ks=Ks, Kus=Ks,
                                            flags=_ffi.discretize_flags(True, True, atmosphere=atm))
    assert (st == 0).all(), st
    for i, (c, K) in enumerate(zip(cases, Ks)):
        worst = max(worst, worst_against_oracle(dev_solve.unpack_stage(stage, i, int(K)), c["x"], c["u"], c["tf"], c["const"], atm, "rk45", True, ("stage", K)))
    print(f"K = 2, 3: worst relative error {worst:.3g}")


@pytest.mark.parametrize("model,j2", [("fixed", False), ("fixed", True), ("general", False), ("general", True)], ids=lambda v: str(v))
def test_stage_layout_vs_oracle(model, j2):
    """(d) the stage records the solve and the benchmark read -- mpcx_discretize_stages_ragged_dev with Ks = [12, 7, 2, 9], NaN in
    the columns past a satellite's count -- against the oracle, satellite by satellite: the drag forms of the stage layout
    compared with something other than themselves"""
    import dev_solve
    from mpconstellation_amd import _ffi
    c, atm = D.stage_case(), D.models()[model]
    _ffi.set_atmosphere(_ffi.context(0), atm)
    stage, st = dev_solve.discretize_stages(c["x"], c["u"], c["tf"], c["const"], Ks=c["Ks"], Kus=c["Ks"], flags=_ffi.discretize_flags(True, j2, atmosphere=atm))
    assert (st == 0).all(), st
    worst = 0.0
    for i, k in enumerate(c["Ks"]):
        k = int(k)
        worst = max(worst, worst_against_oracle(dev_solve.unpack_stage(stage, i, k), c["x"][i][:, :k], c["u"][i][:, :k], c["tf"][i], c["const"][i],
                                                model, "rk45", j2, ("stage", i)))
    print(f"stage layout {model} j2={j2}: worst relative error {worst:.3g}")


@pytest.mark.parametrize("j2", [False, True])
@pytest.mark.parametrize("law", D.LAWS)
def test_rollouts_vs_oracle(law, j2):
    """(e) every thrust law through the general atmosphere, drag without and with J2: three satellites with tf = 0.5, 1, 2 and 20,
    33, 17 output points in one launch; states, step counts, and the thrust at the output points (extract_uk)"""
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.simulator import propagate_batch
    c = D.rollout_case()
    dev_law = {"zero": (_ffi.CTRL_ZERO, None, 0, None), "constant": (_ffi.CTRL_CONSTANT, c["constant"], 0, None),
               "tangential": (_ffi.CTRL_TANGENTIAL, c["tangential"], 0, None), "sequence": (_ffi.CTRL_SEQUENCE, c["sequence"], 12, c["end_tau"])}[law]
    y, st, ns, u = propagate_batch(c["y0"], c["tf"], c["const"], dev_law, c["n_eval"], include_drag=True, include_J2=j2, thrust=True,
                                   atmosphere=D.models()["general"])
    assert (st == 0).all(), st
    worst_y = worst_u = 0.0
    for s in range(3):
        n = int(c["n_eval"][s])
        ref, ns_ref = D.oracle_rollout(law, c, s, j2)
        u_ref = O.extract_uk(ref, np.linspace(0, 1, n), D.oracle_ctrl(law, c, s))
        ey, eu = np.abs(y[s][:, :n] - ref).max(), np.abs(u[s][:, :n] - u_ref).max()
        worst_y, worst_u = max(worst_y, ey), max(worst_u, eu)
        assert ns[s] == ns_ref and ey < ATOL_ROLLOUT and eu < ATOL_ROLLOUT, (s, ns[s], ns_ref, ey, eu)
        assert (y[s][:, n:] == 0).all() and (u[s][:, n:] == 0).all()
    print(f"rollout {law} j2={j2}: max |device - oracle| = {worst_y:.3g} (states), {worst_u:.3g} (thrust)")


@pytest.mark.parametrize("model", ["fixed", "general"])
def test_step_vs_oracle_on_the_oracle_stages(model):
    """(f) mpc_step_batch with drag, then drag and the atmosphere, on three satellites of other R0 and RHO than the Hubble's and
    tf = 1, 0.8, 1.25, K = 12, against the oracle's solve of the oracle's own drag stages: the rules and tolerances of
    tests/test_drag_model_gpu.py::test_drag_step_vs_oracle_on_the_reference_stages"""
    from mpconstellation_amd import mpc_step_batch
    c = D.step_case(model)
    res = mpc_step_batch(c["x"], c["u"], c["tf"], c["const"], c["r_des"], include_drag=True, regularised=True, atmosphere=D.models()[model])
    worst = 0.0
    for s in range(3):
        x, u, tf, cst, r_des = c["x"][s], c["u"][s], float(c["tf"][s]), c["const"][s], float(c["r_des"][s])
        stages = D.oracle_discretize(x, u, tf, cst, model)
        P = N.MpcProblem(x, u, tf, cst[0], {k: stages[k] for k in KEYS}, O.constraint_terms(x, u, cst[0]), {"r_des": r_des})
        ref = N.solve(P)
        assert ref["status"] == 0 and res.status[s] == 0
        n_dev, first_dev = int(res.n_regularised[s]), int(res.first_regularised[s])
        clean = ref["n_regularised"] == 0 and n_dev == 0
        same_path = (clean or (n_dev == ref["n_regularised"] and first_dev == ref["first_regularised"])) and res.iters[s] == ref["iters"]
        assert abs(int(res.iters[s]) - ref["iters"]) <= (1 if clean else 10)
        tol = 5 * TOL if same_path else TOL_SOL
        err = max(np.abs(res.X[s] - ref["X"]).max(), np.abs(res.U[s] - ref["U"]).max(), np.abs(res.NU[s] - ref["NU"]).max(), abs(res.tf[s] - ref["tf"]))
        worst = max(worst, err)
        assert err < tol, (s, err, tol)
        assert np.abs(P.dyn_residual(res.X[s], res.U[s], res.NU[s][:, :-1], res.tf[s])).max() < 1e-8
    print(f"fused step {model}: max |device - oracle| = {worst:.3g}")
