"""The planning model with drag (and J2) on the device: the linearisation with the drag partials against the reference's own
include_drag=True Discretizer (tests/golden/drag_discretize.npz, make_drag_golden.py), the fused step against the oracle's
solve of the reference's stage data, the planning rollouts of the SCP iteration and of the update, the controllers -- and
what the planner buys: plans that a truth model with drag and J2 flies as planned."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import oracle_lib as O
import nlp_ipm as N

pytestmark = pytest.mark.gpu
RTOL = 1e-10                     # tests/test_discretize_gpu.py
TOL, TOL_SOL = 1e-9, 5e-6        # tests/test_solve_gpu.py
KEYS = ("A", "Bp", "Bn", "Sigma", "xi")
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drag_discretize.npz"))
CASES = [str(c) for c in GOLD["cases"]]
S_SCALE = 1e4                    # the drag-scaled satellites of the fixture: S x 1e4


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


class _Const:
    def __init__(self, v):
        self.v = np.asarray(v, dtype=np.float64)

    def as_vector(self):
        return self.v


def satellite_dynamics(*a, **k):  # token accepted by Discretizer.discretize
    raise RuntimeError("host dynamics are never called")


def case(name):
    g = lambda k: GOLD[f"{k}_{name}"]
    return dict(x=g("x"), u=g("u"), tf=float(g("tf")), const=g("const"), j2=bool(g("j2")), solver=str(g("solver")),
                steps=int(g("steps")), **{k: g(k) for k in KEYS})


def drag_discretizer(c):
    from mpconstellation_amd import Discretizer
    d = Discretizer(_Const(c["const"]), include_drag=True, include_J2=c["j2"])
    d.ivp_solver = c["solver"]
    if c["steps"]:
        d.use_uniform_steps = True; d.integrator_steps = c["steps"]
    return d


def hubble_constellation(S, first=0, count=None):
    from mpconstellation_amd.constellation import constellation_states, normalize_batch
    return normalize_batch(constellation_states(S, first=first, count=count))


@pytest.mark.parametrize("name", CASES)
def test_drag_discretize_vs_reference(name):
    """A, B, Sigma, xi of Discretizer(include_drag=True[, include_J2=True]) against the reference's drag branch: adaptive RK45,
    uniform steps, RK23; the Hubble's S (drag 2e-8 of A) and S x 1e4 (2e-4 of A)."""
    c = case(name)
    out = drag_discretizer(c).discretize(satellite_dynamics, c["x"], c["u"], c["tf"])
    for k, o in zip(KEYS, out):
        assert o.shape == c[k].shape
        assert relerr(o, c[k]) < RTOL, (k, relerr(o, c[k]))


def test_mixed_drag_batch_equals_single_calls():
    """Drag-scaled and unscaled satellites in one discretize launch, and in one ragged fused step (stage path, Ks): every
    satellite gets the bits of its own single-satellite call."""
    from mpconstellation_amd import _ffi, mpc_step_batch
    from mpconstellation_amd.simulator import propagate_batch
    a, b = case("tan_K30_tf1"), case("tan_K30_tf1_bigS")
    x = np.stack([a["x"]] * 4); u = np.stack([a["u"]] * 4)
    cs = np.stack([a["const"], b["const"], b["const"], a["const"]]); tf = np.array([1.0, 1.0, 0.9, 1.1])
    d = drag_discretizer(a)
    out = d.discretize_batch(x, u, tf, cs)
    assert (out[5] == 0).all()
    for s in range(4):
        one = d.discretize_batch(x[s:s + 1], u[s:s + 1], tf[s:s + 1], cs[s:s + 1])
        for k in range(6):
            assert np.array_equal(out[k][s], one[k][0]), (s, k)
    # the ragged fused step, drag + J2 in the linearisation
    S = 6
    y0, cst = hubble_constellation(4096, first=100, count=S)
    cst[1::2, 5] *= S_SCALE
    Ks = np.array([30, 21, 26, 30, 17, 24], dtype=np.int32)
    tfs = np.ones(S)
    xr, st, _, ur = propagate_batch(y0, tfs, cst, (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None), Ks, thrust=True)
    assert (st == 0).all()
    r_des = np.array([np.linalg.norm(xr[s, :3, Ks[s] - 1]) for s in range(S)])
    res = mpc_step_batch(xr, ur, tfs, cst, r_des, include_drag=True, include_J2=True, Ks=Ks)
    assert (res.status == 0).all(), res.status
    for s in range(S):
        k = Ks[s]
        one = mpc_step_batch(xr[s:s + 1, :, :k], ur[s:s + 1, :, :k], tfs[s:s + 1], cst[s:s + 1], r_des[s:s + 1],
                             include_drag=True, include_J2=True)
        assert one.status[0] == 0 and one.iters[0] == res.iters[s]
        assert np.array_equal(res.X[s][:, :k], one.X[0]) and np.array_equal(res.U[s][:, :k], one.U[0])
        assert np.array_equal(res.NU[s][:, :k], one.NU[0]) and res.tf[s] == one.tf[0] and res.kkt[s] == one.kkt[0]
    # the model reached the step: the drag-free linearisation gives other plans
    assert not np.array_equal(mpc_step_batch(xr, ur, tfs, cst, r_des, include_J2=True, Ks=Ks).X, res.X)


@pytest.mark.parametrize("name", CASES)
def test_drag_step_vs_oracle_on_the_reference_stages(name):
    """mpc_step_batch(include_drag=True) -- the device's own drag linearisation and solve -- against the oracle's solve of the
    reference's drag stage matrices, at tests/test_solve_gpu.py's tolerances for the same stage data (the two stage sets agree
    to 1e-10 relative: test_drag_discretize_vs_reference)."""
    from mpconstellation_amd import mpc_step_batch
    c = case(name)
    x, u, tf, cst = c["x"], c["u"], c["tf"], c["const"]
    r_des = float(np.linalg.norm(x[:3, -1]))
    res = mpc_step_batch(x[None], u[None], [tf], cst[None], [r_des], include_drag=True, include_J2=c["j2"],
                         uniform_steps=c["steps"], rk23=(c["solver"] == "RK23"), regularised=True)
    P = N.MpcProblem(x, u, tf, cst[0], {k: c[k] for k in KEYS}, O.constraint_terms(x, u, cst[0]), {"r_des": r_des})
    ref = N.solve(P)
    assert ref["status"] == 0 and res.status[0] == 0
    n_dev, first_dev = int(res.n_regularised[0]), int(res.first_regularised[0])
    clean = ref["n_regularised"] == 0 and n_dev == 0
    same_path = (clean or (n_dev == ref["n_regularised"] and first_dev == ref["first_regularised"])) and res.iters[0] == ref["iters"]
    assert abs(int(res.iters[0]) - ref["iters"]) <= (1 if clean else 10)
    tol = 5 * TOL if same_path else TOL_SOL
    for a, b in ((res.X[0], ref["X"]), (res.U[0], ref["U"]), (res.NU[0], ref["NU"])):
        assert np.abs(a - b).max() < tol
    assert abs(res.tf[0] - ref["tf"]) < tol
    # the plan satisfies the reference's drag linearisation
    assert np.abs(P.dyn_residual(res.X[0], res.U[0], res.NU[0][:, :-1], res.tf[0])).max() < 1e-8


def test_scp_iteration_with_the_planning_model():
    """scp_iteration_batch(include_drag, include_J2, rollout_model=True): its reference trajectory is propagate_batch's rollout
    under the same law with drag and J2, and its plan the fused step's with the same linearisation -- bit for bit; without
    rollout_model the rollout is the reference's drag- and J2-free one."""
    from mpconstellation_amd import _ffi, mpc_step_batch, scp_iteration_batch
    from mpconstellation_amd.simulator import propagate_batch
    S, K = 24, 30
    y0, consts = hubble_constellation(4096, first=500, count=S)
    consts[::3, 5] *= S_SCALE
    tf = np.linspace(0.8, 1.2, S)
    law = (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None)
    model = dict(include_drag=True, include_J2=True)
    x, st, _, u = propagate_batch(y0, tf, consts, law, K, thrust=True, **model)
    assert (st == 0).all()
    r_des = np.linalg.norm(x[:, :3, -1], axis=1)
    ref = mpc_step_batch(x, u, tf, consts, r_des, **model)
    one = scp_iteration_batch(y0, tf, consts, r_des, law, K, return_reference=True, rollout_model=True, **model)
    assert (one.prop_status == 0).all() and np.array_equal(one.xbar, x) and np.array_equal(one.ubar, u)
    for f in ("X", "U", "NU", "tf", "status", "iters", "kkt"): assert np.array_equal(getattr(one, f), getattr(ref, f)), f
    lin = scp_iteration_batch(y0, tf, consts, r_des, law, K, return_reference=True, **model)
    x0, _, _, u0 = propagate_batch(y0, tf, consts, law, K, thrust=True)
    assert np.array_equal(lin.xbar, x0) and np.array_equal(lin.ubar, u0) and not np.array_equal(lin.xbar, x)


def test_update_with_the_planning_model_equals_its_iterations():
    """ConstellationMPC(plan_drag=True, plan_J2=True): the one-call update (mpcx_mpc_update_batch with MPCX_FLAG_PLAN_ROLLOUTS)
    against the verbose path (one scp_iteration_batch per SCP iteration, rollout_model=True), bit for bit, over two segments
    (ragged second iterations); and the plan is not the reference planner's."""
    import contextlib, io
    from mpconstellation_amd import Satellite, ConstellationMPC
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(4096)[[3, 500, 1234, 2222, 4000]]
    make = lambda: [Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st]
    kw = dict(base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5, sim_base_res=50, plan_drag=True, plan_J2=True)
    a = ConstellationMPC(make(), **kw)
    b = ConstellationMPC(make(), verbose=True, **kw)
    ref = ConstellationMPC(make(), **{**kw, "plan_drag": False, "plan_J2": False})
    for m in (a, b, ref):
        m.consts[1::2, 5] *= S_SCALE
    ref.update()
    for seg in range(2):
        a.run_segment(1)
        with contextlib.redirect_stdout(io.StringIO()):
            b.run_segment(1)
        assert (a.last_status == 0).all() and np.array_equal(a.last_status, b.last_status)
        assert np.array_equal(a.plan_K, b.plan_K) and np.array_equal(a.plan_tf, b.plan_tf)
        for i in range(5):
            assert np.array_equal(a.plan_x[i], b.plan_x[i]) and np.array_equal(a.plan_u[i], b.plan_u[i])
            assert np.array_equal(a.plan_nu[i], b.plan_nu[i])
        if seg == 0:
            assert not np.array_equal(a.plan_tf, ref.plan_tf)
    for sa, sb in zip(a.sats, b.sats):
        assert np.array_equal(a.sim_data[sa.id], b.sim_data[sb.id]) and np.array_equal(sa.get_state_vector(), sb.get_state_vector())


def test_constellation_plan_equals_single_satellite_controllers():
    """ConstellationMPC(plan_drag=True, plan_J2=True) gives every satellite the plan OptimalController(plan_drag=True,
    plan_J2=True) makes for it alone (default kernels), bit for bit."""
    from mpconstellation_amd import Satellite, ConstellationMPC, OptimalController
    r0 = np.array([5371.4806, -4133.1393, 1399.9594]) * 1000; v0 = np.array([4.6921, 4.9848, -3.2752]) * 1000
    make = lambda: [Satellite(r0, v0 * (1 + 0.01 * i), 12200.0) for i in range(3)]
    kw = dict(base_res=15, tf_horizon=2, tf_interval=1, r_des=1.2, plan_drag=True, plan_J2=True)
    mpc = ConstellationMPC(make(), **kw)
    mpc.update()
    assert (mpc.last_status == 0).all(), mpc.last_status
    for i, sat in enumerate(make()):
        c = OptimalController(sats=[sat], plot_inter=False, opt_verbose=False, time_parallel=False, **kw)
        c.update()
        assert c.last_status == [0, 0]
        assert np.array_equal(c.opt_trajectory, mpc.plan_x[i]) and np.array_equal(c.sequence_controller.u, mpc.plan_u[i])
        assert c.sequence_controller.end_tau == mpc.plan_tf[i] / 1


def test_truth_model_planner_predicts_the_flight(capsys):
    """What the planning model is for: 64 satellites with S x 1e4 (drag as large as J2's effect), planned once by the
    reference's planner and once with plan_drag=True, plan_J2=True; each plan's own thrust table flown under the truth model
    (drag + J2) over the plan's tf_u, sampled at the plan's nodes.  The truth-model plan's largest deviation from its own X must
    be at most a fifth of the reference planner's.  Four SCP iterations: after the reference's two the SCP has not converged
    here and its linearisation error, which both planners share, is most of either deviation (measured: 0.057 against 0.14,
    ratio 0.40); after four it is 8e-3 against 0.18 (ratio 0.05)."""
    from mpconstellation_amd import _ffi, Satellite, ConstellationMPC
    from mpconstellation_amd.constellation import constellation_states
    from mpconstellation_amd.simulator import propagate_batch
    S = 64
    states = constellation_states(S)
    make = lambda: [Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in states]
    dev = {}
    for plan in (False, True):
        mpc = ConstellationMPC(make(), base_res=30, tf_horizon=1, tf_interval=1, r_des=1.02, scp_iterations=4,
                               plan_drag=plan, plan_J2=plan)
        mpc.consts[:, 5] *= S_SCALE
        mpc.update()
        assert np.isin(mpc.last_status, (0, 7)).all(), mpc.last_status
        X, U, _ = mpc._plan
        Kp = mpc.plan_K
        y, st, _ = propagate_batch(mpc._y0(), mpc.plan_tf, mpc.consts, (_ffi.CTRL_SEQUENCE, U, U.shape[2], 1.0), Kp,
                                   include_drag=True, include_J2=True, Kus=Kp)
        assert (st == 0).all()
        per_sat = np.array([np.abs(y[s, :, :Kp[s]] - X[s, :, :Kp[s]]).max() for s in range(S)])
        dev[plan] = per_sat
    with capsys.disabled():
        print(f"\ntruth-model flight vs plan, max node deviation over 64 satellites: reference planner {dev[False].max():.3e} "
              f"(median {np.median(dev[False]):.3e}), truth-model planner {dev[True].max():.3e} (median {np.median(dev[True]):.3e}), "
              f"ratio {dev[True].max() / dev[False].max():.3g}")
    assert dev[True].max() <= dev[False].max() / 5
