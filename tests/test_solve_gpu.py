"""HIP solver / fused MPC step (through the C ABI) against the CPU oracle.
The solve is an iterative fp64 method with tol 1e-8 on ipopt's scaled error; GPU and oracle run the
same iteration, so iterates agree to rounding (asserted at 1e-9), far inside the 1e-6 tolerance that
BASELINE.json's 'trajectory error' is stated at."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import oracle_lib as O
import nlp_ipm as N

pytestmark = pytest.mark.gpu
TOL = 1e-9        # same stage data in -> same iteration path: agreement to rounding
TOL_PATH = 1e-6   # iterates half way along the same path (unrefined directions, see test_solve_vs_oracle)
TOL_SOL = 5e-6    # stated fp64 tolerance of a converged solution (tol 1e-8 on the scaled KKT error leaves the
                  # minimiser determined to ~1e-6 because the objective is flat: w_tr = 0.002); used wherever GPU and
                  # oracle discretise independently, where a 1e-16 difference can flip one line-search decision
CASES = ["tan_K20_tf2", "tan_K30_tf1", "tan_K60_tf2", "tan_K100_tf1", "zero_K20_tf1", "tanJ2_K30_tf1", "const_K30_tf1"]


def oracle_solve(x, u, tf, cst, r_des, stage=None, **kw):
    stage = stage if stage is not None else O.discretize(x, u, tf, cst)
    P = N.MpcProblem(x, u, tf, cst[0], stage, O.constraint_terms(x, u, cst[0]), {"r_des": r_des, **kw.pop("options", {})})
    return P, N.solve(P, **kw)


def load(golden_dir, name):
    d = np.load(os.path.join(golden_dir, f"disc_{name}.npz"))
    return d, d["x"], d["u"], float(d["tf"]), d["const"]


def solution_tolerance(ref, iters, n_dev, first_dev):
    """The tolerance at which a device solution (iters iterations, n_dev of them regularised, the first at first_dev) is held to
    the oracle's `ref`, and the bound on the difference of their iteration counts.
    Same data, same algorithm: the same iteration path.  Two things are decided by rounding and may part the paths
    near their end: whether the last iterate already meets E_0 <= tol (one iteration more or less), and -- on a path
    that runs through factorisation breakdowns (indefinite reduced Hessian far from the solution, regularised by
    delta_w) -- whether a pivot of a nearly singular matrix comes out at +1e-17 or -1e-17.  Both sides still end at
    the same KKT point: the solutions are compared at rounding level when the paths coincide, at the solver
    tolerance otherwise."""
    clean = ref["n_regularised"] == 0 and n_dev == 0
    same_path = (clean or (n_dev == ref["n_regularised"] and first_dev == ref["first_regularised"])) and iters == ref["iters"]
    assert abs(int(iters) - ref["iters"]) <= (1 if clean else 10)
    return 5 * TOL if same_path else TOL_SOL


@pytest.mark.parametrize("name", CASES)
def test_solve_vs_oracle(golden_dir, name):
    from mpconstellation_amd import solve_batch
    d, x, u, tf, cst = load(golden_dir, name)
    r_des = float(np.linalg.norm(x[:3, -1]))
    stage = {k: d[k] for k in ("A", "Bp", "Bn", "Sigma", "xi")}
    P, ref = oracle_solve(x, u, tf, cst, r_des, stage)
    res = solve_batch(d["A"][None], d["Bp"][None], d["Bn"][None], d["Sigma"][None], d["xi"][None], x[None], u[None],
                      [tf], cst[None], [r_des], regularised=True)
    assert ref["status"] == 0 and res.status[0] == 0
    assert res.kkt[0] <= 1e-8
    # the device reports its own regularised iterations (mpcx_solve_regularised): a rounding flip of a breakdown decision
    # shows as a different count / first index, a path divergence without any regularisation on either side would not
    n_dev, first_dev = int(res.n_regularised[0]), int(res.first_regularised[0])
    firsts = ([ref["first_regularised"]] if ref["n_regularised"] > 0 else []) + ([first_dev] if n_dev > 0 else [])
    tol = solution_tolerance(ref, res.iters[0], n_dev, first_dev)
    assert np.abs(res.X[0] - ref["X"]).max() < tol
    assert np.abs(res.U[0] - ref["U"]).max() < tol
    assert np.abs(res.NU[0] - ref["NU"]).max() < tol
    assert abs(res.tf[0] - ref["tf"]) < tol
    # ... and half way (to the end, or to the oracle's first breakdown: the device does not report its own) the two
    # paths are the same: stop both there and compare the iterates.  Tolerance: a direction solved without refinement
    # carries a relative error of 1e-9 .. 1e-6 depending on the barrier weights ("Linear solve"), which the
    # following iterations contract again -- observed up to 2e-8 half way, 1e-14 at the end
    cap = (min(firsts) if firsts else ref["iters"]) // 2
    _, refc = oracle_solve(x, u, tf, cst, r_des, stage, max_iter=cap)
    resc = solve_batch(d["A"][None], d["Bp"][None], d["Bn"][None], d["Sigma"][None], d["xi"][None], x[None], u[None],
                       [tf], cst[None], [r_des], max_iter=cap)
    assert resc.iters[0] == refc["iters"] == cap
    assert np.abs(resc.X[0] - refc["X"]).max() < TOL_PATH and np.abs(resc.U[0] - refc["U"]).max() < TOL_PATH
    assert np.abs(resc.NU[0] - refc["NU"]).max() < TOL_PATH and abs(resc.tf[0] - refc["tf"]) < TOL_PATH
    # the result satisfies the reference NLP: dynamics with the reference's own A/B (from the golden file)
    e = P.dyn_residual(res.X[0], res.U[0], res.NU[0][:, :-1], res.tf[0])
    assert np.abs(e).max() < 1e-8
    assert np.abs(res.X[0][:, 0] - x[:, 0]).max() == 0.0            # x_0 fixed (optimizer.py:344-345)
    h = np.cross(res.X[0][:3, -1], res.X[0][3:6, -1])
    assert abs(np.linalg.norm(h) / np.linalg.norm(res.X[0][:3, -1]) - P.vt_des) < 1e-7   # tangential speed = vt_des


def test_clean_start_classification_matches_the_oracle(golden_dir):
    """The start value of mu and the superlinear barrier rule depend on whether the start is "clean" (reference strictly
    inside its stage constraints and the tf range, ending within 3 eps_r of r_des: DESIGN.md, "Solver algorithm").  Kernel
    and oracle must classify alike on both sides of every criterion: same iteration counts, same solutions -- and the clean
    starts are the short ones."""
    from mpconstellation_amd import solve_batch
    d, x, u, tf, cst = load(golden_dir, "tan_K30_tf1")
    stage = {k: d[k] for k in ("A", "Bp", "Bn", "Sigma", "xi")}
    rK = float(np.linalg.norm(x[:3, -1])); eps = 0.01
    umax = float(np.sqrt((u ** 2).sum(0).max()))
    cases = [("clean", rK, {}, True),
             ("radius 2.9 eps off", rK + 2.9 * eps, {}, True), ("radius 3.1 eps off", rK + 3.1 * eps, {}, False),
             ("tf_bar on its bound", rK, {"tf_max": tf}, False), ("tf_bar inside", rK, {"tf_max": 1.01 * tf}, True),
             ("thrust limit below the reference", rK, {"u_lim": [0, 0.9 * umax]}, False)]
    iters = {}
    for name, r_des, opts, clean in cases:
        P, ref = oracle_solve(x, u, tf, cst, r_des, stage, options=dict(opts))
        assert bool(ref["iterate"].clean) == clean, name
        res = solve_batch(d["A"][None], d["Bp"][None], d["Bn"][None], d["Sigma"][None], d["xi"][None], x[None], u[None],
                          [tf], cst[None], [r_des], options=dict(opts), regularised=True)
        assert ref["status"] == 0 and res.status[0] == 0, name
        if ref["n_regularised"] == 0 and res.n_regularised[0] == 0:
            assert abs(int(res.iters[0]) - ref["iters"]) <= 1, (name, res.iters[0], ref["iters"])
            assert np.abs(res.X[0] - ref["X"]).max() < (5 * TOL if res.iters[0] == ref["iters"] else TOL_SOL), name
        iters[name] = int(res.iters[0])
    assert iters["clean"] < iters["tf_bar on its bound"] and iters["radius 2.9 eps off"] < iters["radius 3.1 eps off"] + 3


def test_fused_step_batch_vs_oracle(golden_dir):
    """discretize + solve fused on the device for a ragged batch (different satellites, constants, r_des)."""
    from mpconstellation_amd import mpc_step_batch
    c64 = np.load(os.path.join(golden_dir, "constellation64.npz"))
    idx = list(c64["idx"])
    x = np.stack([c64[f"x_{i}"] for i in idx]); u = np.stack([c64[f"u_{i}"] for i in idx])
    cs = np.stack([c64[f"const_{i}"] for i in idx])
    r_des = np.linalg.norm(x[:, :3, -1], axis=1)
    res = mpc_step_batch(x, u, np.ones(len(idx)), cs, r_des)
    assert (res.status == 0).all()
    for n, i in enumerate(idx):
        stage = {k: c64[f"{k}_{i}"] for k in ("A", "Bp", "Bn", "Sigma", "xi")}     # the reference's own discretisation
        P, ref = oracle_solve(x[n], u[n], 1.0, cs[n], float(r_des[n]), stage)
        assert ref["status"] == 0
        for a, b in ((res.X[n], ref["X"]), (res.U[n], ref["U"]), (res.NU[n], ref["NU"])):
            assert np.abs(a - b).max() < TOL_SOL
        assert abs(res.tf[n] - ref["tf"]) < TOL_SOL


def test_option_handling_and_status(golden_dir):
    from mpconstellation_amd import mpc_step_batch
    d, x, u, tf, cst = load(golden_dir, "tan_K20_tf2")
    r_des = float(np.linalg.norm(x[:3, -1]))
    opts = {"eps_r": 1e-3, "w_tr": 0.01, "tf_max": 3.0, "u_lim": [0, 2.0]}
    res = mpc_step_batch(x[None], u[None], [tf], cst[None], [r_des], options=opts)
    P, ref = oracle_solve(x, u, tf, cst, r_des, options=opts)
    assert res.status[0] == 0 and ref["status"] == 0
    assert np.abs(res.X[0] - ref["X"]).max() < TOL_SOL and np.abs(res.U[0] - ref["U"]).max() < TOL_SOL
    assert np.linalg.norm(res.U[0], axis=0).max() <= 2.0 + 1e-6
    # iteration cap -> MPCX_ST_MAXITER (5), same iterate as the oracle after 3 iterations
    res3 = mpc_step_batch(x[None], u[None], [tf], cst[None], [r_des], max_iter=3)
    _, ref3 = oracle_solve(x, u, tf, cst, r_des, max_iter=3)
    assert res3.status[0] == 5 and res3.iters[0] == 3
    assert np.abs(res3.X[0] - ref3["X"]).max() < 1e-8        # observed 3.5e-10 (device and oracle discretise independently)


def test_constellation_properties_full_size():
    """BASELINE config 2 (S=64, K=30) end to end on the device: rollout -> discretize -> solve.  Size-independent
    properties: every problem converges, satisfies the linearised dynamics it was given (recomputed by the
    oracle's discretizer for a sample), the terminal constraints and bounds, and never raises tf above tf_max."""
    from mpconstellation_amd import mpc_step_batch, _ffi
    from mpconstellation_amd.constellation import constellation_states, normalize_batch, tangential_thrust
    from mpconstellation_amd.simulator import propagate_batch
    S, K = 64, 30
    y0, consts = normalize_batch(constellation_states(S))
    xbar, st, _ = propagate_batch(y0, np.ones(S), consts, (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None), K)
    assert (st == 0).all()
    ubar = tangential_thrust(xbar, 0.5)
    r_des = np.linalg.norm(xbar[:, :3, -1], axis=1)
    res = mpc_step_batch(xbar, ubar, np.ones(S), consts, r_des)
    assert (res.status == 0).all()
    assert res.kkt.max() <= 1e-8
    assert (res.tf > 0).all() and (res.tf <= 5 + 1e-6).all()
    assert np.abs(res.X[:, :, 0] - xbar[:, :, 0]).max() == 0.0
    rK = np.linalg.norm(res.X[:, :3, -1], axis=1)
    assert np.abs(rK - r_des).max() <= 0.01 + 1e-6                       # eps_r window (optimizer.py:398-403)
    assert np.linalg.norm(res.U, axis=1).max() <= 5 + 1e-6
    assert np.abs(res.NU).max() < 1e-6                                   # virtual control not needed here
    for s in (0, 21, 63):
        od = O.discretize(xbar[s], ubar[s], 1.0, consts[s])
        P = N.MpcProblem(xbar[s], ubar[s], 1.0, consts[s][0], od, O.constraint_terms(xbar[s], ubar[s], consts[s][0]),
                         {"r_des": float(r_des[s])})
        assert np.abs(P.dyn_residual(res.X[s], res.U[s], res.NU[s][:, :-1], res.tf[s])).max() < 1e-8
        ref = N.solve(P)
        assert np.abs(res.X[s] - ref["X"]).max() < TOL_SOL and abs(res.tf[s] - ref["tf"]) < TOL_SOL


def test_optimizer_class_drop_in(golden_dir):
    """The reference's own usage pattern (test_optimizer.py:30-69) at K=20."""
    from mpconstellation_amd import (Satellite, SatelliteScale, Simulator, Discretizer, Optimizer,
                                     ConstantTangentialThrustController, SequenceController)
    sat = Satellite(np.array([5371.4806, -4133.1393, 1399.9594]) * 1000, np.array([4.6921, 4.9848, -3.2752]) * 1000, 12200)
    scale = SatelliteScale(sat=sat); const = scale.get_normalized_constants()
    c = ConstantTangentialThrustController([sat], 0.5)
    sim = Simulator(sats=[sat], controller=c, scale=scale, base_res=10, include_drag=False, include_J2=False)
    sim.run(tf=2)
    x = sim.sim_data[sat.id]
    g = np.load(os.path.join(golden_dir, "disc_tan_K20_tf2.npz"))
    assert np.abs(x - g["x"]).max() < 1e-10                             # device rollout = reference rollout
    d = Discretizer(const, use_scipy_ZOH=False, include_drag=False, include_J2=False)
    u_bar = Discretizer.extract_uk(x, sim.sim_time[sat.id], c)
    assert np.abs(u_bar - g["u"]).max() < 1e-10
    opt = Optimizer([x], [u_bar], [np.zeros((7, 20))], 2, d, Simulator.satellite_dynamics, scale, verbose=False)
    ct = opt.get_constraint_terms()
    for k in ct:
        assert np.allclose(ct[k][0], g["ct_" + k], rtol=0, atol=1e-12, equal_nan=True), k
    opt.solve_OPT(input_options={'r_des': np.linalg.norm(x[0:3, -1])})
    assert opt.get_solved_trajectory(0).shape == (7, 20) and opt.get_solved_u(0).shape == (3, 20)
    assert opt.get_solved_nu(0).shape == (7, 20)
    P, ref = oracle_solve(g["x"], g["u"], 2.0, g["const"], float(np.linalg.norm(g["x"][:3, -1])))
    assert abs(opt.get_solved_tf(0) - ref["tf"]) < TOL_SOL
    assert np.abs(opt.get_solved_trajectory(0) - ref["X"]).max() < TOL_SOL
    # forward simulation with the optimised sequence, as the reference test does (:66-74)
    c_opt = SequenceController(u=opt.get_solved_u(0), tf_u=opt.get_solved_tf(0), tf_sim=5)
    sim = Simulator(sats=[sat], controller=c_opt, scale=scale, base_res=10, include_drag=False, include_J2=False)
    sim.run(tf=5)
    assert sim.sim_data[sat.id].shape == (7, 50) and np.isfinite(sim.sim_data[sat.id]).all()


def test_reference_test_optimizer_as_written():
    """test_optimizer.py:18-69 with the resolution it hard-codes: Hubble, constant tangential thrust 0.5, tf = 2, base_res = 100
    -> K = 200 nodes, r_des = |r_bar_K|, every other option at its default.  The reference's classes end to end on the
    device; the oracle (its own rollout, its own discretisation) must land on the same solution."""
    from mpconstellation_amd import (Satellite, SatelliteScale, Simulator, Discretizer, Optimizer,
                                     ConstantTangentialThrustController, SequenceController)
    sat = Satellite(np.array([5371.4806, -4133.1393, 1399.9594]) * 1000, np.array([4.6921, 4.9848, -3.2752]) * 1000, 12200)
    scale = SatelliteScale(sat=sat); const = scale.get_normalized_constants()
    c = ConstantTangentialThrustController([sat], 0.5)
    tf, base_res = 2, 100
    sim = Simulator(sats=[sat], controller=c, scale=scale, base_res=base_res, include_drag=False, include_J2=False)
    sim.run(tf=tf)
    x = sim.sim_data[sat.id]; K = x.shape[1]
    assert K == 200
    d = Discretizer(const, use_scipy_ZOH=False, include_drag=False, include_J2=False)
    u_bar = Discretizer.extract_uk(x, sim.sim_time[sat.id], c)
    opt = Optimizer([x], [u_bar], [np.zeros((7, K))], tf, d, Simulator.satellite_dynamics, scale, verbose=False)
    r_des = float(np.linalg.norm(x[0:3, -1]))
    opt.solve_OPT(input_options={'r_des': r_des})
    assert opt.status[0] == 0 and opt.result.kkt[0] <= 1e-8
    X, U = opt.get_solved_trajectory(0), opt.get_solved_u(0)
    assert X.shape == (7, K) and U.shape == (3, K) and opt.get_solved_nu(0).shape == (7, K)
    # oracle chain from the same initial state
    cst = const.as_vector()
    tan = O.make_ctrl(O.CTRL_TANGENTIAL, (0.5, 0, 0))
    xo, rc, _ = O.propagate(x[:, 0], float(tf), cst, tan, K)
    assert rc == 0 and np.abs(xo - x).max() < 1e-9
    uo = O.extract_uk(xo, np.linspace(0, 1, K), tan)
    P, ref = oracle_solve(xo, uo, float(tf), cst, float(np.linalg.norm(xo[:3, -1])))
    assert ref["status"] == 0
    assert abs(opt.get_solved_tf(0) - ref["tf"]) < TOL_SOL and np.abs(X - ref["X"]).max() < TOL_SOL
    assert np.abs(U - ref["U"]).max() < 5e-4                            # u is held only by 2 w_tr = 0.004
    # the forward simulation the reference test ends with (:66-74)
    c_opt = SequenceController(u=U, tf_u=opt.get_solved_tf(0), tf_sim=5)
    sim = Simulator(sats=[sat], controller=c_opt, scale=scale, base_res=base_res, include_drag=False, include_J2=False)
    sim.run(tf=5)
    assert sim.sim_data[sat.id].shape == (7, 500) and np.isfinite(sim.sim_data[sat.id]).all()


def test_page_locked_arrays_give_the_same_result(golden_dir):
    """mpcx_host_alloc: caller arrays in page-locked memory are transferred without the staging copy; same results bit for
    bit, and the result buffers of pinned_results=True are reused by the next call of the same shape."""
    from mpconstellation_amd import mpc_step_batch, _ffi
    c64 = np.load(os.path.join(golden_dir, "constellation64.npz"))
    idx = list(c64["idx"])
    x = np.stack([c64[f"x_{i}"] for i in idx]); u = np.stack([c64[f"u_{i}"] for i in idx])
    cs = np.stack([c64[f"const_{i}"] for i in idx]); tf = np.ones(len(idx))
    r_des = np.linalg.norm(x[:, :3, -1], axis=1)
    a = mpc_step_batch(x, u, tf, cs, r_des)
    px, pu, pc, pt, pr = (_ffi.pinned_copy(v) for v in (x, u, cs, tf, r_des))
    b = mpc_step_batch(px, pu, pt, pc, pr, pinned_results=True)
    assert np.array_equal(a.X, b.X) and np.array_equal(a.U, b.U) and np.array_equal(a.tf, b.tf) and np.array_equal(a.iters, b.iters)
    keep = b.X.copy()
    c = mpc_step_batch(px, pu, pt, pc, pr, pinned_results=True)
    assert c.X is b.X and np.array_equal(c.X, keep)


def test_two_solves_of_one_context_on_two_streams():
    """include/mpcx.h, MPCX_SOLVE_INDEX_ORDER: with the plain launch order a context keeps no state between solves, and two
    _dev calls of ONE context may be in flight on different streams -- every launch has its own work-queue counter (a
    shared one would hand each queue position to only one of the two kernels and leave satellites unsolved).  Two fused
    steps of 4096 satellites enqueued back to back on two streams against the same steps run one after the other."""
    import ctypes as C
    import torch
    from mpconstellation_amd import _ffi
    from test_full_size_gpu import workload
    lib = _ffi.load(); ctx = _ffi.context(0)
    S, K = 4096, 30
    dev = torch.device("cuda", 0)
    T = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    sets = []
    for first in (0, 4096):
        xbar, ubar, consts, r_des = workload(8192, K, first=first, count=S)
        sets.append(dict(x=T(xbar), u=T(ubar), tf=T(np.ones(S)), c=T(consts), rd=T(r_des)))
    opts = _ffi.make_solve_opts({}, flags=_ffi.SOLVE_INDEX_ORDER)
    nws = lib.mpcx_mpc_step_workspace_bytes_ctx(ctx, S, K) // 8 + 8
    assert nws * 8 <= lib.mpcx_mpc_step_workspace_bytes(S, K) + 64                      # (the ctx-aware query: slots, not satellites)
    p = lambda t: C.c_void_p(t.data_ptr())

    def run(streams):
        outs = []
        for d, st in zip(sets, streams):
            o = dict(X=torch.empty((S, 7, K), dtype=torch.float64, device=dev), U=torch.empty((S, 3, K), dtype=torch.float64, device=dev),
                     NU=torch.empty((S, 7, K), dtype=torch.float64, device=dev), tf=torch.empty(S, dtype=torch.float64, device=dev),
                     kkt=torch.empty(S, dtype=torch.float64, device=dev), st=torch.full((S,), -1, dtype=torch.int32, device=dev),
                     it=torch.empty(S, dtype=torch.int32, device=dev), ws=torch.empty(nws, dtype=torch.float64, device=dev))
            outs.append(o)
        torch.cuda.synchronize()
        for d, o, st in zip(sets, outs, streams):
            _ffi.check(lib.mpcx_mpc_step_batch_dev(ctx, S, K, p(d["x"]), p(d["u"]), p(d["tf"]), p(d["c"]), p(d["rd"]), 0, 1e-2, C.byref(opts),
                                                   p(o["X"]), p(o["U"]), p(o["NU"]), p(o["tf"]), p(o["st"]), p(o["it"]), p(o["kkt"]), p(o["ws"]),
                                                   C.c_void_p(st.cuda_stream)), ctx, "mpc_step_dev")
        torch.cuda.synchronize()
        return [{k: v.cpu().numpy() for k, v in o.items() if k != "ws"} for o in outs]
    s0 = torch.cuda.current_stream()
    serial = run([s0, s0])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    overlapped = run([s1, s2])
    for a, b in zip(serial, overlapped):
        assert (b["st"] == 0).all()
        for k in a: assert np.array_equal(a[k], b[k]), k
