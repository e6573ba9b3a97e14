"""The altitude-dependent atmosphere on the device (include/mpcx.h, MPCX_FLAG_ATMO / mpcx_set_atmosphere): the linearisation and
the rollouts against arrays the reference's own drag code produced with the same density model (tests/golden/atmo_*.npz,
make_atmo_golden.py), the fused step against the oracle's solve of the reference's stage data, mixed batches, the floor, the
argument checks, ConstellationMPC with the model on both sides -- and what it is for: a plan that knows the atmosphere the truth
model flies through.

The discretize entry points return no step counts, so the accepted step nodes the fixture stores (node_counts_*) are compared
here only through what they produce: a quadrature over another node set would differ from the reference's at 1e-6, not 1e-10."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import oracle_lib as O
import nlp_ipm as N

from mpconstellation_amd import Atmosphere

pytestmark = pytest.mark.gpu
RTOL = 1e-10                     # tests/test_discretize_gpu.py: every discretise mode
TOL, TOL_SOL = 1e-9, 5e-6        # tests/test_solve_gpu.py
KEYS = ("A", "Bp", "Bn", "Sigma", "xi")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "atmo_discretize.npz"))
PROP = np.load(os.path.join(HERE, "golden", "atmo_propagate.npz"))
CASES = [str(c) for c in GOLD["cases"]]
S_SCALE = 1e4
RHO_500 = 9.983e-13              # the fixed density (simulator.py:112)
C_RHO, C_S = 7, 5                # MPCX_C_RHO, MPCX_C_S
POWER = Atmosphere.power_law()


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
    K = int(g("K"))
    return dict(x=GOLD[f"x_K{K}"], u=GOLD[f"u_K{K}"], tf=float(g("tf")), const=g("const"), j2=bool(g("j2")), solver=str(g("solver")),
                steps=int(g("steps")), atm=Atmosphere(*GOLD[f"atmo_{str(g('model'))}"]), **{k: g(k) for k in KEYS})


def atmo_discretizer(c, atmosphere="case"):
    from mpconstellation_amd import Discretizer
    d = Discretizer(_Const(c["const"]), include_drag=True, include_J2=c["j2"], atmosphere=c["atm"] if atmosphere == "case" else atmosphere)
    d.ivp_solver = c["solver"]
    if c["steps"]:
        d.use_uniform_steps = True; d.integrator_steps = c["steps"]
    return d


def hubble_constellation(S, first=0, count=None):
    from mpconstellation_amd.constellation import constellation_states, normalize_batch
    return normalize_batch(constellation_states(S, first=first, count=count))


@pytest.mark.parametrize("name", CASES)
def test_atmosphere_discretize_vs_reference(name):
    """A, B, Sigma, xi of Discretizer(include_drag=True, atmosphere=...) against the reference's drag branch with the same model
    as rho_func / drho_func: adaptive RK45, with J2, RK23, uniform steps, the exponential model, the Hubble's own S.  The
    fixture's position block and altitude dependence are each >= 1e-6 of A on the S x 1e4 cases (test_atmosphere_host.py)."""
    c = case(name)
    out = atmo_discretizer(c).discretize(satellite_dynamics, c["x"], c["u"], c["tf"])
    for k, o in zip(KEYS, out):
        assert o.shape == c[k].shape
        print(f"{name} {k}: relative error {relerr(o, c[k]):.3g}")
        assert relerr(o, c[k]) < RTOL, (k, relerr(o, c[k]))
    # ... and the fixed-density kernel does not pass for it
    if "bigS" in name:
        assert relerr(atmo_discretizer(c, None).discretize(satellite_dynamics, c["x"], c["u"], c["tf"])[0], c["A"]) > 1e-6


@pytest.mark.parametrize("name", [str(c) for c in PROP["cases"]])
def test_atmosphere_propagate_vs_reference(name):
    """rollouts of one orbit through a density that changes by orders of magnitude, drag and J2 on, S x 1e4, against scipy's
    solve_ivp of the reference's dynamics with the same model (tests/test_propagate_gpu.py's comparison, at 1e-10)"""
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.simulator import propagate_batch
    atm = Atmosphere(*PROP[f"atmo_{str(PROP[f'model_{name}'])}"])
    law = (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None) if str(PROP[f"law_{name}"]) == "tan" else \
        (_ffi.CTRL_SEQUENCE, PROP["useq"], PROP["useq"].shape[1], 1.0)
    y, st, _ = propagate_batch(PROP["y0"][None], [1.0], PROP["const"][None], law, int(PROP["n_eval"]), include_drag=True,
                               include_J2=True, atmosphere=atm)
    err = np.abs(y[0] - PROP[f"y_{name}"]).max()
    print(f"{name}: max |device - reference| = {err:.3g}")
    assert st[0] == 0 and err < 1e-10
    fixed = propagate_batch(PROP["y0"][None], [1.0], PROP["const"][None], law, int(PROP["n_eval"]), include_drag=True, include_J2=True)[0]
    assert np.abs(fixed[0] - PROP[f"y_{name}"]).max() > 1e-6


@pytest.mark.parametrize("name", CASES)
def test_atmosphere_step_vs_oracle_on_the_reference_stages(name):
    """mpc_step_batch(include_drag=True, atmosphere=...) -- the device's own linearisation and solve -- against the oracle's solve
    of the reference's stage matrices of the same fixture, as tests/test_drag_model_gpu.py does for the fixed density, at its
    tolerances."""
    from mpconstellation_amd import mpc_step_batch
    c = case(name)
    x, u, tf, cst = c["x"], c["u"], c["tf"], c["const"]
    r_des = float(np.linalg.norm(x[:3, -1]))
    res = mpc_step_batch(x[None], u[None], [tf], cst[None], [r_des], include_drag=True, include_J2=c["j2"],
                         uniform_steps=c["steps"], rk23=(c["solver"] == "RK23"), regularised=True, atmosphere=c["atm"])
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
    assert np.abs(P.dyn_residual(res.X[0], res.U[0], res.NU[0][:, :-1], res.tf[0])).max() < 1e-8


def test_mixed_atmosphere_batch_equals_single_calls():
    """S and S x 1e4 satellites with different tf in one discretize launch, and in one ragged fused step (Ks): every satellite
    gets the bits of its own single-satellite call, and not those of the same batch without the atmosphere."""
    from mpconstellation_amd import _ffi, mpc_step_batch
    from mpconstellation_amd.simulator import propagate_batch
    a, b = case("power_S"), case("power_bigS")
    x = np.stack([a["x"]] * 4); u = np.stack([a["u"]] * 4)
    cs = np.stack([a["const"], b["const"], b["const"], a["const"]]); tf = np.array([1.0, 1.0, 0.9, 1.1])
    d = atmo_discretizer(a)
    out = d.discretize_batch(x, u, tf, cs)
    assert (out[5] == 0).all()
    for s in range(4):
        one = d.discretize_batch(x[s:s + 1], u[s:s + 1], tf[s:s + 1], cs[s:s + 1])
        for k in range(6):
            assert np.array_equal(out[k][s], one[k][0]), (s, k)
    assert not np.array_equal(atmo_discretizer(a, None).discretize_batch(x, u, tf, cs)[0], out[0])
    # the ragged fused step, drag + J2 in the linearisation
    S = 6
    y0, cst = hubble_constellation(4096, first=100, count=S)
    cst[1::2, C_S] *= S_SCALE
    Ks = np.array([30, 21, 26, 30, 17, 24], dtype=np.int32)
    tfs = np.array([1.0, 0.8, 1.1, 0.9, 1.0, 1.2])
    model = dict(include_drag=True, include_J2=True, atmosphere=POWER)
    xr, st, _, ur = propagate_batch(y0, tfs, cst, (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None), Ks, thrust=True, **model)
    assert (st == 0).all()
    r_des = np.array([np.linalg.norm(xr[s, :3, Ks[s] - 1]) for s in range(S)])
    res = mpc_step_batch(xr, ur, tfs, cst, r_des, Ks=Ks, **model)
    assert (res.status == 0).all(), res.status
    for s in range(S):
        k = Ks[s]
        one = mpc_step_batch(xr[s:s + 1, :, :k], ur[s:s + 1, :, :k], tfs[s:s + 1], cst[s:s + 1], r_des[s:s + 1], **model)
        assert one.status[0] == 0 and one.iters[0] == res.iters[s]
        assert np.array_equal(res.X[s][:, :k], one.X[0]) and np.array_equal(res.U[s][:, :k], one.U[0])
        assert np.array_equal(res.NU[s][:, :k], one.NU[0]) and res.tf[s] == one.tf[0] and res.kkt[s] == one.kkt[0]
    assert not np.array_equal(mpc_step_batch(xr, ur, tfs, cst, r_des, include_drag=True, include_J2=True, Ks=Ks).X, res.X)


def test_floor_above_the_trajectory_is_a_fixed_density():
    """h_floor above every altitude the launch meets: the density is rho(h_floor) everywhere and drho = 0, the physics of a
    fixed-density launch whose constants' RHO is scaled by 9.983e-13 / rho(h_floor) -- the path the existing goldens pin.  The two
    agree to 1e-12 relative (they differ by the rounding of the density ratio), in the linearisation and in the rollout."""
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.simulator import propagate_batch
    c = case("power_bigS_J2")
    atm = Atmosphere.power_law(a=2.4e31, b=5.9, h_floor=2e7)             # rho(h_floor) = 2e-12: twice the fixed density
    assert np.linalg.norm(c["x"][:3] * c["const"][6], axis=0).max() - 6.371e6 < 2e7
    scaled = c["const"].copy(); scaled[C_RHO] *= RHO_500 / float(atm.density(2e7))
    got = atmo_discretizer(c, atm).discretize(satellite_dynamics, c["x"], c["u"], c["tf"])
    want = atmo_discretizer({**c, "const": scaled}, None).discretize(satellite_dynamics, c["x"], c["u"], c["tf"])
    plain = atmo_discretizer(c, None).discretize(satellite_dynamics, c["x"], c["u"], c["tf"])
    for k, g, w, p in zip(KEYS, got, want, plain):
        print(f"floor {k}: relative difference {relerr(g, w):.3g}")
        assert relerr(g, w) < 1e-12, (k, relerr(g, w))
    assert relerr(got[0], plain[0]) > 1e-8                       # (the floor's density is not the fixed one: the scaling matters)
    law = (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None)
    y0, cst = PROP["y0"][None], PROP["const"][None]
    scaled = cst.copy(); scaled[:, C_RHO] *= RHO_500 / float(atm.density(2e7))
    y, st, ns = propagate_batch(y0, [1.0], cst, law, 40, include_drag=True, include_J2=True, atmosphere=atm)
    yw, stw, nsw = propagate_batch(y0, [1.0], scaled, law, 40, include_drag=True, include_J2=True)
    print(f"floor rollout: relative difference {relerr(y, yw):.3g}")
    assert st[0] == 0 and stw[0] == 0 and ns[0] == nsw[0] and relerr(y, yw) < 1e-12


def test_argument_checks():
    """MPCX_FLAG_ATMO without MPCX_FLAG_DRAG, or on a context without an atmosphere, and a non-positive floor: MPCX_E_BADARG with
    a message, nothing launched (the result buffers keep what they held); after mpcx_set_atmosphere(ctx, NULL) a plain drag call
    gives the bits it gave before the context ever had an atmosphere."""
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.simulator import _propagate_call
    from mpconstellation_amd.optimizer import _step_call
    slot = 6                                                   # a context of this test's own: it has never had an atmosphere
    ctx = _ffi.context(0, slot)
    y0, cst = PROP["y0"][None].copy(), PROP["const"][None].copy()
    tf = np.ones(1); mag = np.array([0.5])

    def rollout(flags):
        out = dict(y=np.full((1, 7, 20), -7.0), status=np.full(1, -7, dtype=np.int32), nsteps=np.full(1, -7, dtype=np.int32))
        _propagate_call(y0, tf, cst, mag, None, None, None, device=0, slot=slot, out=out, n_eval=20, flags=flags, kind=_ffi.CTRL_TANGENTIAL,
                        Ku=0, max_step=1e-3)
        return out

    def refused(fn, text):
        with pytest.raises(_ffi.MpcxError, match=r"\(-2\)") as e:
            fn()
        assert text in str(e.value), str(e.value)
    DRAG, J2, ATMO = _ffi.FLAG_DRAG, _ffi.FLAG_J2, _ffi.FLAG_ATMO
    before = rollout(DRAG | J2)
    assert before["status"][0] == 0
    refused(lambda: rollout(DRAG | ATMO), "mpcx_set_atmosphere")                 # no atmosphere on the context
    refused(lambda: _ffi.set_atmosphere(ctx, (1.0, -2.0, 0.0, 0.0)), "h_floor")  # non-positive floor ...
    refused(lambda: _ffi.set_atmosphere(ctx, (1.0, -2.0, 0.0, -5.0)), "h_floor")
    refused(lambda: _ffi.set_atmosphere(ctx, (np.nan, -2.0, 0.0, 1e5)), "finite")
    refused(lambda: rollout(DRAG | ATMO), "mpcx_set_atmosphere")                 # ... leaves the context without one
    _ffi.set_atmosphere(ctx, POWER)
    refused(lambda: rollout(J2 | ATMO), "MPCX_FLAG_DRAG")                        # the bit without drag
    with_atmo = rollout(DRAG | J2 | ATMO)
    assert with_atmo["status"][0] == 0 and not np.array_equal(with_atmo["y"], before["y"])
    # the fused step and the discretisation refuse alike, before any launch
    c = case("power_bigS")
    K = c["x"].shape[1]

    def step(flags):
        out = dict(X=np.full((1, 7, K), -7.0), U=np.full((1, 3, K), -7.0), NU=np.full((1, 7, K), -7.0), tf=np.full(1, -7.0),
                   status=np.full(1, -7, dtype=np.int32), iters=np.full(1, -7, dtype=np.int32), kkt=np.full(1, -7.0))
        try:
            _step_call(c["x"][None].copy(), c["u"][None].copy(), tf, c["const"][None].copy(), np.array([np.linalg.norm(c["x"][:3, -1])]), None, None, device=0, slot=slot,
                       out=out, opts=_ffi.make_solve_opts(), dflags=flags, max_step=1e-2)
        finally:
            step.out = out
        return out
    refused(lambda: step(ATMO), "MPCX_FLAG_DRAG")
    assert all((a == -7).all() for a in step.out.values())
    assert step(DRAG | ATMO)["status"][0] == 0
    _ffi.set_atmosphere(ctx, None)
    refused(lambda: step(DRAG | ATMO), "mpcx_set_atmosphere")
    assert all((a == -7).all() for a in step.out.values())
    after = rollout(DRAG | J2)
    assert np.array_equal(after["y"], before["y"]) and after["nsteps"][0] == before["nsteps"][0]


def test_constellation_update_with_the_atmosphere_equals_its_iterations():
    """ConstellationMPC(plan_drag=True, plan_J2=True, atmosphere=...), two segments of five satellites: the one-call update
    (the atmosphere in disc_flags, passed on to the planning rollouts, and in sim_flags) against the verbose path (one library
    call per SCP iteration, the flight as its own call) and against devices=[0, 0] (two contexts, each given the atmosphere), bit
    for bit: plan, plan_tf, plan_K and the flown sim_data; and the plan is not the fixed-density planner's."""
    import contextlib, io
    from mpconstellation_amd import Satellite, ConstellationMPC
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(4096)[[3, 500, 1234, 2222, 4000]]
    make = lambda: [Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st]
    kw = dict(base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5, sim_base_res=50, plan_drag=True, plan_J2=True, atmosphere=POWER)
    a = ConstellationMPC(make(), **kw)
    b = ConstellationMPC(make(), verbose=True, **kw)
    d = ConstellationMPC(make(), devices=[0, 0], **kw)
    ref = ConstellationMPC(make(), **{**kw, "atmosphere": None})
    for m in (a, b, d, ref):
        m.consts[1::2, C_S] *= S_SCALE
    ref.update()
    for seg in range(2):
        a.run_segment(1); d.run_segment(1)
        with contextlib.redirect_stdout(io.StringIO()):
            b.run_segment(1)
        assert (a.last_status == 0).all()
        for o in (b, d):
            assert np.array_equal(a.last_status, o.last_status)
            assert np.array_equal(a.plan_K, o.plan_K) and np.array_equal(a.plan_tf, o.plan_tf)
            for i in range(5):
                assert np.array_equal(a.plan_x[i], o.plan_x[i]) and np.array_equal(a.plan_u[i], o.plan_u[i])
                assert np.array_equal(a.plan_nu[i], o.plan_nu[i])
        if seg == 0:
            assert not np.array_equal(a.plan_tf, ref.plan_tf)
    for o in (b, d):
        for sa, so in zip(a.sats, o.sats):
            assert np.array_equal(a.sim_data[sa.id], o.sim_data[so.id]) and np.array_equal(sa.get_state_vector(), so.get_state_vector())


def test_atmosphere_aware_planner_predicts_the_flight(capsys):
    """What the model is for: 64 satellites with S x 1e4, raised to r_des = 1.02 (680 km from the Hubble's 540: the power law's
    density falls to a fifth on the way), four SCP iterations as in tests/test_drag_model_gpu.py.  The truth model flies through
    the power-law atmosphere.  One plan is made with atmosphere=, one with the fixed density; each plan's thrust table is flown
    over its own tf_u and sampled at its own nodes.  The atmosphere-aware plan's largest deviation from its own X is the smaller
    one.  The test prints both; the ratio is not known in advance and is not asserted (profiles/atmosphere_model.txt)."""
    from mpconstellation_amd import _ffi, Satellite, ConstellationMPC
    from mpconstellation_amd.constellation import constellation_states
    from mpconstellation_amd.simulator import propagate_batch
    S = 64
    states = constellation_states(S)
    make = lambda: [Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in states]
    dev = {}
    for aware in (False, True):
        mpc = ConstellationMPC(make(), base_res=30, tf_horizon=1, tf_interval=1, r_des=1.02, scp_iterations=4,
                               plan_drag=True, plan_J2=True, atmosphere=POWER if aware else None)
        mpc.consts[:, C_S] *= S_SCALE
        mpc.update()
        assert np.isin(mpc.last_status, (0, 7)).all(), mpc.last_status
        X, U, _ = mpc._plan
        Kp = mpc.plan_K
        y, st, _ = propagate_batch(mpc._y0(), mpc.plan_tf, mpc.consts, (_ffi.CTRL_SEQUENCE, U, U.shape[2], 1.0), Kp,
                                   include_drag=True, include_J2=True, Kus=Kp, atmosphere=POWER)
        assert (st == 0).all()
        dev[aware] = np.array([np.abs(y[s, :, :Kp[s]] - X[s, :, :Kp[s]]).max() for s in range(S)])
    with capsys.disabled():
        print(f"\nflight through the power-law atmosphere vs plan, max node deviation over 64 satellites: fixed-density planner "
              f"{dev[False].max():.3e} (median {np.median(dev[False]):.3e}), atmosphere-aware planner {dev[True].max():.3e} "
              f"(median {np.median(dev[True]):.3e}), ratio {dev[True].max() / dev[False].max():.3g}")
    assert dev[True].max() < dev[False].max()
