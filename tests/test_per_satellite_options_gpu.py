"""Per-satellite problem options (include/mpcx.h, the *_sat entry points and MPCX_PO_*): one launch whose satellites are posed
with different option sets must give every satellite, bit for bit, what a launch with its set as the scalar options gives
it -- on every kernel, in every launch order, in both chains of a split update, on several devices -- and a table whose rows
all equal the scalar options must give the bits of the call without a table.

The option sets are three lines of profiles/r02/edge_cases.txt that ended with status 0 for every satellite: A the defaults,
B OptimalController's set (eps_r 1e-6, eps_vr 1e-16, tf_max = tf_bar), C a thrust limit of 0.3 with min_mass 0.999, another
r_lim and doubled w_tr; dealt out by s % 3 so that neighbours differ.  The CPU oracle (oracle/nlp_ipm.py, one MpcProblem per
satellite with its own options) ends every problem used here with status 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))

pytestmark = pytest.mark.gpu

FIELDS = ("X", "U", "NU", "tf", "status", "iters", "kkt", "n_regularised", "first_regularised")
RAGGED = ["tan_K30_tf1", "tan_K20_tf2", "tan_K30_tf1", "tan_K20_tf2", "tan_K20_tf2", "tan_K30_tf1"]      # counts 30 and 20 mixed; set B on tf_bar = 2
RECT = ["tan_K30_tf1"] * 6                                                                                 # the time-parallel kernel: 30 nodes
ONE_WAVE, NO_LDS, TIME_PARALLEL, FIXED_TF, SHARED_TF = 16, 32, 64, 4, 8


def option_sets(tf_bar):
    """A, B, C; tf_bar: the reference final time of the satellites that get set B"""
    return [{}, {"eps_r": 1e-6, "eps_vr": 1e-16, "tf_max": tf_bar},
            {"u_lim": [0, 0.3], "min_mass": 0.999, "r_lim": [1.0, 4.0], "w_tr": 0.004}]


def problems(golden_dir, names):
    """as tests/test_ragged_gpu.py::padded, every satellite a little different: thrust scaled, target radius moved"""
    ds = [np.load(os.path.join(golden_dir, f"disc_{n}.npz")) for n in names]
    Ks = np.array([d["x"].shape[1] for d in ds], dtype=np.int32)
    Kmax, S = int(Ks.max()), len(ds)
    x = np.zeros((S, 7, Kmax)); u = np.zeros((S, 3, Kmax))
    for s, d in enumerate(ds):
        x[s, :, :Ks[s]] = d["x"]; u[s, :, :Ks[s]] = d["u"] * (1.0 + 0.01 * s)
    tf = np.array([float(d["tf"]) for d in ds]); cst = np.stack([d["const"] for d in ds])
    r_des = np.array([np.linalg.norm(d["x"][:3, -1]) + 1e-4 * s for s, d in enumerate(ds)])
    sets = option_sets(2.0 if names is RAGGED else 1.0)
    return dict(S=S, K=Kmax, Ks=Ks, x=x, u=u, tf=tf, cst=cst, r_des=r_des, sets=sets, which=np.arange(S) % 3)


def rows_of(sets, which, flags=0):
    """the table [S][MPCX_NPOPT]: row s = the eleven problem options of the struct make_solve_opts builds for set which[s]"""
    from mpconstellation_amd import _ffi
    structs = [_ffi.make_solve_opts(o, flags=flags) for o in sets]
    rows = np.array([[getattr(o, f) for f in _ffi.PO_FIELDS] for o in structs])
    return np.ascontiguousarray(rows[which]), structs


def options_of(sets, which):
    """the same table as an options dict of per-satellite arrays (what the Python wrappers take)"""
    from mpconstellation_amd.optimizer import DEFAULT_OPTIONS
    keys = sorted(set().union(*[set(o) for o in sets]))
    return {k: np.array([sets[j].get(k, DEFAULT_OPTIONS[k]) for j in which], dtype=np.float64) for k in keys}


def sat_dev(P, opts, popts, step=False, Ks=True, ctx_slot=0, tf_in=None, stage=None):
    """mpcx_solve_batch_ragged_sat_dev (on the stage records `stage`) or mpcx_mpc_step_batch_ragged_sat_dev -> results dict"""
    import torch
    import dev_solve as D
    from mpconstellation_amd import _ffi
    lib = _ffi.load(); ctx = _ffi.context(0, ctx_slot)
    S, K = P["S"], P["K"]
    x, u = D.dev(P["x"]), D.dev(P["u"])
    hold = [D.dev(P["tf"]), D.dev(P["cst"]), D.dev(P["r_des"]), D.dev(P["Ks"], torch.int32) if Ks else None,
            None if popts is None else D.dev(popts)]
    out = D.Outputs(S, K)
    if tf_in is not None:
        out.tf.copy_(D.dev(tf_in))
    st = D._stream(torch)
    if step:
        ws = D.filled(D.step_workspace_doubles(S, K), "zero")
        rc = lib.mpcx_mpc_step_batch_ragged_sat_dev(ctx, S, K, D._p(hold[3]), D._p(x), D._p(u), D._p(hold[0]), D._p(hold[1]), D._p(hold[2]), 0, 1e-2,
                                                    C.byref(opts), D._p(hold[4]), D._p(out.X), D._p(out.U), D._p(out.NU), D._p(out.tf),
                                                    D._p(out.status), D._p(out.iters), D._p(out.kkt), D._p(ws), st)
    else:
        ws = D.filled(D.solver_workspace_doubles(S, K), "zero")
        rc = lib.mpcx_solve_batch_ragged_sat_dev(ctx, S, K, D._p(hold[3]), D._p(stage), D._p(x), D._p(u), D._p(hold[0]), D._p(hold[1]), D._p(hold[2]),
                                                 C.byref(opts), D._p(hold[4]), D._p(out.X), D._p(out.U), D._p(out.NU), D._p(out.tf),
                                                 D._p(out.status), D._p(out.iters), D._p(out.kkt), D._p(ws), st)
    if rc != 0:
        torch.cuda.synchronize()
        return rc
    _ffi.check(lib.mpcx_solve_regularised_dev(ctx, S, D._p(out.reg), st), ctx, "solve_regularised_dev")
    torch.cuda.synchronize()
    return out.numpy()


def assert_sat_bits(a, s, b, what):
    import dev_solve as D
    for f in FIELDS:
        assert D.same_bits(a[f][s], b[f][s]), (what, s, f)


_cache = {}


def stages(golden_dir, names):
    """the problems and their stage records on the device (discretised once per session)"""
    key = tuple(names)
    if key not in _cache:
        import dev_solve as D
        P = problems(golden_dir, RAGGED if names == RAGGED else RECT)
        stage, dst = D.discretize_stages(P["x"], P["u"], P["tf"], P["cst"], Ks=P["Ks"], Kus=P["Ks"])
        assert (dst == 0).all()
        _cache[key] = (P, stage)
    return _cache[key]


def table_and_scalar_runs(golden_dir, names, flags, step):
    """the table launch and the three scalar launches of one kernel, computed once and shared by the tests below"""
    key = (tuple(names), flags, step)
    if key not in _cache:
        P, stage = stages(golden_dir, names)
        rows, structs = rows_of(P["sets"], P["which"], flags)
        table = sat_dev(P, structs[0], rows, step=step, stage=stage)
        scalar = [sat_dev(P, o, None, step=step, stage=stage) for o in structs]
        _cache[key] = (P, rows, structs, table, scalar)
    return _cache[key]


@pytest.mark.parametrize("step", [False, True], ids=["solve", "fused_step"])
@pytest.mark.parametrize("flags", [0, ONE_WAVE, NO_LDS], ids=["default", "one_wave", "no_lds"])
def test_table_equals_scalar_launches(golden_dir, flags, step):
    P, rows, structs, table, scalar = table_and_scalar_runs(golden_dir, RAGGED, flags, step)
    assert (table["status"] == 0).all(), table["status"]
    assert len(set(P["Ks"].tolist())) == 2
    for s in range(P["S"]):
        assert_sat_bits(table, s, scalar[P["which"][s]], (flags, step))
    # the sets really pose different problems: a satellite under another set has other bits
    assert not np.array_equal(scalar[0]["X"][1], scalar[1]["X"][1]) and not np.array_equal(scalar[0]["X"][2], scalar[2]["X"][2])


def test_table_equals_scalar_launches_time_parallel(golden_dir):
    P, rows, structs, table, scalar = table_and_scalar_runs(golden_dir, RECT, TIME_PARALLEL, False)
    _, _, _, plain, _ = table_and_scalar_runs(golden_dir, RECT, 0, False)
    assert not np.array_equal(table["X"], plain["X"])             # the flag took the time-parallel kernel: not the other kernels' bits
    assert (table["status"] == 0).all() and (plain["status"] == 0).all()
    for s in range(P["S"]):
        assert_sat_bits(table, s, scalar[P["which"][s]], "tp")


@pytest.mark.parametrize("flags", [0, ONE_WAVE, NO_LDS, TIME_PARALLEL, FIXED_TF], ids=["default", "one_wave", "no_lds", "time_parallel", "fixed_tf"])
def test_uniform_table_equals_null(golden_dir, flags):
    """every set as the scalar options of the whole batch, with and without a table of equal rows.  The batches are the ones
    the oracle ends with status 0 under that set for EVERY satellite: free tf, all three sets on both batches; tf held at 0.9
    tf_bar, all three on the 30-node batch and A, B on the ragged one (set C's thrust limit of 0.3 cannot fly the 20-node
    fixtures' transfer in a fixed time: the oracle stops at max_iter there, so that combination is not posed)."""
    import dev_solve as D
    from mpconstellation_amd import _ffi
    cases = {TIME_PARALLEL: [(RECT, (0, 1, 2))], FIXED_TF: [(RECT, (0, 1, 2)), (RAGGED, (0, 1))]}.get(flags, [(RAGGED, (0, 1, 2))])
    for names, js in cases:
        P, stage = stages(golden_dir, names)
        tf_in = 0.9 * P["tf"] if flags == FIXED_TF else None
        for j in js:
            opts = _ffi.make_solve_opts(P["sets"][j], flags=flags)
            rows = np.ascontiguousarray(np.tile([getattr(opts, f) for f in _ffi.PO_FIELDS], (P["S"], 1)))
            for step in (False, True):
                null = sat_dev(P, opts, None, step=step, tf_in=tf_in, stage=stage)
                uni = sat_dev(P, opts, rows, step=step, tf_in=tf_in, stage=stage)
                assert np.isin(null["status"], (0, 7)).all(), (j, null["status"])
                for f in FIELDS:
                    assert D.same_bits(null[f], uni[f]), (flags, j, step, f)
    if flags == TIME_PARALLEL:
        assert not np.array_equal(null["X"], sat_dev(P, _ffi.make_solve_opts(P["sets"][2]), None, step=True, stage=stage)["X"])


def test_table_launch_against_the_oracle(golden_dir):
    """every satellite of the table launch against the oracle solved under that satellite's own options, on the device's own
    stage records: the rule of tests/test_solve_gpu.py -- rounding level where the iteration paths coincide (neither side
    regularised, or both alike), the solver tolerance otherwise"""
    from test_solve_gpu import oracle_solve, solution_tolerance
    from dev_solve import unpack_stage
    P, rows, structs, table, scalar = table_and_scalar_runs(golden_dir, RAGGED, 0, False)
    _, stage = stages(golden_dir, RAGGED)
    for s in range(P["S"]):
        k = int(P["Ks"][s])
        x, u = P["x"][s][:, :k], P["u"][s][:, :k]
        _, ref = oracle_solve(x, u, float(P["tf"][s]), P["cst"][s], float(P["r_des"][s]), unpack_stage(stage, s, k),
                              options=dict(P["sets"][P["which"][s]]))
        assert ref["status"] == 0 and table["status"][s] == 0, s
        tol = solution_tolerance(ref, table["iters"][s], int(table["n_regularised"][s]), int(table["first_regularised"][s]))
        assert np.abs(table["X"][s][:, :k] - ref["X"]).max() < tol and np.abs(table["U"][s][:, :k] - ref["U"]).max() < tol, s
        assert np.abs(table["NU"][s][:, :k] - ref["NU"]).max() < tol and abs(table["tf"][s] - ref["tf"]) < tol, s


def test_constraint_terms_per_satellite(golden_dir):
    from mpconstellation_amd.optimizer import constraint_terms_batch
    P = problems(golden_dir, RECT)
    which = P["which"]
    aT, bT, sc = constraint_terms_batch(P["x"], P["cst"], P["r_des"], options_of(P["sets"], which))
    for j, o in enumerate(P["sets"]):
        a1, b1, s1 = constraint_terms_batch(P["x"], P["cst"], P["r_des"], o)
        for s in np.flatnonzero(which == j):
            assert np.array_equal(aT[s], a1[s]) and np.array_equal(bT[s], b1[s]) and np.array_equal(sc[s], s1[s]), (j, s)
    assert not np.array_equal(bT[0], bT[1]) and not np.array_equal(sc[0], sc[2]) and (sc[:, 7] <= 0).all()
    # one satellite with r_min > r_max: its structural violation is positive, its neighbours' rows are untouched
    opt = options_of(P["sets"], which)
    opt["r_lim"] = opt["r_lim"].copy(); opt["r_lim"][3] = [2.0, 1.5]
    a2, b2, s2 = constraint_terms_batch(P["x"], P["cst"], P["r_des"], opt)
    assert s2[3, 7] > 0 and (np.delete(s2[:, 7], 3) <= 0).all()
    keep = np.arange(P["S"]) != 3
    assert np.array_equal(a2[keep], aT[keep]) and np.array_equal(b2[keep], bT[keep]) and np.array_equal(s2[keep], sc[keep])


@pytest.mark.parametrize("empty", ["r_min > r_max", "tf_max <= 0", "window outside r_max"])
def test_empty_set_for_one_satellite(golden_dir, empty):
    from mpconstellation_amd import _ffi
    P, rows, structs, table, scalar = table_and_scalar_runs(golden_dir, RAGGED, 0, True)
    bad = 4
    rows = rows.copy()
    if empty == "r_min > r_max": rows[bad, _ffi.PO_R_MIN], rows[bad, _ffi.PO_R_MAX] = 2.0, 1.5
    elif empty == "tf_max <= 0": rows[bad, _ffi.PO_TF_MAX] = -1.0
    else: rows[bad, _ffi.PO_R_MAX] = 0.5 * P["r_des"][bad]
    res = sat_dev(P, structs[0], rows, step=True)
    assert res["status"][bad] == 8 and res["iters"][bad] == 0 and res["kkt"][bad] > 0
    assert np.array_equal(res["X"][bad], P["x"][bad]) and np.array_equal(res["U"][bad], P["u"][bad]) and not res["NU"][bad].any()
    assert res["tf"][bad] == P["tf"][bad]
    for s in range(P["S"]):
        if s != bad:
            assert_sat_bits(res, s, table, empty)


def test_indexing_under_launch_order_and_split():
    """S just above the device's slot count, 8 nodes: the second of two fused steps on one context runs longest first (workgroup
    b solves satellite order[b]), and MPCX_UPDATE_SPLIT=1 runs the update as two chains of half the batch -- the table is indexed
    by SATELLITE in both"""
    import dev_solve as D
    from mpconstellation_amd import _ffi, mpc_update_batch, propagate_batch
    from mpconstellation_amd.constellation import constellation_states, normalize_batch
    S = D.n_slots() + 64
    base_res, horizon = 4, 2.0
    K = int(base_res * horizon)
    assert K == 8
    y0, cst = normalize_batch(constellation_states(S))
    x, _, _, u = propagate_batch(y0, horizon, cst, (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None), K, thrust=True)
    sets = option_sets(horizon)
    which = np.arange(S) % 3
    P = dict(S=S, K=K, Ks=np.full(S, K, dtype=np.int32), x=x, u=u, tf=np.full(S, horizon), cst=cst, r_des=np.full(S, 1.5))
    rows, structs = rows_of(sets, which)
    runs = []
    for slot, (opts, popts) in enumerate([(structs[0], rows)] + [(o, None) for o in structs]):
        _ffi.context(0, 30 + slot)                                  # a fresh context per run: no launch-order state inherited
        runs.append([sat_dev(P, opts, popts, step=True, Ks=False, ctx_slot=30 + slot) for _ in range(2)])
    assert len(set(runs[0][0]["iters"].tolist())) > 1                # iteration counts differ: the second launch really is reordered
    for call in (0, 1):
        for j in range(3):
            sel = which == j
            for f in FIELDS:
                assert D.same_bits(runs[0][call][f][sel], runs[1 + j][call][f][sel]), (call, j, f)
    for f in FIELDS:
        assert D.same_bits(runs[0][0][f], runs[0][1][f]), f
    # the update as two chains: each half gets the rows of ITS satellites
    fields = ("X", "U", "NU", "tf", "status", "iters", "kkt", "Ks", "prop_status")
    old = os.environ.get("MPCX_UPDATE_SPLIT")
    try:
        os.environ["MPCX_UPDATE_SPLIT"] = "1"
        upd = mpc_update_batch(y0, horizon, cst, 1.5, base_res, options=options_of(sets, which))
        one = [mpc_update_batch(y0, horizon, cst, 1.5, base_res, options=o) for o in sets]
        os.environ["MPCX_UPDATE_SPLIT"] = "0"
        whole = mpc_update_batch(y0, horizon, cst, 1.5, base_res, options=options_of(sets, which))
    finally:
        if old is None: os.environ.pop("MPCX_UPDATE_SPLIT", None)
        else: os.environ["MPCX_UPDATE_SPLIT"] = old
    of_set = lambda a, j: a[:, which == j] if a.shape[0] != S else a[which == j]       # (status, iters: (n_scp, S))
    for f in fields:
        assert np.array_equal(getattr(upd, f), getattr(whole, f)), f
        for j in range(3):
            assert np.array_equal(of_set(getattr(upd, f), j), of_set(getattr(one[j], f), j)), (f, j)


def test_shared_tf_takes_no_table(golden_dir):
    from mpconstellation_amd import _ffi, solve_batch, mpc_step_batch
    P, stage = stages(golden_dir, RECT)
    rows, structs = rows_of(P["sets"], P["which"], SHARED_TF)
    assert sat_dev(P, structs[0], rows, Ks=False, stage=stage) == -2                    # MPCX_E_BADARG
    assert b"per-satellite" in _ffi.load().mpcx_last_error(_ffi.context(0))
    ok = sat_dev(P, structs[0], None, Ks=False, stage=stage)                            # ... and without the table the launch runs
    assert not isinstance(ok, int) and len(set(ok["tf"].tolist())) == 1
    opt = options_of(P["sets"], P["which"])
    d = np.load(os.path.join(golden_dir, "disc_tan_K30_tf1.npz"))
    five = [np.repeat(d[k][None], P["S"], axis=0) for k in ("A", "Bp", "Bn", "Sigma", "xi")]
    with pytest.raises(ValueError):
        solve_batch(*five, P["x"], P["u"], P["tf"], P["cst"], P["r_des"], options=opt, shared_tf=True)
    with pytest.raises(ValueError):
        mpc_step_batch(P["x"], P["u"], P["tf"], P["cst"], P["r_des"], options=opt, shared_tf=True)


def test_constellation_mpc_physical_limits():
    """three satellites at different radii and masses under ONE physical keep-out radius and ONE engine: a different normalised
    r_min and thrust limit for each (normalised_limits), in one call and in verbose mode"""
    import contextlib, io
    from mpconstellation_amd import Satellite, SatelliteScale, ConstellationMPC
    from mpconstellation_amd.constellation import R_HUBBLE, V_HUBBLE
    from mpconstellation_amd.constellation_mpc import normalised_limits
    spec = [(1.0, 12200.0), (1.04, 8000.0), (1.08, 5000.0)]
    make = lambda: [Satellite(R_HUBBLE * g, V_HUBBLE / np.sqrt(g), m) for g, m in spec]
    scales = [SatelliteScale(sat=s) for s in make()]
    limits = normalised_limits(scales, r_min=0.99 * np.linalg.norm(R_HUBBLE), u_max=3000.0)
    assert len(set(limits["r_lim"][:, 0].tolist())) == 3 and len(set(limits["u_lim"][:, 1].tolist())) == 3
    kw = dict(base_res=15, tf_horizon=2, tf_interval=1, r_des=1.2, sim_base_res=40)
    a = ConstellationMPC(make(), options=limits, **kw)
    b = ConstellationMPC(make(), options=limits, verbose=True, **kw)
    a.update()
    with contextlib.redirect_stdout(io.StringIO()):
        b.update()
    assert np.isin(a.last_status, (0, 7)).all(), a.last_status
    assert np.array_equal(a.last_status, b.last_status) and np.array_equal(a.last_iters, b.last_iters)
    assert np.array_equal(a.plan_K, b.plan_K) and np.array_equal(a.plan_tf, b.plan_tf)
    for i in range(3):
        assert np.array_equal(a.plan_x[i], b.plan_x[i]) and np.array_equal(a.plan_u[i], b.plan_u[i]) and np.array_equal(a.plan_nu[i], b.plan_nu[i])
        # the satellite alone, its row as the scalar options
        row = {"r_lim": limits["r_lim"][i].tolist(), "u_lim": limits["u_lim"][i].tolist()}
        c = ConstellationMPC([make()[i]], options=row, time_parallel=False, **kw)
        c.update()
        assert np.array_equal(c.last_status[:, 0], a.last_status[:, i]) and c.plan_K[0] == a.plan_K[i] and c.plan_tf[0] == a.plan_tf[i]
        assert np.array_equal(c.plan_x[0], a.plan_x[i]) and np.array_equal(c.plan_u[0], a.plan_u[i]) and np.array_equal(c.plan_nu[0], a.plan_nu[i])
        # its own thrust limit, to the bound relaxation
        bnd = limits["u_lim"][i, 1] ** 2
        assert ((a.plan_u[i] ** 2).sum(axis=0) <= bnd + 1e-8 * max(1.0, bnd)).all(), i
    plain = ConstellationMPC(make(), **kw)
    plain.update()
    assert plain.options == {} and a.options is not limits


def test_several_devices_with_a_table(golden_dir):
    from mpconstellation_amd import mpc_step_batch, mpc_update_batch
    from mpconstellation_amd.constellation import constellation_states, normalize_batch
    P = problems(golden_dir, RAGGED)
    opt = options_of(P["sets"], P["which"])
    one = mpc_step_batch(P["x"], P["u"], P["tf"], P["cst"], P["r_des"], options=opt, Ks=P["Ks"], regularised=True)
    two = mpc_step_batch(P["x"], P["u"], P["tf"], P["cst"], P["r_des"], options=opt, Ks=P["Ks"], regularised=True, devices=[0, 0])
    assert (one.status == 0).all()
    for f in ("X", "U", "NU", "tf", "status", "iters", "kkt", "n_regularised", "first_regularised"):
        assert np.array_equal(getattr(one, f), getattr(two, f)), f
    # the host-pointer wrapper gives what the device-pointer entry point gives
    _, _, _, table, _ = table_and_scalar_runs(golden_dir, RAGGED, 0, True)
    assert np.array_equal(one.X, table["X"]) and np.array_equal(one.tf, table["tf"]) and np.array_equal(one.iters, table["iters"])
    st = constellation_states(4096)[[1, 100, 900, 1500, 2500]]
    y0, cst = normalize_batch(st)
    opt = options_of(option_sets(2.0), np.arange(5) % 3)
    u1 = mpc_update_batch(y0, 2.0, cst, 1.5, 15, options=opt)
    u2 = mpc_update_batch(y0, 2.0, cst, 1.5, 15, options=opt, devices=[0, 0])
    for f in ("X", "U", "NU", "tf", "status", "iters", "kkt", "Ks", "prop_status"):
        assert np.array_equal(getattr(u1, f), getattr(u2, f)), f
