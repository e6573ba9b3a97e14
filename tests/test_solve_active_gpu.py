"""Every solve kernel against the CPU oracle with each inequality constraint ACTIVE at the solution (tests/solve_active_cases.py;
tests/test_solve_active_host.py keeps that list honest): a thrust ball saturated on most or all nodes, the r_max ball (at
K = 60 on an interior node, at K = 30 on the terminal one), r_min planes, every row of the terminal block, the terminal ball, tf_max, virtual control in use.  Each case
runs on the fixture's own A / B matrices, which the oracle gets too, through

* the sequential builds -- one-wave (flags 16), two-wave (32) and the default dispatch (0: LDS-resident up to 30 nodes): status
  0, kkt <= 1e-8, the rule of tests/test_solve_gpu.py (5e-9 on a common path, 5e-6 otherwise, iteration counts +-1), the three
  builds bit for bit alike, the iterate half way along the path to 1e-6 -- and AT MOST ONE case of the whole list off the
  common path;
* the time-parallel build (64, K >= 24): 5e-6, and 1e-9 wherever the CPU's own partitioned algebra stays within 1e-12 of its
  sequential solve (solve_active_cases.tp_tight) and the path is common and unregularised; half way 1e-6;
* the oracle's NLP functions on the device's own result: feasible to 1e-8, on the constraints the oracle has active to 1e-6;
* one ragged table launch per variant with K = 20, 30, 60 and all the option sets mixed: every satellite's bits are those of its
  own launch;
* the shared-tf solve of two satellites under a thrust limit and a mass floor.

Observed on an MI355X: see profiles/solve_active.txt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import solve_active_cases as A
from test_solve_gpu import TOL_PATH, TOL_SOL, solution_tolerance
from test_time_parallel_oracle_gpu import TOL_TP, tp_really_ran
from test_factor_loop_edges_gpu import F

pytestmark = pytest.mark.gpu
N = A.N
ONE_WAVE, TWO_WAVE, DEFAULT, TIME_PARALLEL, LINEAR_VT = 16, 32, 0, 64, 2
SEQUENTIAL = (ONE_WAVE, TWO_WAVE, DEFAULT)
FEASIBLE, ON_BOUND, DYNAMICS = 1e-8, 1e-6, 1e-8
_runs = {}


def device(cid, flags, **solver):
    """the case alone in a launch of the kernel `flags` asks for (computed once per process, shared, left unchanged)"""
    key = (cid, flags, tuple(sorted(solver.items())))
    if key not in _runs:
        from mpconstellation_amd import solve_batch
        case = A.BY_ID[cid]; d = A.fixture(case["fixture"]); q = A.quantities(d)
        _runs[key] = solve_batch(*[d[k][None] for k in A.STAGE_KEYS], d["x"][None], d["u"][None], [q["tf"]], d["const"][None],
                                 [q["rK"]], options=A.options_of(case), linear_vt=(case["variant"] == "linvt"),
                                 regularised=True, flags=flags, **solver)
    return _runs[key]


def assert_same_path_half_way(cid, flags):
    """as tests/test_solve_gpu.py::test_solve_vs_oracle: both sides stopped after half of the oracle's iterations hold the same
    iterate to TOL_PATH (unrefined directions: 1e-9 .. 1e-6 relative) -- with the constraints on their way to becoming active"""
    refc = A.reference_half_way(cid)
    resc = device(cid, flags, max_iter=refc["iters"])
    assert resc.iters[0] == refc["iters"] == A.reference(cid)[1]["iters"] // 2
    errs = errors(resc, refc)
    report(cid, f"flags {flags}, half way", resc, refc, errs, TOL_PATH)
    assert max(errs) < TOL_PATH, (flags, errs)


def errors(res, ref):
    return (np.abs(res.X[0] - ref["X"]).max(), np.abs(res.U[0] - ref["U"]).max(), np.abs(res.NU[0] - ref["NU"]).max(),
            abs(res.tf[0] - ref["tf"]))


def report(cid, what, res, ref, errs, tol):
    print(f"{cid} [{what}]: iterations {int(res.iters[0])} / oracle {ref['iters']}, regularised {int(res.n_regularised[0])} / {ref['n_regularised']}, "
          f"|dX| {errs[0]:.2e} |dU| {errs[1]:.2e} |dNU| {errs[2]:.2e} |dtf| {errs[3]:.2e} (bound {tol:.0e})")


def sequential_tolerance(cid):
    _, ref, _ = A.reference(cid)
    res = device(cid, DEFAULT)
    return solution_tolerance(ref, res.iters[0], int(res.n_regularised[0]), int(res.first_regularised[0]))


@pytest.mark.parametrize("cid", A.IDS)
def test_sequential_builds_vs_oracle(cid):
    _, ref, _ = A.reference(cid)
    assert ref["status"] == 0
    for flags in SEQUENTIAL:
        res = device(cid, flags)
        assert res.status[0] == 0 and res.kkt[0] <= 1e-8, (flags, res.status[0], res.kkt[0])
        tol = solution_tolerance(ref, res.iters[0], int(res.n_regularised[0]), int(res.first_regularised[0]))
        errs = errors(res, ref)
        report(cid, f"flags {flags}", res, ref, errs, tol)
        assert max(errs) < tol, (flags, errs)
    for flags in SEQUENTIAL[1:]:
        for f in F:
            assert np.array_equal(getattr(device(cid, SEQUENTIAL[0]), f), getattr(device(cid, flags), f)), (flags, f)
    assert_same_path_half_way(cid, DEFAULT)


def test_at_most_one_case_leaves_the_common_path():
    """the cases were chosen so that the oracle alone never leaves the common path (no regularised iteration, no marginal last
    decision): the solver-tolerance fallback of solution_tolerance is for at most one of them"""
    fallback = [cid for cid in A.IDS if sequential_tolerance(cid) == TOL_SOL]
    for cid in fallback:
        print(f"off the common path: {cid}: iterations {int(device(cid, DEFAULT).iters[0])} / oracle {A.reference(cid)[1]['iters']}")
    assert len(fallback) <= 1, fallback


@pytest.mark.parametrize("cid", A.TP_IDS)
def test_time_parallel_build_vs_oracle(cid):
    _, ref, _ = A.reference(cid)
    res = device(cid, TIME_PARALLEL)
    assert tp_really_ran(res, device(cid, DEFAULT))
    assert ref["status"] == 0 and res.status[0] == 0
    assert abs(int(res.iters[0]) - ref["iters"]) <= 1
    _, delta_part = A.partitioned(cid)
    common = ref["n_regularised"] == 0 and int(res.n_regularised[0]) == 0 and int(res.iters[0]) == ref["iters"]
    tol = TOL_TP if (A.tp_tight(cid) and common) else TOL_SOL
    errs = errors(res, ref)
    report(cid, f"time-parallel, delta_part {delta_part:.2e}", res, ref, errs, tol)
    assert max(errs) < TOL_SOL
    assert max(errs) < tol
    assert_same_path_half_way(cid, TIME_PARALLEL)


@pytest.mark.parametrize("cid", A.IDS)
def test_device_result_sits_where_the_oracle_says(cid):
    case = A.BY_ID[cid]
    P, ref, cen = A.reference(cid)
    for flags in (DEFAULT,) + ((TIME_PARALLEL,) if case["K"] >= A.TP_MIN_K else ()):
        res = device(cid, flags)
        X, U, NU, tf = res.X[0], res.U[0], res.NU[0][:, :-1], float(res.tf[0])
        g = P.ineq(X, U, NU, np.abs(NU), tf)
        worst = max(v.max() for v in g.values())
        assert worst <= FEASIBLE, (flags, {k: v.max() for k, v in g.items()})
        for family in case["declares"]:
            assert cen[family], family
            if family == "nu":
                assert np.abs(NU).max() >= A.ACTIVE_NU, flags
                continue
            at = A.family_values(g, family)[sorted(cen[family])]
            assert (at >= -ON_BOUND).all(), (flags, family, at.min())
        assert np.abs(P.dyn_residual(X, U, NU, tf)).max() < DYNAMICS, flags


# ---- neighbours with different active sets in one launch ----
def pack_stage(d):
    """the fixture's K - 1 stage records [A | Bn | Bp | Sigma | xi] (the inverse of dev_solve.unpack_stage)"""
    K = d["x"].shape[1]
    return np.concatenate([d["A"].reshape(K - 1, 49), d["Bn"].reshape(K - 1, 21), d["Bp"].reshape(K - 1, 21), d["Sigma"].T, d["xi"].T], axis=1)


def table_launch(variant, flags):
    import dev_solve as D
    from test_per_satellite_options_gpu import rows_of, sat_dev
    cases = [c for c in A.CASES if c["variant"] == variant]
    ds = [A.fixture(c["fixture"]) for c in cases]
    Ks = np.array([c["K"] for c in cases], dtype=np.int32)
    S, Kmax = len(cases), int(Ks.max())
    x = np.zeros((S, 7, Kmax)); u = np.zeros((S, 3, Kmax)); stage = np.zeros((S, Kmax - 1, D.STAGE_DOUBLES))
    for s, d in enumerate(ds):
        x[s, :, :Ks[s]] = d["x"]; u[s, :, :Ks[s]] = d["u"]; stage[s, :Ks[s] - 1] = pack_stage(d)
    P = dict(S=S, K=Kmax, Ks=Ks, x=x, u=u, tf=np.array([float(d["tf"]) for d in ds]), cst=np.stack([d["const"] for d in ds]),
             r_des=np.array([A.quantities(d)["rK"] for d in ds]))
    rows, structs = rows_of([A.options_of(c) for c in cases], np.arange(S), flags | (LINEAR_VT if variant == "linvt" else 0))
    return cases, Ks, sat_dev(P, structs[0], rows, stage=D.dev(stage))


@pytest.mark.parametrize("flags", [ONE_WAVE, TWO_WAVE], ids=["one_wave", "two_wave"])
@pytest.mark.parametrize("variant", ["linvt", "exact"])
def test_mixed_active_sets_in_one_table_launch(variant, flags):
    import dev_solve as D
    cases, Ks, table = table_launch(variant, flags)
    assert not isinstance(table, int), table
    assert len(cases) >= 6 and (variant == "exact" or set(Ks.tolist()) == {20, 30, 60})
    assert len(set(Ks.tolist())) >= 2
    for s, c in enumerate(cases):
        one = device(c["id"], flags)
        k = int(Ks[s])
        for f in F:
            a, b = table[f][s], getattr(one, f)[0]
            a = a[:, :k] if np.ndim(a) == 2 else a
            assert D.same_bits(np.asarray(a), np.asarray(b)), (c["id"], f)


# ---- two satellites, one final time ----
def test_shared_tf_under_a_thrust_limit_and_a_mass_floor():
    """solve_shared_tf(monolithic=True) against the oracle's decomposition (N.solve_shared_tf) at the tolerances of
    tests/test_solve_xcheck_gpu.py::test_shared_tf_device_vs_monolithic_fixture (convex variant): tf 1e-6, X 1e-5.  The shared-tf
    solve takes no per-satellite options, so both satellites fly under ONE set holding the thrust limit and the mass floor.
    (The oracle's root search ends after 16 evaluations of two inner solves each: the 13 s of this test are the oracle's.)"""
    from mpconstellation_amd import solve_shared_tf
    sh = A.SHARED_TF
    d = A.fixture(sh["fixture"]); q = A.quantities(d)
    Ps = A.shared_tf_problems()
    tf_o, out, ev = N.solve_shared_tf(Ps, 5.0)
    assert all(r["status"] == 0 for r in out) and len(ev) <= 40
    for P, r in zip(Ps, out):
        cen = A.census(P, r)
        assert all(cen[f] for f in sh["declares"]), {f: sorted(v) for f, v in cen.items() if v}
    two = lambda a: np.stack([a, a])
    u = np.stack([d["u"] * f for f in sh["u_scales"]])
    res, search = solve_shared_tf(*[two(d[k]) for k in A.STAGE_KEYS], two(d["x"]), u, np.full(2, q["tf"]), two(d["const"]), np.full(2, q["rK"]),
                                  options=sh["options"](q), linear_vt=True, monolithic=True)
    assert (res.status == 0).all() and search.converged and len(search) == 0
    assert res.tf[0] == res.tf[1] and res.iters[0] == res.iters[1] and res.kkt[0] == res.kkt[1] <= 1e-8
    print(f"shared tf: device {res.tf[0]:.9f} ({int(res.iters[0])} iterations) / oracle {tf_o:.9f} ({len(ev)} evaluations), "
          f"|dX| {max(np.abs(res.X[s] - out[s]['X']).max() for s in range(2)):.2e}")
    assert abs(res.tf[0] - tf_o) < 1e-6
    for s in range(2):
        assert np.abs(res.X[s] - out[s]["X"]).max() < 1e-5
        g = Ps[s].ineq(res.X[s], res.U[s], res.NU[s][:, :-1], np.abs(res.NU[s][:, :-1]), float(res.tf[s]))
        assert max(v.max() for v in g.values()) <= FEASIBLE
        # the mass floor is a bound on one entry of x_K: within 1e-5 of the oracle's x, the device sits on it to 1e-5 + 1e-6
        assert A.family_values(g, "term5")[0] >= -(1e-5 + ON_BOUND), s