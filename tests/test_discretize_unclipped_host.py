"""The discretisation oracle (oracle/discretize.c) against the reference's own Discretizer at ivp_max_step = 1: the anchor of
tests/test_discretize_unclipped_gpu.py, which holds discretize_kernel to that oracle on the same list of inputs
(tests/discretize_cases.py).

tests/golden/discretize_unclipped.npz holds what the reference computes for every (case, mode) of discretize_cases.ANCHORED
(tests/golden/make_discretize_unclipped_golden.py; the inputs are rebuilt here and must hash to what the generator used).  The
oracle must take the reference's steps -- the same accepted nodes and the same number of right-hand sides per interval, rejected
attempts included -- and return its arrays: the same arithmetic in another order, so the difference is rounding, and the
tolerance the device is held to must be at least ten times it.  The conditions that make each input worth a launch (rejections
beside clean intervals in a wave, steps with no and with several uniform points, steps across columns of the thrust table, drag
that matters, no acceptance knife edge) and the guard against a tolerance that another step sequence would pass are asserted here
as well, without a device."""
import os

import numpy as np
import pytest

import discretize_cases as C
import oracle_lib as O


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "discretize_unclipped.npz"))
    assert [tuple(p.rsplit(".", 1)) for p in g["pairs"]] == C.ANCHORED
    return g


def reference_arrays(g, name, mode):
    """per satellite the five arrays of the fixture, cut to the satellite's own intervals"""
    c, tag = C.case(name), f"{name}.{mode}"
    out = []
    for s, k in enumerate(c["Ks"]):
        r = {key: g[f"{key}_{tag}"][s] for key in C.KEYS}
        out.append({key: (v[:, :k - 1] if key in ("Sigma", "xi") else v[:k - 1]) for key, v in r.items()})
    return out


@pytest.mark.parametrize("name,mode", C.ANCHORED, ids=lambda v: str(v))
def test_oracle_reproduces_the_reference(golden, name, mode):
    c, tag = C.case(name), f"{name}.{mode}"
    assert C.input_hash(name) == str(golden[f"inputs_sha256_{name}"]), "the fixture was computed from other inputs: run the generator"
    outs = C.oracle(name, mode)
    assert all(o["status"] == 0 for o in outs)
    tol = C.tolerance(name, mode)                       # (guard (i) is asserted inside, before anything is compared)
    errs = C.errors(outs, reference_arrays(golden, name, mode))
    worst = max(errs.values())
    print(f"{name} {mode}: oracle against the reference {worst:.3g} ({', '.join(f'{k} {e:.3g}' for k, e in errs.items())}); tolerance {tol:.3g}, "
          f"smallest distance to max_step = 1e-2 {min(C.clipped_gap(name, mode)):.3g}")
    assert 10.0 * worst <= tol, (name, mode, worst, tol)                    # guard (ii)
    if not C.MODES[mode][1]:
        for s, (o, k) in enumerate(zip(outs, c["Ks"])):
            assert np.array_equal(o["node_counts"], golden[f"node_counts_{tag}"][s][:k - 1]), (s, o["node_counts"])
            assert np.array_equal(o["node_nfev"], golden[f"nfev_{tag}"][s][:k - 1]), (s, o["node_nfev"])


@pytest.mark.parametrize("name,mode", C.ANCHORED + [("drag-general-k4", "rk23")], ids=lambda v: str(v))
def test_input_conditions(name, mode):
    rec = C.check_conditions(name, mode)
    print(f"{name} {mode}: accepted {rec['accepted']}, rejected {rec['rejected']}, largest step {rec['largest_step']:.3g} over {rec['table_intervals']} "
          f"table intervals, uniform points per step {rec.get('points')}, cond {rec['cond']:.3g}, drag share {rec.get('drag_share')}, "
          f"against the fixed density {rec.get('against_fixed')}, tolerance {C.tolerance(name, mode):.3g}, distances to max_step = 1e-2 "
          f"{['%.2g' % g for g in C.clipped_gap(name, mode)]}")


def test_rk45_rejects_in_mixed_waves_under_the_uniform_points():
    """the uniform modes of the plain cases ride on RK45's steps: 7 to 11 per interval, a third of the intervals with a rejected
    attempt, a rejecting interval beside clean ones in every wave"""
    for name in C.PLAIN:
        accepted, rejected = C.counts(name, "uni33")
        assert 7 <= accepted.min() and accepted.max() <= 11 and (rejected > 0).sum() >= 5
        assert all((w > 0).any() and (w == 0).any() for w in (rejected[0:8], rejected[8:16], rejected[16:21]))


@pytest.mark.parametrize("max_step", (float("inf"), 2.0))
def test_max_step_above_the_interval_is_max_step_one(max_step):
    """no interval is longer than 1: the oracle's bits at max_step = inf (scipy's default) and 2 are those of max_step = 1"""
    for name, mode in C.ANCHORED:
        for a, b in zip(C.oracle(name, mode), C.oracle(name, mode, max_step)):
            assert all(np.array_equal(a[k], b[k]) for k in C.KEYS + ("node_counts", "node_nfev")), (name, mode)


def test_oracle_refuses_a_node_that_is_not_finite():
    """scipy raises on such a y0 (the reference's discretize dies of it); the oracle reports it for that satellite instead of
    shrinking a NaN step for ever, and the device's code for it is MPCX_ST_STEP"""
    solve_ivp = pytest.importorskip("scipy.integrate").solve_ivp
    c = C.case("plain")
    x = C.bad_x(c)
    with pytest.raises(ValueError):
        solve_ivp(lambda t, y: y, (0.0, 1.0), x[C.BAD_SAT][:, C.BAD_NODE])
    status = [o["status"] for o in C.run_oracle(c, "rk23", x=x)]
    assert status == [O.ST_START_NOT_FINITE if s == C.BAD_SAT else 0 for s in range(c["S"])]
    assert O.DEVICE_STATUS[O.ST_START_NOT_FINITE] == 2
