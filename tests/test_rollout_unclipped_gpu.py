"""propagate_kernel (csrc/propagate.hip) against the CPU oracle where max_step does not clip its steps.

Every other device test of the rollout flies at max_step = 1e-3, where each step is max_step long and the kernel's controller runs
two shortcuts (`surely_small`, and the step that keeps its size).  Here max_step is 1, inf, 2 or 0.05: the step factor with its pow,
rejected attempts and the factor's cap after them, the shorter last step, several output points per step, quads of one wave on
different step sequences, thrust tables whose intervals and whose end fall between the stages of one step.  The inputs, the
oracle's counts for them and the tolerance are those of tests/rollout_cases.py, which tests/test_rollout_unclipped_host.py
anchors to scipy without a device: per case

    tol = 4 2^-52 6 (accepted + rejected) kappa max(1, |y|_inf)

with kappa the oracle's own amplification of a change in y0 (all three factors the largest of the case's satellites:
rollout_cases.case_tolerance), asserted below 1e-8 and 1e3 times below what another step sequence moves the output by.  The
accepted-step counts must be the oracle's.  Measured on an MI355X: profiles/rollout_unclipped.txt."""
import numpy as np
import pytest

import rollout_cases as R

pytestmark = pytest.mark.gpu
ST_STEP = 2                      # MPCX_ST_STEP (include/mpcx.h)


def device_flight(case, max_step=None, thrust=False, y0=None):
    """the case as one launch of the public wrapper -> y (S,7,n), status, nsteps[, u (S,3,n)]"""
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.simulator import propagate_batch
    law = {"zero": lambda: (_ffi.CTRL_ZERO, None, 0, None), "constant": lambda: (_ffi.CTRL_CONSTANT, case["constant"], 0, None),
           "tangential": lambda: (_ffi.CTRL_TANGENTIAL, case["tangential"], 0, None),
           "sequence": lambda: (_ffi.CTRL_SEQUENCE, case["table"], case["table"].shape[2], case["end_tau"])}[case["law"]]()
    return propagate_batch(case["y0"] if y0 is None else y0, case["tf"], case["const"], law, case["n_eval"], include_drag=bool(case["flags"] & R.DRAG),
                           include_J2=bool(case["flags"] & R.J2), max_step=case["max_step"] if max_step is None else max_step, thrust=thrust,
                           atmosphere=case["atmosphere"])


def hold_to_oracle(case, y, st, ns):
    """status 0, the oracle's accepted steps, every satellite's samples within the case's bound (exactly the start state where
    there is one output point); prints the record of profiles/rollout_unclipped.txt -> the worst error / bound of the case"""
    tol = R.case_tolerance(case, R.DEVICE_ULPS)              # (with its conditions, before anything of the device is looked at)
    ref = R.reference(case)
    errs = np.array([np.abs(y[s, :, :R.n_eval_of(case, s)] - r["y"]).max() for s, r in enumerate(ref)])
    tols = np.array([R.tolerance_of(case, s, tol) for s in range(case["S"])])
    for s, r in enumerate(ref):
        print(f"{case['name']}: satellite {s}: accepted {r['accepted']} (device {ns[s]}) rejected {r['rejected']} kappa {r['kappa']:.3g} "
              f"own figure {R.own_bound(r, R.DEVICE_ULPS):.3g} error {errs[s]:.3g}")
    ratio = errs.max() / tol if tol > 0 else 0.0
    print(f"{case['name']}: tolerance {tol:.3g}, worst error {errs.max():.3g} = {ratio:.3g} of it")
    assert (st == 0).all(), st
    assert np.array_equal(ns, [r["accepted"] for r in ref]), (ns, R.counts(case)[0])
    assert (errs <= tols).all(), (errs, tols)
    return ratio


@pytest.fixture(scope="module")
def mixed():
    """(a) and its launch at max_step = 1, which (c) and (f) compare theirs with"""
    case = R.mixed_waves()
    R.check_mixed_waves(case)
    return (case,) + tuple(device_flight(case))


def test_mixed_waves(mixed):
    """S = 21: a full wave of 16 quads and one with five; twelve satellites reject up to six attempts and nine none, both kinds in
    the first wave, whose quads finish after 3 to 21 accepted steps; tables of five columns under steps that span several of
    them, a third of them ending at 0.6 or 0.37 between two stages"""
    case, y, st, ns = mixed
    acc, rej = R.counts(case)
    print(f"accepted {acc.tolist()}, rejected {rej.tolist()}")
    hold_to_oracle(case, y, st, ns)


@pytest.mark.parametrize("n_eval", R.SHORT_N_EVALS, ids=str)
def test_all_output_points_in_two_steps(n_eval):
    """tf = 1e-4: two accepted steps hold every output point -- 1, 2, 3 or 40 of them, and a ragged launch of (1, 40, 3), whose columns
    past a satellite's count stay zero; u_out from the same launch against the host form of the hold (SequenceController, and
    foh_reference where the table spans the flight), at the existing test's tolerance; two tables end inside a step"""
    from mpconstellation_amd.control import SequenceController
    from foh_reference import foh_resample_ragged
    case = R.dense_points(R.SHORT_TF, n_eval)
    acc, _ = R.counts(case)
    assert (acc == 2).all()
    y, st, ns, u = device_flight(case, thrust=True)
    hold_to_oracle(case, y, st, ns)
    y_plain, _, ns_plain = device_flight(case)
    assert np.array_equal(y, y_plain) and np.array_equal(ns, ns_plain)
    nmax = y.shape[2]
    for s in range(case["S"]):
        n = R.n_eval_of(case, s)
        assert (y[s, :, n:] == 0.0).all() and (u[s, :, n:] == 0.0).all()
        if n == 1:
            assert np.array_equal(y[s, :, 0], case["y0"][s])
        ctrl = SequenceController(u=case["table"][s])
        ctrl.end_tau = float(case["end_tau"][s])
        u_func = ctrl.get_u_func()
        want = np.stack([u_func(None, tau) for tau in np.linspace(0, 1, n)], axis=1)
        assert np.abs(u[s, :, :n] - want).max() <= 1e-15 * max(1.0, np.abs(want).max()), (s, n)
        if n > 1 and case["end_tau"][s] < 1.0:
            assert (u[s, :, n - 1] == 0.0).all() and np.abs(u[s, :, 0]).max() > 0        # (the table has ended; it had begun)
    full = [s for s in range(case["S"]) if case["end_tau"][s] == 1.0]
    ref = foh_resample_ragged(case["table"][full], np.full(len(full), R.KU), [R.n_eval_of(case, s) for s in full])
    assert np.abs(u[full][:, :, :ref.shape[2]] - ref).max() <= 1e-15 * max(1.0, np.abs(ref).max()) and nmax >= ref.shape[2]


@pytest.mark.parametrize("law", ("sequence", "tangential"))
def test_forty_output_points_in_a_few_steps(law):
    """tf = 0.5, n_eval = 40: four to eight accepted steps with five to ten output points each; the tangential law's u_out against
    tangential_thrust on the returned trajectory at the existing test's tolerance"""
    from mpconstellation_amd.constellation import tangential_thrust
    case = R.dense_points(0.5, 40, law)
    acc, rej = R.counts(case)
    print(f"accepted {acc.tolist()}, rejected {rej.tolist()}: 40 output points")
    assert acc.max() <= 8
    y, st, ns, u = device_flight(case, thrust=True)
    hold_to_oracle(case, y, st, ns)
    if law == "tangential":
        assert np.abs(u - tangential_thrust(y, case["tangential"][:, None])).max() < 1e-14


@pytest.mark.parametrize("max_step", (float("inf"), 2.0))
def test_max_step_above_one_is_max_step_one(mixed, max_step):
    """scipy's default max_step = inf, and 2: no step of an interval of length 1 is clipped by either -- the bits and the counts of
    max_step = 1 (which test_mixed_waves holds to the oracle), and the oracle's counts at this max_step"""
    case, y1, st1, ns1 = mixed
    y, st, ns = device_flight(case, max_step=max_step)
    assert (st == 0).all() and np.array_equal(ns, ns1) and np.array_equal(y, y1)
    assert np.array_equal(ns, [R.oracle_flight(case, s, max_step=max_step)[2] for s in range(case["S"])])


def test_between_the_regimes():
    """max_step = 0.05: the steps grow by the factor's maximum from the initial one, run at max_step (`surely_small` and the full
    norm alternate), and the last one is shorter; one satellite takes 20 steps and rejects none, the others reject one and three"""
    case = R.between_regimes()
    acc, rej = R.counts(case)
    print(f"accepted {acc.tolist()}, rejected {rej.tolist()}")
    assert ((acc >= 20) & (rej == 0)).any() and (rej >= 1).any()
    hold_to_oracle(case, *device_flight(case))


@pytest.mark.parametrize("law", R.OTHER_LAWS)
def test_other_thrust_laws(law):
    """the same controller through the kernel's other thrust-law templates: S = 3, max_step = 1, drag + J2"""
    case = R.other_law(law)
    hold_to_oracle(case, *device_flight(case))


@pytest.mark.parametrize("which", list(R.OTHER_FLAGS))
def test_other_model_flags(which):
    """and through its model templates: no perturbation, J2, drag, drag under the atmosphere of tests/drag_cases.py with J2"""
    case = R.other_flags(which)
    hold_to_oracle(case, *device_flight(case))


@pytest.mark.parametrize("max_step", (1.0, 1e-3))
def test_a_failing_satellite_leaves_its_neighbours_alone(mixed, max_step):
    """one quad of the first wave starts from a NaN velocity component: every attempt's error norm is NaN, the step shrinks by
    MIN_FACTOR until it is below min_step (at t = 0: ten denormals, some 460 attempts) and the satellite reports MPCX_ST_STEP
    -- the oracle refuses the start as scipy does -- while every other satellite's output is the launch's without it, bit for bit"""
    case, y1, st1, ns1 = mixed
    y0 = case["y0"].copy()
    y0[R.BAD_SAT, R.BAD_COMPONENT] = np.nan
    assert R.oracle_flight(case, R.BAD_SAT, y0[R.BAD_SAT])[1] != 0
    if max_step != case["max_step"]:
        y1, st1, ns1 = device_flight(case, max_step=max_step)
        assert (st1 == 0).all()
        assert np.array_equal(ns1, [R.oracle_flight(case, s, max_step=max_step)[2] for s in range(case["S"])])
    y, st, ns = device_flight(case, max_step=max_step, y0=y0)
    good = np.arange(case["S"]) != R.BAD_SAT
    print(f"max_step {max_step:g}: status {st.tolist()}, accepted steps of the failing satellite {ns[R.BAD_SAT]}")
    assert st[R.BAD_SAT] == ST_STEP and ns[R.BAD_SAT] == 0 and (st[good] == 0).all()
    assert np.array_equal(ns[good], ns1[good]) and np.array_equal(y[good], y1[good])
