"""discretize_kernel (csrc/discretize.hip) against the CPU oracle where max_step does not clip its steps.

Of the kernel's 24 forms -- two layouts x {adaptive nodes, uniform dense-output nodes} x {RK45, RK23} x {no drag, drag, drag +
atmosphere} -- only plain adaptive RK45 in the stage layout was tested at max_step = 1
(test_discretize_step_factor_gpu.py::test_rejections_and_pow_in_mixed_waves); everything else ran at 1e-2, where every step is
max_step long, nothing is rejected and the controller's pow is never evaluated.  Here, at max_step = 1 (and inf, and 2):
rk_accepted_h_abs<23> with its exponent, its threshold and its cubic shortcut, and the rejection branch's own exponent; the
uniform branch after an accepted step -- Q from RK_P / RK23_P, a step with up to ten points beside a group of the same wave that
rejected or has finished, integrator_steps = 2 where A_k is the interpolant at x = 1; uniform points that walk the thrust
table's cache backwards through columns the stages have left; drag_lin / drag_dv under rejections, and the node of a wave that
mixes a rejecting group with an accepting one, which re-evaluates the drag partials instead of taking the last stage's.

The inputs, the oracle's counts for them, the conditions that say each launch does take those paths and the tolerance are those
of tests/discretize_cases.py, which tests/test_discretize_unclipped_host.py anchors to the reference's own arrays without a
device: 1e-8 max(1, cond(A_k) / 2e4) relative to each array's magnitude, at most 1e-3 of what another step sequence moves the
arrays by.  Measured on an MI355X: profiles/discretize_unclipped.txt."""
import functools

import numpy as np
import pytest

import discretize_cases as C
import oracle_lib as O

pytestmark = pytest.mark.gpu
ST_STEP = 2                      # MPCX_ST_STEP (include/mpcx.h)


def device_flags(c, mode):
    from mpconstellation_amd import _ffi
    fl, uni = C.MODES[mode]
    return _ffi.discretize_flags(bool(c["flags"] & C.DRAG), bool(c["flags"] & C.J2), uniform_steps=uni, rk23=bool(fl & C.RK23), atmosphere=C.atmosphere(c))


def launch(c, mode, max_step=C.MAX_STEP, x=None):
    """one launch of mpcx_discretize_stages_ragged_dev (Ks only where the case is ragged) -> (stage records (S, K-1, 105), status)"""
    import dev_solve
    from mpconstellation_amd import _ffi
    if C.atmosphere(c) is not None:
        _ffi.set_atmosphere(_ffi.context(0), C.atmosphere(c))
    ragged = bool((c["Ks"] != c["K"]).any())
    stage, st = dev_solve.discretize_stages(c["x"] if x is None else x, c["u"], c["tf"], c["const"], Ks=c["Ks"] if ragged else None,
                                            flags=device_flags(c, mode), max_step=max_step)
    return stage.cpu().numpy(), st


@functools.lru_cache(None)
def launched(name, mode):
    """the (case, mode) at max_step = 1: launched once, shared by the tests that compare other launches with it"""
    return launch(C.case(name), mode)


def unpack(c, stage):
    import dev_solve
    import torch
    t = torch.from_numpy(stage)
    return [dev_solve.unpack_stage(t, s, int(c["Ks"][s])) for s in range(c["S"])]


def hold_to_oracle(name, mode, stage, st):
    """the conditions and the tolerance first (properties of the oracle alone), then: status 0 and every satellite's five arrays
    within the tolerance of the oracle's; prints the record of profiles/discretize_unclipped.txt"""
    c = C.case(name)
    rec = C.check_conditions(name, mode)
    tol = C.tolerance(name, mode)
    errs = C.errors(unpack(c, stage), C.oracle(name, mode))
    worst = max(errs.values())
    print(f"{name} {mode}: accepted {rec['accepted']} rejected {rec['rejected']} cond {rec['cond']:.3g} tolerance {tol:.3g}; relative errors "
          f"{', '.join(f'{k} {e:.3g}' for k, e in errs.items())}: worst {worst:.3g} = {worst / tol:.3g} of the tolerance")
    assert (st == 0).all(), st
    assert worst <= tol, (name, mode, errs, tol)
    return worst / tol


@pytest.mark.parametrize("j2", (False, True), ids=("nj2", "j2"))
@pytest.mark.parametrize("mode", C.PLAIN_MODES)
def test_plain_modes_in_mixed_waves(mode, j2):
    """(A) S = 7, K = 4, Ku = 13: 21 intervals in three waves, the last with five live groups.  RK23: 20 to 33 steps per interval
    and one to nine rejected attempts in every one; the uniform modes on RK45's 7 to 11 steps, five intervals with rejected
    attempts spread over the three waves: uni33 with up to ten points in a step, uni5 with most steps empty, uni2 with its
    one point at the end of the last step; a step reaches into up to three intervals of the thrust table"""
    name = "plain+j2" if j2 else "plain"
    hold_to_oracle(name, mode, *launched(name, mode))


@pytest.mark.parametrize("mode", C.DRAG_MODES)
@pytest.mark.parametrize("model", ("fixed", "general"))
def test_drag_forms_reject_and_interpolate(model, mode):
    """(B) three low satellites with drag + J2 under the fixed density and the general atmosphere, Ks = (4, 3, 4) in one ragged stage
    launch: nine slots in two waves, one a shadow, the second wave with one group; the first wave holds rejecting intervals (up
    to 15 attempts) beside clean ones, so its nodes take the arm that evaluates the drag partials again.  Satellite by satellite
    against the oracle; the NaN columns behind the middle satellite's nodes are never read: the status is 0"""
    name = f"drag-{model}"
    c = C.case(name)
    assert np.isnan(c["x"][1, :, 3]).all() and c["Ks"].tolist() == [4, 3, 4]
    hold_to_oracle(name, mode, *launched(name, mode))


def test_reference_layout_matches_stage_layout():
    """Discretizer.discretize_batch with ivp_max_step = 1 is the kernel's other layout (its own Sigma / xi indexing, five output
    arrays): bit for bit the unpacked stage records of the same inputs -- (A) under uni33, (B) under the general atmosphere and
    RK23 with Ks = 4 throughout (that layout is not ragged), which is held to the oracle here as well"""
    from mpconstellation_amd import Discretizer
    from test_drag_oracle_gpu import _Const
    for name, mode in (("plain", "uni33"), ("drag-general-k4", "rk23")):
        c = C.case(name)
        stage, st = launched(name, mode)
        hold_to_oracle(name, mode, stage, st)
        fl, uni = C.MODES[mode]
        d = Discretizer(_Const(c["const"][0]), include_drag=bool(c["flags"] & C.DRAG), include_J2=bool(c["flags"] & C.J2), atmosphere=C.atmosphere(c))
        d.ivp_max_step = C.MAX_STEP
        if fl & C.RK23:
            d.ivp_solver = "RK23"
        if uni:
            d.use_uniform_steps = True; d.integrator_steps = uni
        out = d.discretize_batch(c["x"], c["u"], c["tf"], c["const"])
        assert (out[5] == 0).all(), out[5]
        import dev_solve
        for s, rec in enumerate(unpack(c, stage)):
            for i, k in enumerate(C.KEYS):
                assert dev_solve.same_bits(out[i][s], rec[k]), (name, mode, s, k, np.abs(out[i][s] - rec[k]).max())


@pytest.mark.parametrize("mode", C.ONE_MODES)
def test_one_interval(mode):
    """(C) S = 1, K = 2, tf = 2.5: one live group in the only wave -- seven groups shadow it -- on one interval of the whole
    horizon: 69 RK23 steps with 11 rejected attempts; 32 uniform points over 21 RK45 steps, none to three in a step"""
    hold_to_oracle(C.ONE, mode, *launched(C.ONE, mode))


@pytest.mark.parametrize("mode", ("rk23", "uni33"))
@pytest.mark.parametrize("max_step", (float("inf"), 2.0))
def test_max_step_above_one_is_max_step_one(max_step, mode):
    """no interval is longer than 1, so no step is clipped by inf (scipy's default) or 2 either: the stage records of max_step = 1,
    which test_plain_modes_in_mixed_waves holds to the oracle, bit for bit.  Shortcut (c) of rk_accepted_h_abs returns 2 max_step
    here where the formula returns another length beyond the interval's end: both are cut to the end point"""
    import dev_solve
    stage1, st1 = launched("plain", mode)
    stage, st = launch(C.case("plain"), mode, max_step=max_step)
    assert (st == 0).all() and (st1 == 0).all()
    assert dev_solve.same_bits(stage, stage1)


@pytest.mark.parametrize("mode", ("uni5", "rk23", "rk23+uni7"))
def test_a_failing_satellite_leaves_its_neighbours_alone(mode):
    """(A) with x[3, 0, 1] = NaN: the second interval of satellite 3 -- a group of the second wave -- has a NaN error norm on every
    attempt, its step shrinks by MIN_FACTOR to the step-size floor (some twenty attempts beside groups that go on stepping) and
    the satellite reports MPCX_ST_STEP -- the oracle refuses that start as scipy does; every other satellite's records are
    those of the launch without the NaN, bit for bit.  The failed group accepted no step and, once failed, commits no node --
    not a uniform point either, though its t then stands at the interval's end: its record is the start, A = I and the
    integrals zero, and its satellite's other two intervals are untouched.  (Under RK45 the other groups of the wave have
    finished by the time this one gives up; under RK23 with uniform points they are still accepting steps, and the uniform
    loop runs with the failed group in it.)"""
    import dev_solve
    c = C.case("plain")
    x = C.bad_x(c)
    oracle_status = [o["status"] for o in C.run_oracle(c, mode, x=x)]
    assert oracle_status == [O.ST_START_NOT_FINITE if s == C.BAD_SAT else 0 for s in range(c["S"])]
    assert O.DEVICE_STATUS[oracle_status[C.BAD_SAT]] == ST_STEP
    stage1, st1 = launched("plain", mode)
    stage, st = launch(c, mode, x=x)
    good = np.arange(c["S"]) != C.BAD_SAT
    print(f"{mode}: status {st.tolist()}")
    assert st[C.BAD_SAT] == O.DEVICE_STATUS[oracle_status[C.BAD_SAT]] and (st[good] == 0).all() and (st1 == 0).all()
    assert dev_solve.same_bits(stage[good], stage1[good])
    others = [k for k in range(c["K"] - 1) if k != C.BAD_NODE]
    assert dev_solve.same_bits(stage[C.BAD_SAT, others], stage1[C.BAD_SAT, others])
    failed = stage[C.BAD_SAT, C.BAD_NODE]
    assert np.array_equal(failed[:49].reshape(7, 7), np.eye(7)) and (failed[49:] == 0.0).all(), failed
