"""The planning model without a device: Discretizer's drag mode and its flags, the flag words an SCP iteration and an update
hand the library for a planning model (include/mpcx.h: MPCX_FLAG_DRAG, MPCX_FLAG_J2, MPCX_FLAG_PLAN_ROLLOUTS), and the
controllers passing their planning model on."""
import numpy as np
import pytest


class _Const:
    def as_vector(self):
        return np.zeros(8)


def satellite_dynamics(*a, **k):  # token accepted by Discretizer.discretize
    raise RuntimeError("host dynamics are never called")


def hubble():
    from mpconstellation_amd import Satellite
    return Satellite(np.array([5371.4806, -4133.1393, 1399.9594]) * 1000, np.array([4.6921, 4.9848, -3.2752]) * 1000, 12200)


def test_drag_discretizer_flags():
    from mpconstellation_amd import Discretizer, _ffi
    d = Discretizer(_Const(), include_drag=True)
    d._check_modes()                                          # the simulator's atmosphere: accepted
    assert d.device_flags() == _ffi.FLAG_DRAG
    d.use_uniform_steps = True; d.integrator_steps = 11; d.ivp_solver = 'RK23'
    assert d.device_flags() == _ffi.FLAG_DRAG | _ffi.FLAG_UNIFORM_STEPS | (11 << 8) | _ffi.FLAG_RK23
    assert Discretizer(_Const()).device_flags() == 0
    # a density model is read only with drag (linearize_discretize.py:162-165): without drag it is ignored, as there
    Discretizer(_Const(), rho_func=lambda r: 1.0, include_drag=False)._check_modes()


@pytest.mark.parametrize("which", ["rho_func", "drho_func"])
def test_foreign_density_model_raises_before_the_device(which, monkeypatch):
    from mpconstellation_amd import Discretizer, _ffi

    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(_ffi, "load", no_device)
    monkeypatch.setattr(_ffi, "context", no_device)
    d = Discretizer(_Const(), include_drag=True, **{which: lambda r: 1.0})
    x = np.ones((7, 5)); u = np.zeros((3, 5))
    with pytest.raises(NotImplementedError):
        d.discretize(satellite_dynamics, x, u, 1.0)
    with pytest.raises(NotImplementedError):
        d.discretize_batch(x[None], u[None], [1.0], np.zeros((1, 8)))


def test_planning_flag_words():
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.optimizer import scp_flags, update_flags
    D, J, P = _ffi.FLAG_DRAG, _ffi.FLAG_J2, _ffi.FLAG_PLAN_ROLLOUTS
    assert P == 16 and P & (_ffi.FLAG_UNIFORM_STEPS | _ffi.FLAG_RK23 | D | J) == 0 and (P >> 8) == 0
    # the reference's planner: nothing anywhere (what every existing call passes)
    assert scp_flags() == (0, 0) and update_flags() == 0
    assert scp_flags(include_J2=True) == (0, J) and update_flags(include_J2=True) == J
    # the model in the linearisation only
    assert scp_flags(True) == (0, D) and update_flags(True) == D
    assert scp_flags(True, True) == (0, D | J) and update_flags(True, True) == D | J
    # ... and in the rollouts
    assert scp_flags(True, True, True) == (D | J, D | J) and update_flags(True, True, True) == D | J | P
    assert scp_flags(False, True, True) == (J, J) and update_flags(False, True, True) == J | P
    assert scp_flags(True, False, True) == (D, D) and update_flags(True, False, True) == D | P


class _Stop(Exception):
    pass


def test_controllers_pass_their_planning_model_on(monkeypatch):
    """ConstellationMPC's one-call update, its verbose per-iteration path and OptimalController hand the planning model to the
    library calls; by default they ask for the reference's planner."""
    from mpconstellation_amd import constellation_mpc as CM, ConstellationMPC, OptimalController
    seen = []

    def fake(*a, **k):
        seen.append(k); raise _Stop
    monkeypatch.setattr(CM, "mpc_update_batch", fake)
    monkeypatch.setattr(CM, "scp_iteration_batch", fake)
    model = lambda k: (k["include_drag"], k["include_J2"], k["rollout_model"])
    for kw, want in ((dict(), (False, False, False)), (dict(plan_drag=True, plan_J2=True), (True, True, True)),
                     (dict(plan_J2=True), (False, True, True))):
        for verbose in (False, True):
            with pytest.raises(_Stop):
                ConstellationMPC([hubble()], verbose=verbose, **kw).update()
            assert model(seen[-1]) == want, (kw, verbose)
        with pytest.raises(_Stop):
            OptimalController(sats=[hubble()], plot_inter=False, opt_verbose=False, **kw).update()
        assert model(seen[-1]) == want, kw
