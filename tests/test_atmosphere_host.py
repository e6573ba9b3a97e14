"""The altitude-dependent atmosphere without a device: the model's numbers (Atmosphere), the reference-convention functions,
the flag words and the mpcx_set_atmosphere calls the wrappers make with atmosphere= (a recording stub in place of the library,
as in tests/test_wrapper_calls_host.py), Discretizer's refusal of foreign density callables, and the assertions the fixture
generator stored beside tests/golden/atmo_*.npz."""
import os

import numpy as np
import pytest

from mpconstellation_amd import Atmosphere, Discretizer, _ffi
from mpconstellation_amd.constants import R_EARTH
from mpconstellation_amd.optimizer import mpc_step_batch, mpc_update_batch, scp_iteration_batch
from mpconstellation_amd.simulator import propagate_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = 5
DRAG_ATMO = _ffi.FLAG_DRAG | _ffi.FLAG_ATMO


# ------------------------------------------------------------------------------------------------ the model
def test_power_law_is_the_reference_fit():
    """simulator.py:110: 8E26 * altitude**-6.828"""
    atm = Atmosphere.power_law()
    want = 8e26 * 5e5 ** -6.828
    assert abs(float(atm.density(5e5)) - want) <= 1e-14 * want
    c0, c1, c2, floor = atm.coefficients()
    assert (c0, c1, c2) == (np.log(8e26), -6.828, 0.0) and floor > 0


def test_exponential_coefficients():
    atm = Atmosphere.exponential(rho_ref=3e-12, h_ref=4e5, H=6e4, h_floor=2e5)
    assert atm.coefficients() == (np.log(3e-12) + 4e5 / 6e4, 0.0, -1.0 / 6e4, 2e5)
    for h in (2.5e5, 4e5, 9e5):
        want = 3e-12 * np.exp(-(h - 4e5) / 6e4)
        assert abs(float(atm.density(h)) - want) <= 1e-13 * want
    assert abs(float(atm.density(4e5)) - 3e-12) <= 1e-13 * 3e-12


@pytest.mark.parametrize("atm", [Atmosphere.power_law(h_floor=2e5), Atmosphere.exponential(6e-13, 540e3, 7.9e4, h_floor=2e5),
                                 Atmosphere(-20.0, -1.5, -4e-6, 2e5)])
def test_ddensity_is_the_derivative_of_density(atm):
    h = np.array([2.5e5, 5.4e5, 6.8e5, 4e6])
    step = np.imag(atm.density(h + 1e-20j)) / 1e-20
    assert np.abs(atm.ddensity(h) - step).max() <= 1e-13 * np.abs(step).max()
    assert (atm.ddensity(h) < 0).all()


def test_floor():
    atm = Atmosphere.power_law(h_floor=3e5)
    below = np.array([-5e6, 0.0, 1.0, 2.9e5, 3e5])
    assert (atm.density(below) == atm.density(3e5)).all() and (atm.ddensity(below) == 0.0).all()
    assert atm.density(3.1e5) < atm.density(3e5) and atm.ddensity(3.1e5) < 0
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            Atmosphere.power_law(h_floor=bad)
    with pytest.raises(ValueError):
        Atmosphere(np.inf, 0.0, 0.0, 1e5)


def test_reference_funcs_are_the_formula_in_normalised_units():
    class Const:
        R0, RHO = 6.9e6, 2.3e-5
    atm = Atmosphere.exponential(6e-13, 540e3, 7.9e4, h_floor=2e5)
    rho_func, drho_func = atm.reference_funcs(Const)
    r = np.array([0.7, -0.6, 0.45])
    alt = np.linalg.norm(r * Const.R0) - R_EARTH
    assert alt > 2e5
    assert rho_func(r) == atm.density(alt) / Const.RHO
    assert drho_func(r) == atm.ddensity(alt) * Const.R0 / Const.RHO
    # ... and drho_func is the derivative of rho_func along the radius
    eps = 1e-6
    fd = (rho_func(r * (1 + eps)) - rho_func(r * (1 - eps))) / (2 * eps * np.linalg.norm(r))
    assert abs(fd - drho_func(r)) <= 1e-7 * abs(fd)
    # on the floor: the floor's density, no slope
    low = r * (R_EARTH + 1e5) / np.linalg.norm(r * Const.R0)
    assert rho_func(low) == atm.density(2e5) / Const.RHO and drho_func(low) == 0.0


# ------------------------------------------------------------------------------------------------ what the wrappers hand over
class Recorder:
    """stands in for the loaded library (tests/test_wrapper_calls_host.py): records (name, args), returns 0"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if not name.startswith("mpcx_"):
            raise AttributeError(name)
        if name == "mpcx_default_solve_opts":
            return getattr(self.real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    from mpconstellation_amd import build
    build.build()                                       # (cross-compiles without a GPU, as in test_cabi.py; no-op when built)
    r = Recorder(_ffi.load())
    monkeypatch.setattr(_ffi, "load", lambda: r)
    monkeypatch.setattr(_ffi, "context", lambda device=0, slot=0: ("ctx", int(device), int(slot)))
    monkeypatch.setattr(_ffi, "dptr", lambda a: a)
    monkeypatch.setattr(_ffi, "iptr", lambda a: a)
    return r


ATM = Atmosphere.power_law(h_floor=1.5e5)


def flag_args(name):
    """positions of the int flag words of an entry point that follow a pointer and precede an int or a double: found by name"""
    return {"mpcx_mpc_step_batch": [8], "mpcx_mpc_step_batch_ragged": [9], "mpcx_propagate_batch": [6], "mpcx_propagate_batch_ragged": [7],
            "mpcx_propagate_thrust_batch_ragged": [7], "mpcx_discretize_batch": [8], "mpcx_scp_iteration_batch_ragged": [8, 15],
            "mpcx_mpc_update_batch": [11, 26]}[name]


def one_call(rec, ctx=("ctx", 0, 0), atmosphere=True):
    """the recorded calls are [mpcx_set_atmosphere(ctx, coefficients)], the entry point: returns (name, its flag words)"""
    calls = rec.calls
    if atmosphere:
        assert calls[0][0] == "mpcx_set_atmosphere" and calls[0][1][0] == ctx
        coef = calls[0][1][1]
        assert coef.dtype == np.float64 and coef.flags.c_contiguous and np.array_equal(coef, ATM.coefficients())
        calls = calls[1:]
    assert len(calls) == 1, [c[0] for c in rec.calls]
    name, args = calls[0]
    assert args[0] == ctx and len(args) == len(_ffi._SIGS[name][1])
    return name, [args[i] for i in flag_args(name)]


def step_inputs(S):
    return np.ones((S, 7, K)), np.zeros((S, 3, K)), np.ones((S, 8))


def test_step_flag_word_carries_the_bit(rec):
    x, u, c = step_inputs(3)
    mpc_step_batch(x, u, 1.0, c, 1.0, include_drag=True, include_J2=True, atmosphere=ATM)
    assert one_call(rec) == ("mpcx_mpc_step_batch", [DRAG_ATMO | _ffi.FLAG_J2])
    rec.calls.clear()
    mpc_step_batch(x, u, 1.0, c, 1.0, include_drag=True, atmosphere=ATM, Ks=[5, 4, 3], uniform_steps=7, rk23=True)
    assert one_call(rec) == ("mpcx_mpc_step_batch_ragged", [DRAG_ATMO | _ffi.FLAG_UNIFORM_STEPS | _ffi.FLAG_RK23 | (7 << 8)])
    # without drag there is nothing for the atmosphere to act on: the call it was, and the context is left alone
    rec.calls.clear()
    mpc_step_batch(x, u, 1.0, c, 1.0, include_J2=True, atmosphere=ATM)
    assert one_call(rec, atmosphere=False) == ("mpcx_mpc_step_batch", [_ffi.FLAG_J2])
    # atmosphere=None: the call it was
    rec.calls.clear()
    mpc_step_batch(x, u, 1.0, c, 1.0, include_drag=True)
    assert one_call(rec, atmosphere=False) == ("mpcx_mpc_step_batch", [_ffi.FLAG_DRAG])


def test_every_block_of_a_multi_device_step_gets_the_atmosphere(rec):
    x, u, c = step_inputs(4)
    mpc_step_batch(x, u, 1.0, c, 1.0, include_drag=True, atmosphere=ATM, devices=[0, 0])
    by_ctx = {}
    for name, args in rec.calls:
        by_ctx.setdefault(args[0], []).append((name, args))
    assert set(by_ctx) == {("ctx", 0, 0), ("ctx", 0, 1)}
    for ctx, calls in by_ctx.items():
        assert [n for n, _ in calls] == ["mpcx_set_atmosphere", "mpcx_mpc_step_batch"]          # (set before the block's call)
        assert np.array_equal(calls[0][1][1], ATM.coefficients()) and calls[1][1][8] == DRAG_ATMO


def test_propagate_flag_word_carries_the_bit(rec):
    y0 = np.ones((2, 7)); c = np.ones((2, 8)); law = (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None)
    propagate_batch(y0, 1.0, c, law, 6, include_drag=True, include_J2=True, atmosphere=ATM)
    assert one_call(rec) == ("mpcx_propagate_batch", [DRAG_ATMO | _ffi.FLAG_J2])
    rec.calls.clear()
    propagate_batch(y0, 1.0, c, law, [6, 4], include_drag=True, atmosphere=ATM, thrust=True)
    assert one_call(rec) == ("mpcx_propagate_thrust_batch_ragged", [DRAG_ATMO])
    rec.calls.clear()
    propagate_batch(y0, 1.0, c, law, 6, include_drag=True)
    assert one_call(rec, atmosphere=False) == ("mpcx_propagate_batch", [_ffi.FLAG_DRAG])


def test_scp_iteration_flag_words_carry_the_bit(rec):
    y0 = np.ones((2, 7)); c = np.ones((2, 8)); law = (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None)
    scp_iteration_batch(y0, 1.0, c, 1.0, law, K, include_drag=True, rollout_model=True, atmosphere=ATM)
    assert one_call(rec) == ("mpcx_scp_iteration_batch_ragged", [DRAG_ATMO, DRAG_ATMO])
    rec.calls.clear()
    scp_iteration_batch(y0, 1.0, c, 1.0, law, K, include_drag=True, include_J2=True, atmosphere=ATM)           # the reference's rollout
    assert one_call(rec) == ("mpcx_scp_iteration_batch_ragged", [0, DRAG_ATMO | _ffi.FLAG_J2])


def test_update_flag_words_carry_the_bit_on_both_sides(rec):
    y0 = np.ones((2, 7)); c = np.ones((2, 8))
    fly = (1.0, 1.0, 4, True, True)
    mpc_update_batch(y0, 1.0, c, 1.0, K, include_drag=True, include_J2=True, rollout_model=True, fly=fly, atmosphere=ATM)
    assert one_call(rec) == ("mpcx_mpc_update_batch", [DRAG_ATMO | _ffi.FLAG_J2 | _ffi.FLAG_PLAN_ROLLOUTS, DRAG_ATMO | _ffi.FLAG_J2])
    rec.calls.clear()          # the reference's planner, the truth model with the atmosphere
    mpc_update_batch(y0, 1.0, c, 1.0, K, fly=fly, atmosphere=ATM)
    assert one_call(rec) == ("mpcx_mpc_update_batch", [0, DRAG_ATMO | _ffi.FLAG_J2])
    rec.calls.clear()          # a plan with the atmosphere, a flight without drag
    mpc_update_batch(y0, 1.0, c, 1.0, K, include_drag=True, fly=(1.0, 1.0, 4, False, True), atmosphere=ATM)
    assert one_call(rec) == ("mpcx_mpc_update_batch", [DRAG_ATMO, _ffi.FLAG_J2])
    rec.calls.clear()
    mpc_update_batch(y0, 1.0, c, 1.0, K, include_drag=True, fly=fly)
    assert one_call(rec, atmosphere=False) == ("mpcx_mpc_update_batch", [_ffi.FLAG_DRAG, _ffi.FLAG_DRAG | _ffi.FLAG_J2])


class _Const:
    def as_vector(self):
        return np.ones(8)


def test_discretizer_flag_word_and_refusal(rec):
    d = Discretizer(_Const(), include_drag=True, include_J2=True, atmosphere=ATM)
    assert d.device_flags(True) == DRAG_ATMO | _ffi.FLAG_J2
    d.discretize_batch(np.ones((1, 7, K)), np.zeros((1, 3, K)), [1.0], np.ones((1, 8)))
    assert one_call(rec) == ("mpcx_discretize_batch", [DRAG_ATMO | _ffi.FLAG_J2])
    # a foreign density callable is still refused, and the message names the keyword
    for kw in (dict(rho_func=lambda r: 1.0), dict(drho_func=lambda r: 0.0), dict(rho_func=lambda r: 1.0, drho_func=lambda r: 0.0)):
        for atmosphere in (None, ATM):
            with pytest.raises(NotImplementedError, match="atmosphere="):
                Discretizer(_Const(), include_drag=True, atmosphere=atmosphere, **kw)._check_modes()
    Discretizer(_Const(), include_drag=True, atmosphere=ATM)._check_modes()
    assert Discretizer(_Const(), include_drag=True).device_flags() == _ffi.FLAG_DRAG


def test_constellation_mpc_hands_the_atmosphere_to_plan_and_flight(rec, monkeypatch):
    from mpconstellation_amd import ConstellationMPC, Satellite
    sats = [Satellite(np.array([7e6, 0.0, 0.0]), np.array([0.0, 7.5e3, 0.0]), 100.0) for _ in range(2)]
    mpc = ConstellationMPC(sats, base_res=K, plan_drag=True, plan_J2=True, atmosphere=ATM)
    assert mpc._plan_model["atmosphere"] is ATM
    flags = []
    import mpconstellation_amd.constellation_mpc as M

    def fake_update(*a, **kw):
        flags.append(kw)
        raise RuntimeError("stop here")
    monkeypatch.setattr(M, "mpc_update_batch", fake_update)
    with pytest.raises(RuntimeError, match="stop here"):
        mpc.run_segment(1)
    assert flags[0]["atmosphere"] is ATM and flags[0]["include_drag"] is True and flags[0]["fly"][3] is True


def test_set_atmosphere_binding(rec):
    _ffi.set_atmosphere(("ctx", 0, 0), None)
    assert rec.calls == [("mpcx_set_atmosphere", (("ctx", 0, 0), None))]
    rec.calls.clear()
    _ffi.set_atmosphere(("ctx", 0, 0), (1.0, 2.0, 3.0, 4.0))
    assert np.array_equal(rec.calls[0][1][1], [1.0, 2.0, 3.0, 4.0])
    with pytest.raises(ValueError):
        _ffi.set_atmosphere(("ctx", 0, 0), (1.0, 2.0, 3.0))
    assert _ffi.FLAG_ATMO == 32 and _ffi.NATMO == 4


# ------------------------------------------------------------------------------------------------ the committed fixtures
def test_fixture_assertions_hold():
    """(a) the drag is >= 1e-4 of A on the S x 1e4 cases, (b) the position block and (c) the altitude dependence each >= 1e-6 of A
    -- a kernel without either fails the 1e-10 comparison --, (d) the pinned Jacobian is the derivative of the pinned dynamics;
    the rollouts cross a factor >= 2 of density and end >= 1e-6 from the fixed-density rollout."""
    g = np.load(os.path.join(GOLDEN, "atmo_discretize.npz"))
    cases = [str(c) for c in g["cases"]]
    big = [c for c in cases if "bigS" in c]
    assert len(cases) == 6 and len(big) == 5
    assert {str(g[f"solver_{c}"]) for c in cases} == {"RK45", "RK23"} and {int(g[f"steps_{c}"]) for c in cases} == {0, 11}
    assert {str(g[f"model_{c}"]) for c in cases} == {"power", "exp"} and any(bool(g[f"j2_{c}"]) for c in cases)
    for c in big:
        assert g[f"drag_share_{c}"] >= 1e-4, c
        assert g[f"position_share_{c}"] >= 1e-6, c
        assert g[f"fixed_density_share_{c}"] >= 1e-6, c
    for c in cases:
        assert g[f"jacobian_error_{c}"] < 1e-9, c
    assert np.array_equal(g["atmo_power"][:3], Atmosphere.power_law().coefficients()[:3])
    power, expo = Atmosphere(*g["atmo_power"]), Atmosphere(*g["atmo_exp"])
    assert abs(expo.density(540e3) / power.density(540e3) - 1) < 1e-12 and abs(expo.ddensity(540e3) / power.ddensity(540e3) - 1) < 1e-12
    p = np.load(os.path.join(GOLDEN, "atmo_propagate.npz"))
    for c in (str(c) for c in p["cases"]):
        assert p[f"density_ratio_{c}"] >= 2.0 and p[f"fixed_density_end_{c}"] >= 1e-6, c
        assert p[f"y_{c}"].shape == (7, int(p["n_eval"]))
    for f in ("atmo_discretize.npz", "atmo_propagate.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, f)) <= os.path.getsize(os.path.join(GOLDEN, "drag_discretize.npz"))
