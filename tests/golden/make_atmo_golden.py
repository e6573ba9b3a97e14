#!/usr/bin/env python3
"""Golden vectors of the altitude-dependent atmosphere: the reference's own drag branch -- Discretizer(include_drag=True) with
rho_func / drho_func (linearize_discretize.py:162-173) and Simulator.satellite_dynamics with get_atmo_density (simulator.py:97-153)
-- given the density model of mpconstellation_amd.Atmosphere, which holds the power fit the reference keeps commented out
(simulator.py:110).

The reference's code computes everything: its get_atmo_density is replaced by the model at the altitude expression of
simulator.py:109, its Discretizer gets the model's reference_funcs (module-level here: the reference's discretize ships its
Discretizer through multiprocessing.Pool, which cannot pickle lambdas) and const.CD = C_D.

Runs ONLY in the build container, like make_golden.py (whose import shims and helpers it reuses); writes atmo_discretize.npz and
atmo_propagate.npz.  Every assertion the generator makes about a fixture is stored beside its arrays.
"""
import copy
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG                    # noqa: E402  (registers the pyomo placeholders, puts the reference on the path)

import numpy as np                          # noqa: E402
from scipy import integrate                 # noqa: E402

import constants as RC                      # noqa: E402
import simulator as RSIM                    # noqa: E402
from simulator import Simulator             # noqa: E402
from linearize_discretize import Discretizer  # noqa: E402
from control import ConstantTangentialThrustController, SequenceController  # noqa: E402
from satellite import Satellite             # noqa: E402
from satellite_scale import SatelliteScale  # noqa: E402

sys.path.insert(0, os.path.join(HERE, "..", ".."))
from mpconstellation_amd.atmosphere import Atmosphere  # noqa: E402
from mpconstellation_amd.constants import R_EARTH      # noqa: E402

S_SCALE = 1e4
RHO_500 = 9.983e-13
H_FIT = 540e3                                # the Hubble's altitude: where the exponential model is fitted to the power law
_MODEL = {"atm": None, "rho": None, "drho": None, "no_drho": False}      # the model of the case being computed (inherited by the pool's forks)


def _norm(x):
    """np.linalg.norm for the reference's real vectors; the analytic form for a complex step"""
    return np.linalg.norm(x) if np.isrealobj(x) else np.sqrt(np.sum(x * x))


def atmo_density(r, r0):
    """stands in for Simulator.get_atmo_density: the model at the altitude of simulator.py:109; None: the reference's constant"""
    if _MODEL["atm"] is None:
        return RHO_500
    return _MODEL["atm"].density(_norm(r * r0) - RC.R_EARTH)


def rho_func(r):
    return _MODEL["rho"](r)


def drho_func(r):
    return 0.0 if _MODEL["no_drho"] else _MODEL["drho"](r)


def set_model(atm, const, no_drho=False):
    _MODEL["atm"] = atm
    if atm is None:
        _MODEL["rho"], _MODEL["drho"] = (lambda r: RHO_500 / const.RHO), (lambda r: 0.0)
    else:
        _MODEL["rho"], _MODEL["drho"] = atm.reference_funcs(const)
    _MODEL["no_drho"] = no_drho


def discretizer(const, j2, solver, steps, drag=True):
    const = copy.copy(const)
    const.CD = RC.C_D
    d = Discretizer(const, rho_func=rho_func, drho_func=drho_func, include_drag=drag, include_J2=j2)
    d.ivp_solver = solver
    if steps:
        d.use_uniform_steps = True; d.integrator_steps = steps
    return d


class _ComplexNumpy:
    """numpy as the reference's simulator module sees it during a complex step: arrays it allocates hold complex numbers and the
    norm is analytic; everything else is numpy's"""

    class linalg:
        norm = staticmethod(lambda x: np.sqrt(np.sum(np.asarray(x) * np.asarray(x))))

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def zeros(shape, *a, **k):
        return np.zeros(shape, dtype=complex)


def complex_step_jacobian(x, u, const, drag):
    """d satellite_dynamics / d x at (x, u), tf = 1, no J2, by complex steps through the reference's own (patched) function"""
    J = np.zeros((7, 7))
    saved = RSIM.np
    RSIM.np = _ComplexNumpy()
    try:
        for j in range(7):
            xc = x.astype(complex); xc[j] += 1e-30j
            J[:, j] = np.imag(MG.F(0.0, xc, lambda y, tau: u, 1, const, include_drag=drag, include_J2=False)) / 1e-30
    finally:
        RSIM.np = saved
    return J


def check_jacobian(x, u, const):
    """(d): the drag part of A_func against the complex-step derivative of the drag part of the patched dynamics, at every
    seventh node; the largest difference over the largest drag entry of those nodes (both parts are differences of a Jacobian
    with and without drag: at the high nodes, where the density has fallen by orders of magnitude, the drag part is smaller than
    the rounding of the gravity terms it is taken from -- a ratio per node would measure that rounding)"""
    err = size = 0.0
    d1, d0 = discretizer(const, False, "RK45", 0), discretizer(const, False, "RK45", 0, drag=False)
    for k in range(0, x.shape[1], 7):
        A_drag = d1.A_func(x[:, k], u[:, k], 1) - d0.A_func(x[:, k], u[:, k], 1)
        J_drag = complex_step_jacobian(x[:, k], u[:, k], const, True) - complex_step_jacobian(x[:, k], u[:, k], const, False)
        err, size = max(err, np.abs(A_drag - J_drag).max()), max(size, np.abs(J_drag).max())
    return err / size


def gen_discretize():
    assert RC.R_EARTH == R_EARTH
    sat = Satellite(MG.R_HUBBLE, MG.V_HUBBLE, MG.M_HUBBLE)
    scale = SatelliteScale(sat=sat)
    const = scale.get_normalized_constants()
    const_big = copy.copy(const)
    const_big.S = const.S * S_SCALE
    ctrl = ConstantTangentialThrustController([sat], 0.5)
    set_model(None, const)
    x30, t30, u30 = MG.reference_case(sat, scale, ctrl, 1, 30)
    x12, t12, u12 = MG.reference_case(sat, scale, ctrl, 1, 12)
    power = Atmosphere.power_law()
    # the exponential atmosphere with the power law's value and slope at 540 km: the same size of drag, another shape
    expo = Atmosphere.exponential(float(power.density(H_FIT)), H_FIT, float(-power.density(H_FIT) / power.ddensity(H_FIT)))
    assert abs(expo.density(H_FIT) / power.density(H_FIT) - 1) < 1e-12 and abs(expo.ddensity(H_FIT) / power.ddensity(H_FIT) - 1) < 1e-12
    out = {"x_K30": x30, "u_K30": u30, "x_K12": x12, "u_K12": u12,
           "atmo_power": np.array(power.coefficients()), "atmo_exp": np.array(expo.coefficients())}
    cases = [
        # name, nodes, model, const, J2, ivp_solver, uniform steps (0: adaptive), store the accepted step nodes
        ("power_bigS", 30, "power", const_big, False, "RK45", 0, True),
        ("power_bigS_J2", 30, "power", const_big, True, "RK45", 0, False),
        ("power_bigS_J2_rk23", 30, "power", const_big, True, "RK23", 0, True),
        ("power_bigS_K12_uni11", 12, "power", const_big, False, "RK45", 11, False),
        ("exp_bigS", 30, "exp", const_big, False, "RK45", 0, False),
        ("power_S", 30, "power", const, False, "RK45", 0, False),
    ]
    for name, K, model, cst, j2, solver, steps, nodes in cases:
        x, u = (x30, u30) if K == 30 else (x12, u12)
        atm = power if model == "power" else expo
        set_model(atm, cst)
        d = discretizer(cst, j2, solver, steps)
        A, Bp, Bn, Sig, xi = d.discretize(MG.F, x, u, 1)
        rec = {f"K_{name}": np.int64(K), f"model_{name}": np.array(model), f"const_{name}": MG.const_vec(cst), f"j2_{name}": np.bool_(j2),
               f"solver_{name}": np.array(solver), f"steps_{name}": np.int64(steps), f"tf_{name}": np.float64(1),
               f"A_{name}": A, f"Bp_{name}": Bp, f"Bn_{name}": Bn, f"Sigma_{name}": Sig, f"xi_{name}": xi}
        if nodes:
            counts, nfev, nt, ny = MG.rk_nodes(d, x, u, 1)
            rec.update({f"node_counts_{name}": counts, f"node_t_{name}": nt})
        # (d) the Jacobian the fixture pins is the derivative of the dynamics it pins
        jac = check_jacobian(x, u, copy.copy(d.const))
        assert jac < 1e-9, (name, jac)
        rec[f"jacobian_error_{name}"] = np.float64(jac)
        if cst is const_big:
            amax = np.abs(A).max()
            # (a) how much of A the drag is
            A0 = discretizer(cst, j2, solver, steps, drag=False).discretize(MG.F, x, u, 1)[0]
            share = np.abs(A - A0).max() / amax
            # (b) ... the position block Dr a_D: the same model with drho_func = 0
            set_model(atm, cst, no_drho=True)
            A1 = discretizer(cst, j2, solver, steps).discretize(MG.F, x, u, 1)[0]
            position = np.abs(A - A1).max() / amax
            # (c) ... the altitude dependence: the reference's fixed density
            set_model(None, cst)
            A2 = discretizer(cst, j2, solver, steps).discretize(MG.F, x, u, 1)[0]
            fixed = np.abs(A - A2).max() / amax
            print(f"{name}: drag share {share:.3g}, position block {position:.3g}, against the fixed density {fixed:.3g}, jacobian {jac:.3g}")
            assert share >= 1e-4 and position >= 1e-6 and fixed >= 1e-6, (name, share, position, fixed)
            rec.update({f"drag_share_{name}": np.float64(share), f"position_share_{name}": np.float64(position),
                        f"fixed_density_share_{name}": np.float64(fixed)})
        out.update(rec)
    MG.save("atmo_discretize.npz", cases=np.array([c[0] for c in cases]), **out)


def rollout(y0, const, u_func, n_eval):
    """Simulator.get_trajectory_ODE's solve (simulator.py:185-187) with drag and J2"""
    sol = integrate.solve_ivp(Simulator.satellite_dynamics, [0, 1], y0, args=(u_func, 1, const, True, True),
                              t_eval=np.linspace(0, 1, n_eval), max_step=0.001)
    assert sol.success
    return sol.y


def gen_propagate():
    sat = Satellite(MG.R_HUBBLE, MG.V_HUBBLE, MG.M_HUBBLE)
    scale = SatelliteScale(sat=sat)
    const = scale.get_normalized_constants()
    const.S = const.S * S_SCALE
    y0 = scale.normalize_state(sat.get_state_vector())
    power = Atmosphere.power_law()
    expo = Atmosphere.exponential(float(power.density(H_FIT)), H_FIT, float(-power.density(H_FIT) / power.ddensity(H_FIT)))
    useq = np.random.default_rng(11).normal(size=(3, 12)) * 0.5
    n_eval = 50
    out = {"y0": y0, "const": MG.const_vec(const), "useq": useq, "n_eval": np.int64(n_eval),
           "atmo_power": np.array(power.coefficients()), "atmo_exp": np.array(expo.coefficients())}
    cases = [("power_tan", power, "tan"), ("power_seq", power, "seq"), ("exp_tan", expo, "tan")]
    for name, atm, law in cases:
        ctrl = ConstantTangentialThrustController([sat], 0.5) if law == "tan" else SequenceController(u=useq, tf_u=1, tf_sim=1)
        set_model(atm, const)
        y = rollout(y0, const, ctrl.get_u_func(), n_eval)
        rho = atm.density(np.linalg.norm(y[0:3] * const.R0, axis=0) - RC.R_EARTH)
        ratio = rho.max() / rho.min()
        set_model(None, const)
        y_fixed = rollout(y0, const, ctrl.get_u_func(), n_eval)
        end = np.abs(y[:, -1] - y_fixed[:, -1]).max()
        print(f"{name}: density varies by a factor {ratio:.3g} along the trajectory, end state {end:.3g} from the fixed-density rollout")
        assert ratio >= 2.0 and end >= 1e-6, (name, ratio, end)
        out.update({f"y_{name}": y, f"model_{name}": np.array("power" if atm is power else "exp"), f"law_{name}": np.array(law),
                    f"density_ratio_{name}": np.float64(ratio), f"fixed_density_end_{name}": np.float64(end)})
    MG.save("atmo_propagate.npz", cases=np.array([c[0] for c in cases]), **out)


if __name__ == "__main__":
    os.chdir("/tmp")  # reference code may write files into the CWD
    RSIM.Simulator.get_atmo_density = staticmethod(atmo_density)
    if len(sys.argv) < 2 or sys.argv[1] == "propagate":
        gen_propagate()
    if len(sys.argv) < 2 or sys.argv[1] == "discretize":
        gen_discretize()
