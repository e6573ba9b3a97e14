#!/usr/bin/env python3
"""Golden vectors of the linearisation WITH drag: the reference's own include_drag=True branch of Discretizer
(linearize_discretize.py:162-173), made runnable.

As shipped, that branch cannot run: Constants has no CD and rho_func / drho_func default to None.  Here it gets the
simulator's atmosphere -- the fixed density 9.983e-13 kg/m^3 normalised by const.RHO (simulator.py:112, 152), drho = 0 -- and
C_D of constants.py; f = Simulator.satellite_dynamics applies the same drag to the state column and Sigma.  The density
functions are module-level: the reference's discretize ships its Discretizer through multiprocessing.Pool, which cannot
pickle lambdas.

Runs ONLY in the build container, like make_golden.py (whose import shims and helpers it reuses); writes
drag_discretize.npz.  Not disc_*.npz: the drag-free discretize tests glob that pattern.
"""
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as MG                    # noqa: E402  (registers the pyomo placeholders, puts the reference on the path)

import numpy as np                          # noqa: E402

import constants as RC                      # noqa: E402
from linearize_discretize import Discretizer  # noqa: E402
from control import ConstantTangentialThrustController  # noqa: E402
from satellite import Satellite             # noqa: E402
from satellite_scale import SatelliteScale  # noqa: E402

RHO_500 = 9.983e-13
S_SCALE = 1e4
_RHO_NORM = [None]          # const.RHO of the satellite being discretised (set before every case)


def rho_func(r):
    return RHO_500 / _RHO_NORM[0]


def drho_func(r):
    return 0.0


def drag_discretizer(const, j2):
    const = copy.copy(const)
    const.CD = RC.C_D
    _RHO_NORM[0] = const.RHO
    return Discretizer(const, rho_func=rho_func, drho_func=drho_func, include_drag=True, include_J2=j2)


def main():
    sat = Satellite(MG.R_HUBBLE, MG.V_HUBBLE, MG.M_HUBBLE)
    scale = SatelliteScale(sat=sat)
    const = scale.get_normalized_constants()
    const_big = copy.copy(const)
    const_big.S = const.S * S_SCALE
    ctrl = ConstantTangentialThrustController([sat], 0.5)
    x30, t30, u30 = MG.reference_case(sat, scale, ctrl, 1, 30)
    x12, t12, u12 = MG.reference_case(sat, scale, ctrl, 1, 12)
    out = {}
    cases = [
        # name, x, t, u, const, J2, ivp_solver, uniform steps (0: adaptive), store the accepted step nodes
        ("tan_K30_tf1", x30, t30, u30, const, False, "RK45", 0, True),
        ("tan_K30_tf1_J2", x30, t30, u30, const, True, "RK45", 0, False),
        ("tan_K30_tf1_bigS", x30, t30, u30, const_big, False, "RK45", 0, True),
        ("tan_K30_tf1_bigS_J2", x30, t30, u30, const_big, True, "RK45", 0, False),
        ("tan_K12_tf1_uni11_bigS", x12, t12, u12, const_big, False, "RK45", 11, False),
        ("tan_K30_tf1_rk23_bigS_J2", x30, t30, u30, const_big, True, "RK23", 0, True),
    ]
    for name, x, t, u, cst, j2, solver, steps, nodes in cases:
        d = drag_discretizer(cst, j2)
        d.ivp_solver = solver
        if steps:
            d.use_uniform_steps = True; d.integrator_steps = steps
        A, Bp, Bn, Sig, xi = d.discretize(MG.F, x, u, 1)
        # the same linearisation without drag: how much of A the drag partials are
        d0 = Discretizer(cst, include_drag=False, include_J2=j2)
        d0.ivp_solver = solver
        if steps:
            d0.use_uniform_steps = True; d0.integrator_steps = steps
        A0 = d0.discretize(MG.F, x, u, 1)[0]
        share = np.abs(A - A0).max() / np.abs(A).max()
        print(f"{name}: max|A - A(no drag)| / max|A| = {share:.3g}")
        if cst is const_big:
            assert share >= 1e-4, (name, share)
        out.update({f"x_{name}": x, f"t_{name}": t, f"u_{name}": u, f"tf_{name}": np.float64(1), f"const_{name}": MG.const_vec(cst),
                    f"j2_{name}": np.bool_(j2), f"solver_{name}": np.array(solver), f"steps_{name}": np.int64(steps),
                    f"A_{name}": A, f"Bp_{name}": Bp, f"Bn_{name}": Bn, f"Sigma_{name}": Sig, f"xi_{name}": xi,
                    f"drag_share_{name}": np.float64(share)})
        if nodes:
            counts, nfev, nt, ny = MG.rk_nodes(d, x, u, 1)
            out.update({f"node_counts_{name}": counts, f"node_t_{name}": nt})
    MG.save("drag_discretize.npz", cases=np.array([c[0] for c in cases]), **out)


if __name__ == "__main__":
    os.chdir("/tmp")  # reference code may write files into the CWD
    main()
