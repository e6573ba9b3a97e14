#!/usr/bin/env python3
"""Golden vectors of the discretisation where ivp_max_step does not clip the steps: the reference's own Discretizer with
ivp_max_step = 1.0 (as make_drag_edges_golden.py runs it, whose helpers this reuses) on the inputs of tests/discretize_cases.py
-- RK23, the uniform-step mode with 2 to 33 points and both together on long intervals, the drag branch under the fixed density
and the general atmosphere on a ragged set of horizons, one interval of a whole horizon.

Runs ONLY in the build container, like make_golden.py; writes discretize_unclipped.npz: arrays only.  The inputs are not stored --
tests/test_discretize_unclipped_host.py rebuilds them from discretize_cases.py -- but their hash is.  `check` as the only argument
compares what it computes with the committed file instead of writing it.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_drag_edges_golden as EG         # noqa: E402  (and through it make_atmo_golden, make_golden: the reference on the path)
AG, MG = EG.AG, EG.MG

import numpy as np                          # noqa: E402

import simulator as RSIM                    # noqa: E402

sys.path.insert(0, os.path.join(HERE, ".."))
import discretize_cases as C                # noqa: E402

NAME = "discretize_unclipped.npz"


def solver_of(mode):
    flag, steps = C.MODES[mode]
    return ("RK23" if flag & C.RK23 else "RK45"), steps


def discretize(c, s, mode):
    """satellite s of the case through the reference at ivp_max_step = 1 -> its five arrays and, in the adaptive modes, the node
    counts and nfev of the solve_ivp calls it makes"""
    x, u, tf, cst = C.sat_inputs(c, s)
    const = EG.Const(cst)
    AG.set_model(C.atmosphere(c), const)
    solver, steps = solver_of(mode)
    d = AG.discretizer(const, bool(c["flags"] & C.J2), solver, steps, drag=bool(c["flags"] & C.DRAG))
    d.ivp_max_step = C.MAX_STEP
    out = dict(zip(C.KEYS, d.discretize(MG.F, x, u, tf)))
    if not steps:
        out["node_counts"], out["nfev"], _, _ = MG.rk_nodes(d, x, u, tf)
    return out


def padded(c, parts, key):
    """the satellites' arrays in one, NaN (-1 for the counts) behind a satellite's own intervals: the interval axis is the last
    of Sigma and xi, the first of the others"""
    n = c["K"] - 1
    out = []
    for p in parts:
        a = np.asarray(p[key])
        axis = a.ndim - 1 if key in ("Sigma", "xi") else 0
        pad = [(0, 0)] * a.ndim
        pad[axis] = (0, n - a.shape[axis])
        out.append(np.pad(a, pad, constant_values=-1) if a.dtype.kind == "i" else np.pad(a, pad, constant_values=np.nan))
    return np.stack(out)


def generate():
    out = {"pairs": np.array([f"{n}.{m}" for n, m in C.ANCHORED])}
    for name in sorted({n for n, _ in C.ANCHORED}):
        out[f"inputs_sha256_{name}"] = np.array(C.input_hash(name))
    for name, mode in C.ANCHORED:
        c = C.case(name)
        assert C.input_hash(name) == str(out[f"inputs_sha256_{name}"])
        parts = [discretize(c, s, mode) for s in range(c["S"])]
        for key in parts[0]:
            out[f"{key}_{name}.{mode}"] = padded(c, parts, key)
        if "nfev" in parts[0]:
            print(f"{name} {mode}: accepted {[(p['node_counts'] - 1).tolist() for p in parts]}, nfev {[p['nfev'].tolist() for p in parts]}")
    return out


if __name__ == "__main__":
    os.chdir("/tmp")  # reference code may write files into the CWD
    RSIM.Simulator.get_atmo_density = staticmethod(AG.atmo_density)
    out = generate()
    if sys.argv[1:] == ["check"]:
        have = np.load(os.path.join(HERE, NAME))
        assert sorted(have.files) == sorted(out), "other arrays than the committed file's"
        for k, v in out.items():
            a, b = np.asarray(v), have[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        print(f"{NAME}: every array reproduced bit for bit")
    else:
        MG.save(NAME, **out)
