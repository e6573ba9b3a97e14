#!/usr/bin/env python3
"""Golden vectors of the drag and atmosphere away from the Hubble's tangential climb: the reference's own drag branch and rollout
(as make_atmo_golden.py runs them, whose helpers this reuses) on the inputs of tests/drag_cases.py that the reference can
compute -- low inclined orbits with random thrust directions and tf != 1, the density model with c1 and c2 both non-zero, the
orbit that crosses the model's floor, every thrust law through the atmosphere with and without J2.

Runs ONLY in the build container, like make_golden.py; writes drag_edges.npz: arrays only, the inputs beside the results, and
what the generator measured about each input's sensitivity.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_atmo_golden as AG               # noqa: E402  (and through it make_golden: the reference on the path)
MG = AG.MG

import numpy as np                          # noqa: E402
from scipy import integrate                 # noqa: E402

import simulator as RSIM                    # noqa: E402
from simulator import Simulator             # noqa: E402
from control import Controller, ConstantThrustController, ConstantTangentialThrustController, SequenceController  # noqa: E402
from satellite import Satellite             # noqa: E402

sys.path.insert(0, os.path.join(HERE, ".."))
import drag_cases as D                      # noqa: E402

CONST_KEYS = MG.CONST_KEYS
SOLVER = {"rk45": ("RK45", 0), "rk23": ("RK23", 0), "uni11": ("RK45", 11)}


class Const:
    """a Constants object of the reference from the eight normalised numbers"""

    def __init__(self, vec):
        for k, v in zip(CONST_KEYS, vec):
            setattr(self, k, float(v))


def discretize(x, u, tf, cst, atm, solver, j2, drag=True, no_drho=False, nodes=False):
    const = Const(cst)
    AG.set_model(atm, const, no_drho=no_drho)
    d = AG.discretizer(const, j2, *SOLVER[solver], drag=drag)
    out = dict(zip(D.KEYS, d.discretize(MG.F, x, u, tf)))
    if nodes:
        out["node_counts"], _, out["node_t"], _ = MG.rk_nodes(d, x, u, tf)
    return out


def shares(x, u, tf, cst, atm, solver, j2, A):
    """how much of A the drag is, its position block, its altitude dependence (make_atmo_golden.py (a)-(c))"""
    amax = np.abs(A).max()
    drag = np.abs(A - discretize(x, u, tf, cst, atm, solver, j2, drag=False)["A"]).max() / amax
    if atm is None:
        return drag, 0.0, 0.0
    position = np.abs(A - discretize(x, u, tf, cst, atm, solver, j2, no_drho=True)["A"]).max() / amax
    fixed = np.abs(A - discretize(x, u, tf, cst, None, solver, j2)["A"]).max() / amax
    return drag, position, fixed


def rollout(y0, tf, cst, atm, u_func, n_eval, j2):
    """Simulator.get_trajectory_ODE's solve (simulator.py:185-187)"""
    const = Const(cst)
    AG.set_model(atm, const)
    sol = integrate.solve_ivp(Simulator.satellite_dynamics, [0, 1], y0, args=(u_func, tf, const, True, j2),
                              t_eval=np.linspace(0, 1, n_eval), max_step=0.001)
    assert sol.success
    return sol.y


def gen_batch(out):
    b = D.batch()
    S = b["x"].shape[0]
    out.update({f"batch_{k}": b[k] for k in ("x", "u", "tf", "const", "y0")})
    out["batch_configs"] = np.array(["/".join([m, s, "j2" if j else "nj2"]) for m, s, j in D.REFERENCE_CONFIGS])
    for (model, solver, j2), tag in zip(D.REFERENCE_CONFIGS, out["batch_configs"]):
        atm = D.models()[model]
        if atm is not None:
            out[f"batch_atmo_{model}"] = np.array(atm.coefficients())
        rs = [discretize(b["x"][s], b["u"][s], b["tf"][s], b["const"][s], atm, solver, j2, nodes=(solver != "uni11")) for s in range(S)]
        for k in D.KEYS:
            out[f"batch_{k}_{tag}"] = np.stack([r[k] for r in rs])
        if solver != "uni11":
            out[f"batch_node_counts_{tag}"] = np.stack([r["node_counts"] for r in rs])
            out[f"batch_node_t_{tag}"] = np.concatenate([r["node_t"] for r in rs])
        sh = np.array([shares(b["x"][s], b["u"][s], b["tf"][s], b["const"][s], atm, solver, j2, rs[s]["A"]) for s in range(S)])
        print(f"batch {tag}: drag share {sh[:, 0]}, position block {sh[:, 1]}, against the fixed density {sh[:, 2]}")
        big = D.BIG_S
        assert (sh[big, 0] >= 1e-7).all() and (atm is None or ((sh[big, 1] >= 1e-7).all() and (sh[big, 2] >= 1e-7).all())), (tag, sh)
        out[f"batch_shares_{tag}"] = sh


def gen_floor(out):
    atm = D.floor_model()
    out["floor_atmo"] = np.array(atm.coefficients())
    for tf in D.FLOOR_TFS:
        c = D.floor_case(tf)
        t = f"tf{int(tf)}"
        out.update({f"floor_{k}_{t}": c[k] for k in ("x", "u", "const", "y0")})
        for solver in ("rk45", "rk23"):
            r = discretize(c["x"], c["u"], tf, c["const"], atm, solver, True, nodes=True)
            out.update({f"floor_{k}_{t}_{solver}": v for k, v in r.items()})
            sh = shares(c["x"], c["u"], tf, c["const"], atm, solver, True, r["A"])
            # ... and the floor itself: the same model with the floor below the whole orbit
            low = D.Atmosphere(atm.c0, atm.c1, atm.c2, 1e5)
            floor = np.abs(r["A"] - discretize(c["x"], c["u"], tf, c["const"], low, solver, True)["A"]).max() / np.abs(r["A"]).max()
            print(f"floor {t} {solver}: drag share {sh[0]:.3g}, position block {sh[1]:.3g}, fixed density {sh[2]:.3g}, the floor {floor:.3g}")
            assert min(sh) >= 1e-7 and floor >= 1e-7
            out[f"floor_shares_{t}_{solver}"] = np.array(list(sh) + [floor])
        ctrl = SequenceController(u=c["u"], tf_u=1, tf_sim=1)
        y = rollout(c["y0"], tf, c["const"], atm, ctrl.get_u_func(), 20, True)
        end = np.abs(y[:, -1] - rollout(c["y0"], tf, c["const"], D.Atmosphere(atm.c0, atm.c1, atm.c2, 1e5), ctrl.get_u_func(), 20, True)[:, -1]).max()
        print(f"floor {t} rollout: end state {end:.3g} from the rollout without the floor")
        assert end >= 1e-7
        out[f"floor_y_{t}"] = y
        out[f"floor_y_end_share_{t}"] = np.float64(end)


def gen_rollouts(out):
    c = D.rollout_case()
    atm = D.models()["general"]
    out["roll_atmo"] = np.array(atm.coefficients())
    out.update({f"roll_{k}": c[k] for k in ("y0", "const", "tf", "n_eval", "end_tau", "constant", "tangential", "sequence")})
    sat = Satellite(MG.R_HUBBLE, MG.V_HUBBLE, MG.M_HUBBLE)       # (the controllers keep a list of satellites and never read it here)
    for law in D.LAWS:
        for j2 in (False, True):
            for s in range(3):
                ctrl = {"zero": lambda: Controller, "constant": lambda: ConstantThrustController([sat], c["constant"][s]),
                        "tangential": lambda: ConstantTangentialThrustController([sat], c["tangential"][s]),
                        "sequence": lambda: SequenceController(u=c["sequence"][s], tf_u=c["end_tau"][s], tf_sim=1)}[law]()
                assert law != "sequence" or ctrl.end_tau == c["end_tau"][s]
                y = rollout(c["y0"][s], c["tf"][s], c["const"][s], atm, ctrl.get_u_func(), int(c["n_eval"][s]), j2)
                end = np.abs(y[:, -1] - rollout(c["y0"][s], c["tf"][s], c["const"][s], None, ctrl.get_u_func(), int(c["n_eval"][s]), j2)[:, -1]).max()
                print(f"rollout {law} j2={j2} sat {s}: end state {end:.3g} from the fixed-density rollout")
                assert end >= 1e-7
                tag = f"{law}_{'j2' if j2 else 'nj2'}_{s}"
                out[f"roll_y_{tag}"] = y
                out[f"roll_end_share_{tag}"] = np.float64(end)


if __name__ == "__main__":
    os.chdir("/tmp")  # reference code may write files into the CWD
    RSIM.Simulator.get_atmo_density = staticmethod(AG.atmo_density)
    out = {}
    gen_batch(out)
    gen_floor(out)
    gen_rollouts(out)
    MG.save("drag_edges.npz", **out)
