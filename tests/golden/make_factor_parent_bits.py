#!/usr/bin/env python3
"""Bits of the solver BEFORE the factorisation's LDS arrays were re-laid for wide reads (Pn with row stride 8, WlLi
transposed: csrc/solve_riccati.hpp): inputs and results of a handful of small batches, written by the library built from the
commit before that change.  tests/test_factor_wide_lds_gpu.py holds every later build to them with array_equal.

Needs an MI355X and the OLD library: build the parent commit in a checkout of its own and name its libmpcx.so in MPCX_LIB
(mpconstellation_amd/_ffi.py loads that file instead of the tree's own):

    MPCX_LIB=/path/to/parent/mpconstellation_amd/libmpcx.so python tests/golden/make_factor_parent_bits.py [OUT.npz]

`check` as the only argument runs whatever library is loaded on the stored inputs and compares instead of writing.

Per case the file holds the inputs (xbar, ubar, consts, r_des, Ks for the ragged batch; the options are in CASES below) and, per
kernel selection (flags 0: the default -- LDS-resident and two-wave builds at these sizes --, 16: the one-wave kernel, 64: the
time-parallel kernel where K >= 24, whose bits are its own), X, U, NU, tf, status, iters and kkt.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

NAME = "factor_parent_bits.npz"
FIELDS = ("X", "U", "NU", "tf", "status", "iters", "kkt")
# name: (satellites, row length K, node counts of a ragged batch or None, solver options)
CASES = {
    "k3": (4, 3, None, {}),                     # the loop body runs exactly once between the peeled terminal node and node 0
    "k4": (4, 4, None, {}),
    "k30": (6, 30, None, {}),                   # the benchmark constellation
    "ragged": (3, 30, (3, 17, 30), {}),
    "options": (4, 30, None, {"eps_r": 1e-3, "w_tr": 0.01, "tf_max": 3.0, "u_lim": [0, 2.0]}),       # test_solve_gpu.py's option set
    "stiff": (4, 30, None, {"eps_r": 1e-6, "eps_vr": 1e-16, "tf_max": 1.0}),     # stiff terminal windows: refinement keeps Pt
    "thrust": (4, 30, None, {"u_lim": [0, 0.3]}),                                # limit below the reference thrust: regularised iterations
}


def flag_sets(K):
    return (0, 16, 64) if K >= 24 else (0, 16)


def inputs(S, K, Ks):
    """the first S satellites of the benchmark constellation under the benchmark's reference thrust"""
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.constellation import constellation_states, normalize_batch, tangential_thrust
    from mpconstellation_amd.simulator import propagate_batch
    y0, consts = normalize_batch(constellation_states(4096, first=0, count=S))
    xbar, st, _ = propagate_batch(y0, np.ones(S), consts, (_ffi.CTRL_TANGENTIAL, np.array([0.5]), 0, None), K)
    assert (st == 0).all()
    ubar = np.ascontiguousarray(tangential_thrust(xbar, 0.5))
    if Ks is None:
        return xbar, ubar, consts, np.linalg.norm(xbar[:, :3, -1], axis=1)
    for s, k in enumerate(Ks):
        xbar[s, :, k:] = 0.0; ubar[s, :, k:] = 0.0
    return xbar, ubar, consts, np.array([np.linalg.norm(xbar[s, :3, k - 1]) for s, k in enumerate(Ks)])


def solve(xbar, ubar, consts, r_des, Ks, opts, flags):
    from mpconstellation_amd import mpc_step_batch
    ks = None if Ks is None else np.asarray(Ks, dtype=np.int32)
    r = mpc_step_batch(xbar, ubar, np.ones(len(r_des)), consts, r_des, options=dict(opts), Ks=ks, flags=flags)
    return {f: np.asarray(getattr(r, f)) for f in FIELDS}


def main():
    check = sys.argv[1:] == ["check"]
    path = os.path.join(HERE, NAME) if check or not sys.argv[1:] else sys.argv[1]
    old = np.load(path) if check else None
    out, bad = {}, 0
    for name, (S, K, Ks, opts) in CASES.items():
        if check:
            xbar, ubar, consts, r_des = (old[f"{name}.{k}"] for k in ("xbar", "ubar", "consts", "r_des"))
        else:
            xbar, ubar, consts, r_des = inputs(S, K, Ks)
            out.update({f"{name}.xbar": xbar, f"{name}.ubar": ubar, f"{name}.consts": consts, f"{name}.r_des": r_des})
        for flags in flag_sets(K):
            res = solve(xbar, ubar, consts, r_des, Ks, opts, flags)
            ok = np.isin(res["status"], (0, 7)).all()
            print(f"{name:8s} flags {flags:2d}: status {res['status'].tolist()} iters {res['iters'].tolist()}" + ("" if ok else "  NOT CONVERGED"))
            for f in FIELDS:
                if check:
                    same = np.array_equal(res[f], old[f"{name}.f{flags}.{f}"])
                    bad += not same
                    if not same: print(f"    {f}: differs from {NAME}")
                else:
                    out[f"{name}.f{flags}.{f}"] = res[f]
    if check:
        print("identical" if not bad else f"{bad} arrays differ")
        return 1 if bad else 0
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
