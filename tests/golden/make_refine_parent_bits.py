"""Recorded results of the solve kernels where they refine, for tests/test_refine_two_lane_bits_gpu.py: refine_parent_bits.npz.

Run ONCE on an MI355X against the library of the commit BEFORE a change that must keep every bit of the refinement passes
(MPCX_LIB names another build of libmpcx.so, mpconstellation_amd/_ffi.py):

    MPCX_LIB=/path/to/parent/libmpcx.so python tests/golden/make_refine_parent_bits.py [OUT.npz]

The refinement residual (solve_phases.hpp, reduced_residual) works in passes of 32 nodes, two lanes per node.  The cases are the
smallest at which that form takes another path; options, flag constants, FIELDS and workload are those of
make_solve_driver_parent_bits.py:

* stiff terminal windows through the one-wave kernel (flags 16), S = 2, at K = 3, 4, 31, 32, 33 and 63: the shortest horizon, the
  node before a pass ends, the exact pass, the pass plus one node, two passes less one;
* one ragged stiff batch, rows of 65 with 3, 31, 32, 33, 64 and 65 nodes in one launch;
* stiff windows at n_refine = 2, K = 33: two residuals per iteration, zeta carried between them;
* stiff windows with linear_vt=True, K = 30 (the sd.linvt branch of the residual and of the border);
* stiff windows with a fixed final time, K = 30 (the border without dtf);
* stiff and thrust-limited, S = 8, K = 30: refinement is skipped while delta_w > 0 and resumes;
* the stiff K = 30 case through the two-wave (flags 32), LDS-resident (0), time-parallel (64) kernels and, at K = 20, the shared
  final time.

Asserted while recording: every satellite ends with status 0 or 7; every case differs in some bit of X, U, NU, tf or kkt from the
same inputs at n_refine = 0 (a refinement pass ran); the thrust-limited case has regularised iterations; the time-parallel result
differs from the one-wave result in some bit (that kernel ran)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(HERE, "..")); sys.path.insert(0, os.path.join(HERE, "..", ".."))
from make_solve_driver_parent_bits import DEFAULT, FIELDS, NO_LDS, ONE_WAVE, STIFF, THRUST_LIMITED, TIME_PARALLEL      # noqa: E402

RAGGED_KS, RAGGED_ROW = (3, 31, 32, 33, 64, 65), 65
BITS = ("X", "U", "NU", "tf", "kkt")

# name -> (S, K, options, keyword arguments of mpc_step_batch)
CASES = {f"stiff_k{K}": (2, K, STIFF, dict(flags=ONE_WAVE)) for K in (3, 4, 31, 32, 33, 63)}
CASES.update({
    "refine2_k33": (2, 33, STIFF, dict(flags=ONE_WAVE, n_refine=2)),
    "linear_vt": (2, 30, STIFF, dict(flags=ONE_WAVE, linear_vt=True)),
    "fixed_tf": (2, 30, STIFF, dict(flags=ONE_WAVE, fixed_tf=1.0)),
    "thrust_limited": (8, 30, {**STIFF, **THRUST_LIMITED}, dict(flags=ONE_WAVE)),
    "one_wave": (2, 30, STIFF, dict(flags=ONE_WAVE)),
    "two_wave": (2, 30, STIFF, dict(flags=NO_LDS)),
    "lds": (2, 30, STIFF, dict(flags=DEFAULT)),
    "time_parallel": (2, 30, STIFF, dict(flags=TIME_PARALLEL)),
    "shared_tf": (2, 20, STIFF, dict(shared_tf=True, linear_vt=True)),
})
NAMES = list(CASES) + ["ragged"]


def run_case(name, **override):
    from mpconstellation_amd import mpc_step_batch
    from test_full_size_gpu import workload
    S, K, opts, kw = CASES[name]
    xbar, ubar, consts, r_des = workload(4096, K, first=0, count=S)
    return mpc_step_batch(xbar, ubar, np.ones(S), consts, r_des, options=opts, regularised=True, **{**kw, **override})


def run_ragged(**override):
    """satellite s: its own rollout at RAGGED_KS[s] nodes in the first columns of a row of RAGGED_ROW"""
    from mpconstellation_amd import mpc_step_batch
    from test_full_size_gpu import workload
    S = len(RAGGED_KS)
    xbar = np.zeros((S, 7, RAGGED_ROW)); ubar = np.zeros((S, 3, RAGGED_ROW))
    _, _, consts, r_des = workload(4096, RAGGED_ROW, first=0, count=S)
    r_des = r_des.copy()
    for s, k in enumerate(RAGGED_KS):
        x, u, _, rd = workload(4096, k, first=s, count=1)
        xbar[s, :, :k] = x[0]; ubar[s, :, :k] = u[0]; r_des[s] = rd[0]
    return mpc_step_batch(xbar, ubar, np.ones(S), consts, r_des, options=STIFF, Ks=np.array(RAGGED_KS, dtype=np.int32), regularised=True,
                          **{**dict(flags=ONE_WAVE), **override})


def run(name, **override):
    return run_ragged(**override) if name == "ragged" else run_case(name, **override)


def main():
    from mpconstellation_amd import _ffi
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "refine_parent_bits.npz")
    print("library:", _ffi.LIB_PATH)
    arrays, failed = {}, []
    for name in NAMES:
        r = run(name)
        rec = {f: np.asarray(getattr(r, f)).copy() for f in FIELDS}
        r0 = run(name, n_refine=0)
        plain = {f: np.asarray(getattr(r0, f)).copy() for f in BITS}
        refined = any(not np.array_equal(rec[f], plain[f]) for f in BITS)
        st = rec["status"]
        print(f"{name}: status {st.tolist()}, iterations {rec['iters'].tolist()}, regularised {rec['n_regularised'].tolist()}, "
              f"differs from n_refine = 0: {refined} (status there {np.asarray(r0.status).tolist()})", flush=True)
        if not np.isin(st, (0, 7)).all():
            failed.append(f"{name}: status {st.tolist()}")
        if not refined:
            failed.append(f"{name}: equal to n_refine = 0 in every bit, no refinement pass ran")
        for f in FIELDS:
            arrays[f"{name}.{f}"] = rec[f]
    if arrays["thrust_limited.n_regularised"].sum() == 0:
        failed.append("thrust_limited: no regularised iteration")
    # (the time-parallel algebra rounds differently from the sequential one: equal bits would mean the launch fell back)
    if all(np.array_equal(arrays[f"time_parallel.{f}"], arrays[f"one_wave.{f}"]) for f in BITS):
        failed.append("time_parallel: equal to the one-wave result in every bit, that kernel did not run")
    assert not failed, "\n".join(failed)
    np.savez_compressed(out_path, **arrays)
    print(f"wrote {out_path}: {os.path.getsize(out_path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
