"""Recorded results of the solve kernels for tests/test_solve_driver_bits_gpu.py: solve_driver_parent_bits.npz.

Run ONCE on an MI355X against the library of the commit BEFORE a change that must keep every bit of the solver (MPCX_LIB names
another build of libmpcx.so, mpconstellation_amd/_ffi.py):

    MPCX_LIB=/path/to/parent/libmpcx.so python tests/golden/make_solve_driver_parent_bits.py [OUT.npz]

The cases are the smallest at which the driver of a solve (solve_driver.hpp) and the phases it calls take another path:

* K = 3, the shortest horizon, S = 3;
* one ragged batch, rows of 40 with 3, 17, 32, 33 and 40 nodes -- 32 is the pass length of the phases that run two lanes per
  node -- and one row with a count the solver refuses (status 9);
* K = 64, 65 and 70, S = 2, with stiff terminal windows: the refinement residual runs in passes of 64 nodes;
* stiff terminal windows at n_refine = 0, 1 and 2 (0 and 1 must differ in bits: the refinement pass ran);
* a thrust limit that makes iterations regularise (the retry loop): the counts must not all be zero;
* one case through each kernel: one-wave (flags 16), two-wave (32: no LDS residence), LDS-resident (0, S <= 256 and
  K <= 30), time-parallel (64, K >= 24) and the shared final time.

Every satellite must end with status 0 or 7, the refused row apart.  The inputs come from the package's own constellation and
rollout (tests/test_full_size_gpu.py, workload), which the test calls again."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..")); sys.path.insert(0, os.path.join(HERE, "..", ".."))

FIELDS = ("X", "U", "NU", "tf", "status", "iters", "kkt", "n_regularised", "first_regularised")
# mpcx_solve_opts.flags (include/mpcx.h).  NO_LDS without ONE_WAVE runs the two-wave kernel at these batch sizes; DEFAULT the
# LDS-resident one (S <= 256, K <= 30) and TIME_PARALLEL the time-parallel one (K >= 24) where the device has room for them --
# which kernel a launch goes through is the library's choice (main() checks what it can tell apart)
ONE_WAVE, NO_LDS, DEFAULT, TIME_PARALLEL = 16, 32, 0, 64
STIFF = {"eps_r": 1e-6, "eps_vr": 1e-16, "tf_max": 1.0}        # stiff terminal windows: refinement passes
THRUST_LIMITED = {"u_lim": [0, 0.3]}                           # thrust ball active: regularised iterations
RAGGED_KS, RAGGED_ROW, BADK = (3, 17, 32, 33, 40, 2), 40, 5     # (the last row: a count below 3, MPCX_ST_BADK)
ST_BADK = 9

# name -> (S, K, options, keyword arguments of mpc_step_batch)
CASES = {
    "k3": (3, 3, {}, dict(flags=DEFAULT)),
    "k64_stiff": (2, 64, STIFF, dict(flags=ONE_WAVE)),
    "k65_stiff": (2, 65, STIFF, dict(flags=ONE_WAVE)),
    "k70_stiff": (2, 70, STIFF, dict(flags=ONE_WAVE)),
    "refine0": (4, 30, STIFF, dict(flags=ONE_WAVE, n_refine=0)),
    "refine1": (4, 30, STIFF, dict(flags=ONE_WAVE, n_refine=1)),
    "refine2": (4, 30, STIFF, dict(flags=ONE_WAVE, n_refine=2)),
    "regularised": (16, 30, THRUST_LIMITED, dict(flags=ONE_WAVE)),
    "one_wave": (4, 30, {}, dict(flags=ONE_WAVE)),
    "two_wave": (4, 30, {}, dict(flags=NO_LDS)),
    "lds": (4, 30, {}, dict(flags=DEFAULT)),
    "time_parallel": (2, 30, {}, dict(flags=TIME_PARALLEL)),
    "shared_tf": (2, 20, {}, dict(shared_tf=True, linear_vt=True)),
}


def run_case(name):
    from mpconstellation_amd import mpc_step_batch
    from test_full_size_gpu import workload
    S, K, opts, kw = CASES[name]
    xbar, ubar, consts, r_des = workload(4096, K, first=0, count=S)
    return mpc_step_batch(xbar, ubar, np.ones(S), consts, r_des, options=opts, regularised=True, **kw)


def run_ragged():
    """satellite s: its own rollout at RAGGED_KS[s] nodes in the first columns of a row of RAGGED_ROW (the refused row: a full row)"""
    from mpconstellation_amd import mpc_step_batch
    from test_full_size_gpu import workload
    S = len(RAGGED_KS)
    xbar = np.zeros((S, 7, RAGGED_ROW)); ubar = np.zeros((S, 3, RAGGED_ROW))
    _, _, consts, r_des = workload(4096, RAGGED_ROW, first=0, count=S)
    r_des = r_des.copy()
    for s, k in enumerate(RAGGED_KS):
        k = RAGGED_ROW if s == BADK else k
        x, u, _, rd = workload(4096, k, first=s, count=1)
        xbar[s, :, :k] = x[0]; ubar[s, :, :k] = u[0]; r_des[s] = rd[0]
    return mpc_step_batch(xbar, ubar, np.ones(S), consts, r_des, Ks=np.array(RAGGED_KS, dtype=np.int32), regularised=True, flags=ONE_WAVE)


def run_all():
    """{name: SolveResult} of every case (each runs once)"""
    out = {name: run_case(name) for name in CASES}
    out["ragged"] = run_ragged()
    return out


def main():
    from mpconstellation_amd import _ffi
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "solve_driver_parent_bits.npz")
    print("library:", _ffi.LIB_PATH)
    res = run_all()
    arrays = {}
    for name, r in res.items():
        st = np.asarray(r.status)
        print(f"{name}: status {st.tolist()}, iterations {np.asarray(r.iters).tolist()}, regularised {np.asarray(r.n_regularised).tolist()}")
        ok = np.isin(st, (0, 7))
        if name == "ragged":
            assert st[BADK] == ST_BADK, st
            ok[BADK] = True
        assert ok.all(), (name, st)
        for f in FIELDS:
            arrays[f"{name}.{f}"] = np.asarray(getattr(r, f)).copy()
    assert any(not np.array_equal(arrays[f"refine0.{f}"], arrays[f"refine1.{f}"]) for f in ("X", "U", "NU", "tf", "kkt")), \
        "n_refine = 0 and 1 agree in every bit: no refinement pass ran"
    assert arrays["regularised.n_regularised"].sum() > 0, "no regularised iteration: the retry loop did not run"
    # (the time-parallel algebra rounds differently from the sequential one: equal bits would mean the launch fell back)
    assert not np.array_equal(arrays["time_parallel.X"], arrays["one_wave.X"][:2]), "the time-parallel kernel did not run"
    np.savez_compressed(out_path, **arrays)
    print(f"wrote {out_path}: {os.path.getsize(out_path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
