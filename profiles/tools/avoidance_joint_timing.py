"""profiling helper: duration of the joint avoidance step by HIP events on its stream.
  mpcx_avoidance_joint_dev for n = 1024 and n = 65 536 rows in the all-pairs form: avoidance_timing.py's plan and lists (random pairs
  i < j of S = 4096 thrusting satellites of a random LEO shell, K = 30 and K = 100 nodes over one orbit, random times in the last 95 %
  of the span, target 1e9 m beyond every pair so that every row is violated), object i moving, without rows / tsens, in three settings:
  no ball and no hold; the terminal hold; the hold and a ball at 0.9 of each satellite's largest |ubar + du| of the hold run.  Beside
  them mpcx_avoidance_dev (i moves) and mpcx_discretize_stages_ragged_dev alone on the same plan, the calls alternating.  Statuses and
  Newton iteration counts of every setting are printed (with 65 536 pairs a satellite has 16 rows on average: more than
  MPCX_AJ_MAX_ROWS, MPCX_ST_BADK -- the call is then the rows kernel and the gather).
Every shape is warmed up WARM times and timed REPS times in one process; median, minimum and maximum are printed."""
import ctypes as C, os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conjunction_reference as R

WARM, REPS = 3, 20

import torch
from mpconstellation_amd import _ffi
from mpconstellation_amd.constellation import normalize_batch
lib = _ffi.load(); ctx = _ffi.context(0)
dev = torch.device("cuda", 0)
p = lambda t: C.c_void_p(t.data_ptr())
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
T = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
E = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    assert fn() == 0
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(runs):
    """runs: name -> call; alternating; -> name -> median ms"""
    for _ in range(WARM):
        for fn in runs.values():
            timed(fn)
    ms = {k: [] for k in runs}
    for _ in range(REPS):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    for k, v in ms.items():
        print(f"    {k:44s} median {statistics.median(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  ({len(v)} runs)", flush=True)
    return {k: statistics.median(v) for k, v in ms.items()}


def histogram(x):
    v, c = np.unique(x, return_counts=True)
    return ", ".join(f"{int(a)}: {int(b)}" for a, b in zip(v, c))


S = 4096
rng = np.random.default_rng(0)
for K in (30, 100):
    orb = R.random_orbits(S, seed=K)
    T1 = 2 * np.pi / np.sqrt(R.MU_EARTH / 6.9e6 ** 3)
    Y, units, span = R.trajectories(orb, K, (0.0, T1))
    state = np.zeros((S, 7)); state[:, 0] = units[:, 0]; state[:, 6] = 1.0
    consts = normalize_batch(state)[1]
    dY, dU, du, dsp, dc = T(Y), T(0.01 * rng.standard_normal((S, 3, K))), T(units), T(span), T(consts)
    dtf, stage, dst2 = T((span[:, 1] - span[:, 0]) / units[:, 1]), E((S, K - 1, _ffi.STAGE_DOUBLES)), E(S, torch.int32)
    for n in (1024, 65536):
        i = rng.integers(0, S - 1, n); j = rng.integers(i + 1, S)
        pairs = np.column_stack([i, j, np.zeros(n), rng.uniform(0.05 * T1, T1, n)]).astype(np.float64)
        dpairs, out, ddu, pst = T(pairs), E((n, _ffi.NAV)), E((n, 2, 3, K)), E(n, torch.int32)
        jdu, jso, jro, jss, jrs = E((S, 3, K)), E((S, _ffi.NAJ)), E((n, _ffi.NAR)), E(S, torch.int32), E(n, torch.int32)
        dumax = T(np.full(S, np.inf))
        ws = E(max(lib.mpcx_avoidance_workspace_bytes(n, S, K), lib.mpcx_avoidance_joint_workspace_bytes(n, S, K)), torch.uint8)

        def joint(hold, ball):
            return lambda: lib.mpcx_avoidance_joint_dev(ctx, n, p(dpairs), None, S, K, None, p(dY), p(dU), p(du), p(dsp), p(dc), _ffi.FLAG_J2, 1e-2,
                                                        None, 0, 0, None, None, None, None, None, R.MU_EARTH, 1.0e9, p(dumax) if ball else None,
                                                        hold, _ffi.AJ_DEFAULT_TOL, _ffi.AJ_DEFAULT_MAX_ITER, 0, S, p(jdu), p(jso), p(jro), None, None,
                                                        p(jss), p(jrs), p(ws), st)

        def report(name):
            torch.cuda.synchronize()
            ss, so = jss.cpu().numpy(), jso.cpu().numpy()
            ok = (ss == 0) & (so[:, _ffi.AJ_ROWS] > 0)
            print(f"    {name}: satellite statuses {{{histogram(ss)}}}, row statuses {{{histogram(jrs.cpu().numpy())}}}; of the {int(ok.sum())} solved: rows "
                  f"{{{histogram(so[ok, _ffi.AJ_ROWS])}}}, iterations {{{histogram(so[ok, _ffi.AJ_ITERS])}}}, nodes on the ball {{{histogram(so[ok, _ffi.AJ_ONBALL])}}}",
                  flush=True)
            return ss, so
        print(f"avoidance_joint n {n} (all-pairs form, S {S}, K {K}, J2, target in metres, no rows / tsens)", flush=True)
        assert joint(1, False)() == 0
        ss, so = report("hold, no ball")
        dumax.copy_(T(np.where((ss == 0) & (so[:, _ffi.AJ_ROWS] > 0), 0.9 * so[:, _ffi.AJ_UMAX], np.inf)))
        assert joint(1, True)() == 0
        report("hold and ball")
        assert joint(0, False)() == 0
        report("no hold, no ball")
        med = measure({"mpcx_avoidance_joint_dev, no hold, no ball": joint(0, False), "mpcx_avoidance_joint_dev, hold": joint(1, False),
                       "mpcx_avoidance_joint_dev, hold and ball": joint(1, True),
                       "mpcx_avoidance_dev, i moves": lambda: lib.mpcx_avoidance_dev(
                           ctx, n, p(dpairs), S, K, None, p(dY), p(dU), p(du), p(dsp), p(dc), _ffi.FLAG_J2, 1e-2, None, 0, 0, None, None, None, None,
                           None, R.MU_EARTH, 1.0e9, 0, p(out), p(ddu), None, p(pst), p(ws), st),
                       "mpcx_discretize_stages_ragged_dev alone": lambda: lib.mpcx_discretize_stages_ragged_dev(
                           ctx, S, K, None, K, None, p(dY), p(dU), p(dtf), p(dc), _ffi.FLAG_J2, 1e-2, p(stage), p(dst2), st)})
        d = med["mpcx_discretize_stages_ragged_dev alone"]
        for k in med:
            if k != "mpcx_discretize_stages_ragged_dev alone":
                print(f"    {k} less the linearisation (difference of the medians): {med[k] - d:.3f} ms", flush=True)
        del dpairs, out, ddu, ws, jdu, jso, jro
        torch.cuda.empty_cache()
