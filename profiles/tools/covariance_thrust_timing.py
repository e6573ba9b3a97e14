"""profiling helper: durations of the covariance with thrust execution errors by HIP events on its stream.
  mpcx_covariance_thrust_batch_dev at S = 4096 satellites of a random LEO shell, K = 30 and K = 100 nodes over one orbit, J2 on, a
  thrust table of 0.02 standard_normal, q = 1e-8, execution errors of 2 % in magnitude and 1 degree in pointing with fixed parts of
  1e-4, a mass variance of 1e-4; beside it mpcx_covariance_batch_dev on the same inputs (the same linearisation, the 6 x 6 chain) and
  mpcx_discretize_stages_ragged_dev alone (both calls' first and largest step), the three alternating; the chains are the differences
  of the medians.
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
        print(f"    {k:58s} median {statistics.median(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  ({len(v)} runs)", flush=True)
    return {k: statistics.median(v) for k, v in ms.items()}


def shell(S, K, seed):
    orb = R.random_orbits(S, seed=seed)
    T1 = 2 * np.pi / np.sqrt(R.MU_EARTH / 6.9e6 ** 3)
    Y, units, span = R.trajectories(orb, K, (0.0, T1))
    state = np.zeros((S, 7)); state[:, 0] = units[:, 0]; state[:, 6] = 1.0
    return Y, units, span, normalize_batch(state)[1]


P0 = np.diag([100.0 ** 2] * 3 + [0.1 ** 2] * 3)
EXEC = np.array([1e-4, 0.02, 1e-4, 0.01745, 1e-3])
S = 4096
for K in (30, 100):
    Y, units, span, consts = shell(S, K, seed=K)
    U = 0.02 * np.random.default_rng(K).standard_normal((S, 3, K))
    dY, dU, du, dsp, dc = T(Y), T(U), T(units), T(span), T(consts)
    dP0, dq = T(np.broadcast_to(P0, (S, 6, 6))), T(np.full(S, 1e-8))
    dex, dmv = T(np.broadcast_to(EXEC, (S, 5))), T(np.full(S, 1e-4))
    dP, dPm, dPc, dst, dstc = E((S, K, 6, 6)), E((S, K, 7)), E((S, K, 6, 6)), E(S, torch.int32), E(S, torch.int32)
    ws = E(lib.mpcx_covariance_thrust_workspace_bytes(S, K), torch.uint8)
    wsc = E(lib.mpcx_covariance_workspace_bytes(S, K), torch.uint8)
    dtf = T((span[:, 1] - span[:, 0]) / units[:, 1])
    stage, dst2 = E((S, K - 1, _ffi.STAGE_DOUBLES)), E(S, torch.int32)
    print(f"covariance_thrust S {S} K {K} (J2, q = 1e-8, 2 % and 1 degree, mass variance 1e-4)", flush=True)
    med = measure({
        "mpcx_covariance_thrust_batch_dev": lambda: lib.mpcx_covariance_thrust_batch_dev(ctx, S, K, None, p(dY), p(dU), p(du), p(dsp), p(dc), _ffi.FLAG_J2,
                                                                                         1e-2, p(dP0), p(dq), p(dex), p(dmv), p(dP), p(dPm), p(dst),
                                                                                         p(ws), st),
        "mpcx_covariance_batch_dev": lambda: lib.mpcx_covariance_batch_dev(ctx, S, K, None, p(dY), p(dU), p(du), p(dsp), p(dc), _ffi.FLAG_J2, 1e-2,
                                                                           p(dP0), p(dq), p(dPc), p(dstc), p(wsc), st),
        "mpcx_discretize_stages_ragged_dev alone": lambda: lib.mpcx_discretize_stages_ragged_dev(ctx, S, K, None, K, None, p(dY), p(dU), p(dtf), p(dc),
                                                                                                 _ffi.FLAG_J2, 1e-2, p(stage), p(dst2), st)})
    a, b, c = med["mpcx_covariance_thrust_batch_dev"], med["mpcx_covariance_batch_dev"], med["mpcx_discretize_stages_ragged_dev alone"]
    print(f"    the 7 x 7 chain with execution errors (difference of the medians): {a - c:.3f} ms = {100.0 * (a - c) / a:.1f} % of the call; "
          f"the 6 x 6 chain: {b - c:.3f} ms", flush=True)
    Ph, Pc = dP.cpu().numpy(), dPc.cpu().numpy()
    assert int(dst.abs().sum()) == 0 and int(dstc.abs().sum()) == 0 and np.isfinite(Ph).all() and np.array_equal(Ph, np.transpose(Ph, (0, 1, 3, 2)))
    print(f"    position sigma at the last node: {np.sqrt(Ph[:, -1, 0, 0]).min():.0f} .. {np.sqrt(Ph[:, -1, 0, 0]).max():.0f} m with execution errors, "
          f"{np.sqrt(Pc[:, -1, 0, 0]).min():.0f} .. {np.sqrt(Pc[:, -1, 0, 0]).max():.0f} m without (100 m at the first)", flush=True)
    del dY, dP, dPc, ws, wsc, stage
    torch.cuda.empty_cache()
