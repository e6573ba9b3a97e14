"""profiling helper: durations of the covariance propagation and of the collision probability by HIP events on their stream.
  covariance: mpcx_covariance_batch_dev at S = 4096 satellites of a random LEO shell, K = 30 and K = 100 nodes over one orbit, J2 on,
      zero thrust, q = 1e-8; beside it mpcx_discretize_stages_ragged_dev alone on the same inputs (the call's first and largest step),
      the two alternating; the chain (tf kernel, memset, covariance_kernel) is the difference of the medians.
  collision probability: mpcx_collision_probability_dev for n = 1024 and n = 65 536 rows in the all-pairs form: random pairs (i < j)
      of 4096 satellites with 40 nodes and random covariances at random times inside the span (the objects need not be close: the
      kernel does the same work for every row whose status is 0, asserted).
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
S = 4096
for K in (30, 100):
    Y, units, span, consts = shell(S, K, seed=K)
    dY, du, dsp, dc = T(Y), T(units), T(span), T(consts)
    dP0, dq = T(np.broadcast_to(P0, (S, 6, 6))), T(np.full(S, 1e-8))
    dP, dst = E((S, K, 6, 6)), E(S, torch.int32)
    ws = E(lib.mpcx_covariance_workspace_bytes(S, K), torch.uint8)
    dtf, dU = T((span[:, 1] - span[:, 0]) / units[:, 1]), torch.zeros((S, 3, K), dtype=torch.float64, device=dev)
    stage, dst2 = E((S, K - 1, _ffi.STAGE_DOUBLES)), E(S, torch.int32)
    print(f"covariance S {S} K {K} (J2, q = 1e-8)", flush=True)
    med = measure({
        "mpcx_covariance_batch_dev": lambda: lib.mpcx_covariance_batch_dev(ctx, S, K, None, p(dY), None, p(du), p(dsp), p(dc), _ffi.FLAG_J2, 1e-2,
                                                                           p(dP0), p(dq), p(dP), p(dst), p(ws), st),
        "mpcx_discretize_stages_ragged_dev alone": lambda: lib.mpcx_discretize_stages_ragged_dev(ctx, S, K, None, K, None, p(dY), p(dU), p(dtf), p(dc),
                                                                                                 _ffi.FLAG_J2, 1e-2, p(stage), p(dst2), st)})
    a, b = med["mpcx_covariance_batch_dev"], med["mpcx_discretize_stages_ragged_dev alone"]
    print(f"    the chain (difference of the medians): {a - b:.3f} ms = {100.0 * (a - b) / a:.1f} % of the call", flush=True)
    Ph = dP.cpu().numpy()
    assert int(dst.abs().sum()) == 0 and np.isfinite(Ph).all() and np.array_equal(Ph, np.transpose(Ph, (0, 1, 3, 2)))
    print(f"    position sigma at the last node: {np.sqrt(Ph[:, -1, 0, 0]).min():.0f} .. {np.sqrt(Ph[:, -1, 0, 0]).max():.0f} m (100 m at the first)", flush=True)
    del dY, dP, ws, stage
    torch.cuda.empty_cache()

K = 40
Y, units, span, _ = shell(S, K, seed=7)
rng = np.random.default_rng(0)
D = np.concatenate([rng.uniform(100.0, 400.0, (S, 3)), rng.uniform(0.05, 0.3, (S, 3))], axis=1)
P = np.zeros((S, K, 6, 6)); P[:, :, np.arange(6), np.arange(6)] = (D * D)[:, None, :]
dY, du, dsp, dP, dr = T(Y), T(units), T(span), T(P), T(rng.uniform(1.0, 50.0, S))
for n in (1024, 65536):
    i = rng.integers(0, S - 1, n); j = rng.integers(i + 1, S)
    pairs = np.column_stack([i, j, np.zeros(n), rng.uniform(span[0, 0], span[0, 1], n)]).astype(np.float64)
    dpairs, out, pst = T(pairs), E((n, _ffi.NPC)), E(n, torch.int32)
    print(f"collision probability n {n} (all-pairs form, S {S}, K {K})", flush=True)
    measure({"mpcx_collision_probability_dev": lambda: lib.mpcx_collision_probability_dev(ctx, n, p(dpairs), S, K, None, p(dY), p(du), p(dsp), p(dP),
                                                                                          p(dr), 0, 0, None, None, None, None, None, None, R.MU_EARTH,
                                                                                          p(out), p(pst), st)})
    assert int(pst.abs().sum()) == 0 and bool(torch.isfinite(out).all())
