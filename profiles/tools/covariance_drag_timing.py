"""profiling helper: durations of the covariance with an uncertain drag by HIP events on its stream.
  S = 4096 satellites (1 kg: drag 2e-4 of A under the fixed density) of a random LEO shell, K = 30 nodes over one orbit, drag and J2
  on, a thrust table of 0.02 standard_normal, q = 1e-8, execution errors of 2 % in magnitude and 1 degree in pointing with fixed parts
  of 1e-4, a mass variance of 1e-4, a density error of 20 % with a correlation time of one hour.  Four calls on the same inputs,
  alternating in one process, ROUNDS times over:
    mpcx_covariance_drag_batch_dev            the whole call
    mpcx_covariance_thrust_batch_dev          the call it extends (same flags)
    mpcx_discretize_stages_ragged_dev, MPCX_FLAG_DRAG_COLUMN   the first call's linearisation alone
    mpcx_discretize_stages_ragged_dev, plain DRAG              the second call's linearisation alone
  the chains are the differences of the medians (whole call minus its linearisation).
Every call is warmed up WARM times and timed REPS times per round; median, minimum and maximum of a round are printed, and the spread
of the rounds' medians at the end."""
import ctypes as C, os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conjunction_reference as R

WARM, REPS, ROUNDS = 3, 20, 3

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
S, K = 4096, 30
FLAGS = _ffi.FLAG_DRAG | _ffi.FLAG_J2
Y, units, span, consts = shell(S, K, seed=K)
U = 0.02 * np.random.default_rng(K).standard_normal((S, 3, K))
dY, dU, du, dsp, dc = T(Y), T(U), T(units), T(span), T(consts)
dP0, dq = T(np.broadcast_to(P0, (S, 6, 6))), T(np.full(S, 1e-8))
dex, dmv, ddn = T(np.broadcast_to(EXEC, (S, 5))), T(np.full(S, 1e-4)), T(np.broadcast_to([0.2, 3600.0], (S, 2)))
dP, dPm, dPb, dPt, dPmt = E((S, K, 6, 6)), E((S, K, 7)), E((S, K, 8)), E((S, K, 6, 6)), E((S, K, 7))
dst, dstt, dst2, dst3 = (E(S, torch.int32) for _ in range(4))
ws = E(lib.mpcx_covariance_drag_workspace_bytes(S, K), torch.uint8)
wst = E(lib.mpcx_covariance_thrust_workspace_bytes(S, K), torch.uint8)
dtf = T((span[:, 1] - span[:, 0]) / units[:, 1])
stage, stage2 = E((S, K - 1, _ffi.STAGE_DOUBLES)), E((S, K - 1, _ffi.STAGE_DOUBLES))
runs = {
    "mpcx_covariance_drag_batch_dev": lambda: lib.mpcx_covariance_drag_batch_dev(ctx, S, K, None, p(dY), p(dU), p(du), p(dsp), p(dc), FLAGS, 1e-2, p(dP0), p(dq),
                                                                                 p(dex), p(dmv), p(ddn), p(dP), p(dPm), p(dPb), p(dst), p(ws), st),
    "mpcx_covariance_thrust_batch_dev": lambda: lib.mpcx_covariance_thrust_batch_dev(ctx, S, K, None, p(dY), p(dU), p(du), p(dsp), p(dc), FLAGS, 1e-2, p(dP0),
                                                                                     p(dq), p(dex), p(dmv), p(dPt), p(dPmt), p(dstt), p(wst), st),
    "mpcx_discretize_stages_ragged_dev, DRAG_COLUMN": lambda: lib.mpcx_discretize_stages_ragged_dev(ctx, S, K, None, K, None, p(dY), p(dU), p(dtf), p(dc),
                                                                                                    FLAGS | _ffi.FLAG_DRAG_COLUMN, 1e-2, p(stage), p(dst2), st),
    "mpcx_discretize_stages_ragged_dev, plain DRAG": lambda: lib.mpcx_discretize_stages_ragged_dev(ctx, S, K, None, K, None, p(dY), p(dU), p(dtf), p(dc),
                                                                                                   FLAGS, 1e-2, p(stage2), p(dst3), st)}
print(f"covariance_drag S {S} K {K} (drag, J2, q = 1e-8, 2 % and 1 degree, mass variance 1e-4, density 20 % over one hour)", flush=True)
rounds = []
for r in range(ROUNDS):
    print(f"  round {r + 1}", flush=True)
    rounds.append(measure(runs))
names = list(runs)
print("  medians of the rounds (ms):", flush=True)
for k in names:
    v = [m[k] for m in rounds]
    print(f"    {k:58s} {'  '.join(f'{x:7.3f}' for x in v)}   spread {max(v) - min(v):.3f}", flush=True)
a, b, c, d = (statistics.median([m[k] for m in rounds]) for k in names)
print(f"    linearisation, column form - plain DRAG form: {c - d:+.3f} ms; the 8 x 8 chain (whole call - its linearisation): {a - c:.3f} ms = "
      f"{100.0 * (a - c) / a:.1f} % of the call; the 7 x 7 chain: {b - d:.3f} ms; whole call drag - thrust: {a - b:+.3f} ms", flush=True)
Ph, Pt, rec, rec2 = dP.cpu().numpy(), dPt.cpu().numpy(), stage.cpu().numpy(), stage2.cpu().numpy()
assert int(dst.abs().sum()) == 0 and int(dstt.abs().sum()) == 0 and int(dst2.abs().sum()) == 0 and int(dst3.abs().sum()) == 0
assert np.isfinite(Ph).all() and np.array_equal(Ph, np.transpose(Ph, (0, 1, 3, 2)))
assert rec[:, :, :91].tobytes() == rec2[:, :, :91].tobytes() and rec[:, :, 98:].tobytes() == rec2[:, :, 98:].tobytes()
print(f"    the two linearisations: A, B_kn, B_kp, xi equal to the bit; position sigma at the last node: {np.sqrt(Ph[:, -1, 0, 0]).min():.0f} .. "
      f"{np.sqrt(Ph[:, -1, 0, 0]).max():.0f} m with the density error, {np.sqrt(Pt[:, -1, 0, 0]).min():.0f} .. {np.sqrt(Pt[:, -1, 0, 0]).max():.0f} m without "
      f"(100 m at the first)", flush=True)
