"""profiling helper: duration of the iterated avoidance by HIP events on its stream, per round.
  mpcx_avoidance_refine_dev in the all-pairs form on avoidance_joint_timing.py's plan (S = 4096 thrusting satellites of a random LEO
  shell, K = 30 nodes over one orbit, n = 1024 random pairs i < j at random times, object i moving, no rows / tsens / rhs), the target
  at the list's 10th percentile of d0 so that a tenth of the rows is violated, hold, no ball, with rounds = 0, 1 and 3: a round (flight,
  re-screen on M = 4 (K - 1) + 1 instants, linearisation, rows, solve, glue) is (rounds 3 - rounds 1) / 2, the closing flight and
  re-screen rounds 0 less mpcx_avoidance_joint_dev.  Beside it the same round composed from the public host-pointer calls:
  AvoidanceJointResult.apply -> propagate_batch -> screen_pairs -> avoidance_joint (wall clock: they copy in and out and wait).
Every shape is warmed up WARM times and timed REPS times in one process; median, minimum and maximum are printed."""
import ctypes as C, os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conjunction_reference as R

WARM, REPS = 3, 20

import torch
from mpconstellation_amd import _ffi, avoidance_joint, propagate_batch, screen_pairs
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def measure(runs, clock):
    for _ in range(WARM):
        for fn in runs.values():
            clock(fn)
    ms = {k: [] for k in runs}
    for _ in range(REPS):
        for k, fn in runs.items():
            ms[k].append(clock(fn))
    for k, v in ms.items():
        print(f"    {k:52s} median {statistics.median(v):8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  ({len(v)} runs)", flush=True)
    return {k: statistics.median(v) for k, v in ms.items()}


def histogram(x):
    v, c = np.unique(x, return_counts=True)
    return ", ".join(f"{int(a)}: {int(b)}" for a, b in zip(v, c))


S, K, n = 4096, 30, 1024
M = 4 * (K - 1) + 1
rng = np.random.default_rng(0)
orb = R.random_orbits(S, seed=K)
T1 = 2 * np.pi / np.sqrt(R.MU_EARTH / 6.9e6 ** 3)
Y, units, span = R.trajectories(orb, K, (0.0, T1))
state = np.zeros((S, 7)); state[:, 0] = units[:, 0]; state[:, 6] = 1.0
consts = normalize_batch(state)[1]
U = 0.01 * rng.standard_normal((S, 3, K))
i = rng.integers(0, S - 1, n); j = rng.integers(i + 1, S)
pairs = np.column_stack([i, j, np.zeros(n), rng.uniform(0.05 * T1, T1, n)]).astype(np.float64)
model = dict(include_J2=True)
first = avoidance_joint(pairs, 1.0, Y, U, units, span, consts, **model)
target = float(np.percentile(first.d0[first.row_status == 0], 10.0))
print(f"avoidance_refine n {n} (all-pairs form, S {S}, K {K}, M {M}, J2, hold, no ball, target {target:.4e} m: the 10th percentile of d0)", flush=True)

dY, dU, du_, dsp, dc, dpairs = T(Y), T(U), T(units), T(span), T(consts), T(pairs)
jdu, jso, jro, jss, jrs = E((S, 3, K)), E((S, _ffi.NAJ)), E((n, _ffi.NAR)), E(S, torch.int32), E(n, torch.int32)
Yo, po, rd = E((S, 7, K)), E((n, 4)), E(S, torch.int32)
h0, h1, h2 = E((5, n)), E((5, n)), E((5, S))
ws = E(lib.mpcx_avoidance_refine_workspace_bytes(n, S, K, 0, M), torch.uint8)


def refine(rounds):
    return lambda: lib.mpcx_avoidance_refine_dev(ctx, n, p(dpairs), None, S, K, None, p(dY), p(dU), p(du_), p(dsp), p(dc), _ffi.FLAG_J2, 1e-2, None, 0, 0,
                                                 None, None, None, None, None, R.MU_EARTH, target, None, 1, _ffi.AJ_DEFAULT_TOL, _ffi.AJ_DEFAULT_MAX_ITER,
                                                 M, 0.0, float(T1), 1e-3, rounds, p(jdu), p(jso), p(jro), None, None, p(jss), p(jrs), p(Yo), p(po), p(h0),
                                                 p(h1), p(h2), p(rd), None, None, p(ws), st)


def joint():
    return lib.mpcx_avoidance_joint_dev(ctx, n, p(dpairs), None, S, K, None, p(dY), p(dU), p(du_), p(dsp), p(dc), _ffi.FLAG_J2, 1e-2, None, 0, 0, None, None,
                                        None, None, None, R.MU_EARTH, target, None, 1, _ffi.AJ_DEFAULT_TOL, _ffi.AJ_DEFAULT_MAX_ITER, 0, S, p(jdu), p(jso),
                                        p(jro), None, None, p(jss), p(jrs), p(ws), st)


assert refine(3)() == 0
torch.cuda.synchronize()
ss, so, done, d0 = jss.cpu().numpy(), jso.cpu().numpy(), rd.cpu().numpy(), h0.cpu().numpy()
short = np.maximum(target - d0, 0.0) / target
print(f"    rounds 3: satellite statuses {{{histogram(ss)}}}, rounds_done {{{histogram(done)}}}, iterations of the last accepted solve "
      f"{{{histogram(so[(ss == 0) & (so[:, _ffi.AJ_ROWS] > 0), _ffi.AJ_ITERS])}}}; rows short of the target by pass {(short > 0).sum(axis=1).tolist()}, "
      f"worst shortfall by pass {np.nanmax(short, axis=1)}", flush=True)
med = measure({"mpcx_avoidance_joint_dev": joint, "mpcx_avoidance_refine_dev, rounds 0": refine(0), "mpcx_avoidance_refine_dev, rounds 1": refine(1),
               "mpcx_avoidance_refine_dev, rounds 3": refine(3)}, timed)
print(f"    a round (rounds 3 less rounds 1, halved): {(med['mpcx_avoidance_refine_dev, rounds 3'] - med['mpcx_avoidance_refine_dev, rounds 1']) / 2:.3f} ms; "
      f"the closing flight, re-screen and rows (rounds 0 less the joint call): {med['mpcx_avoidance_refine_dev, rounds 0'] - med['mpcx_avoidance_joint_dev']:.3f} ms",
      flush=True)

# the same round from the public calls (host pointers in, results out, every call waits)
res = avoidance_joint(pairs, target, Y, U, units, span, consts, **model)
flies = (res.status == 0) & (res.n_rows > 0)
tf = (span[:, 1] - span[:, 0]) / units[:, 1]
state_ = {}


def composed():
    Ut = np.where(flies[:, None, None], U + np.where(flies[:, None, None], res.du, 0.0), U)
    y, pst, _ = propagate_batch(np.ascontiguousarray(Y[:, :, 0]), tf, consts, (_ffi.CTRL_SEQUENCE, Ut, K, 1.0), K, include_J2=True, max_step=1e-3)
    Yt = np.where((flies & (pst == 0))[:, None, None], y, Y)
    again = screen_pairs(pairs, 0.0, float(T1), Y=Yt, units=units, span=span, M=M)[0]
    state_["next"] = avoidance_joint(again, target, Yt, Ut, units, span, consts, **model)


measure({"apply -> propagate_batch -> screen_pairs -> avoidance_joint": composed}, wall)
