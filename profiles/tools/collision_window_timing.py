"""profiling helper: duration of the window collision probability by HIP events on its stream.
  mpcx_collision_probability_window_dev for n = 1024 and n = 65 536 rows at panels = 1 and 4, in the all-pairs form, on 4096 objects
  with 40 nodes and random full 6 x 6 covariances at random times inside the span, half window 60 s, two lists: random pairs (i < j)
  -- far apart, the density underflows, the loops are the same -- and slow neighbours (2048 orbits and the same orbits 70 m higher:
  0.075 m/s), where every term of the sums counts.  Every status is 0, asserted.
Every shape is warmed up WARM times and timed REPS times in one process; median, minimum and maximum are printed."""
import ctypes as C, os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conjunction_reference as R
import collision_reference as CR

WARM, REPS = 3, 20

import torch
from mpconstellation_amd import _ffi
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


def measure(name, fn):
    for _ in range(WARM):
        timed(fn)
    v = [timed(fn) for _ in range(REPS)]
    print(f"    {name:44s} median {statistics.median(v):9.3f} ms  min {min(v):9.3f}  max {max(v):9.3f}  ({len(v)} runs)", flush=True)
    return statistics.median(v)


S, K = 4096, 40
orb = R.random_orbits(S // 2, seed=7)
T1 = 2 * np.pi / np.sqrt(R.MU_EARTH / 6.9e6 ** 3)
Y, units, span = R.trajectories(orb, K, (0.0, T1))
# the second half: the first half again, every length unit larger by 1e-5 (70 m higher, 0.075 m/s faster: a slow neighbour)
Y, units, span = np.concatenate([Y, Y]), np.concatenate([units, units * np.array([1.0 + 1e-5, 1.0])]), np.concatenate([span, span])
rng = np.random.default_rng(0)
P = np.concatenate([CR.random_covariances(rng, 256, K)] * (S // 256))
dY, du, dsp, dP, dr = T(Y), T(units), T(span), T(P), T(rng.uniform(1.0, 50.0, S))
for n in (1024, 65536):
    t = rng.uniform(span[0, 0] + 100.0, span[0, 1] - 100.0, n)
    i = rng.integers(0, S - 1, n); j = rng.integers(i + 1, S)
    k = rng.integers(0, S // 2, n)
    lists = {"random pairs (far apart: the density underflows)": np.column_stack([i, j, np.zeros(n), t]),
             "slow neighbours (70 m, 0.075 m/s: every term counts)": np.column_stack([k, k + S // 2, np.zeros(n), t])}
    for what, pairs in lists.items():
        dpairs, dhalf, out, pst = T(pairs.astype(np.float64)), T(np.full(n, 60.0)), E((n, _ffi.NPW)), E(n, torch.int32)
        for panels in (1, 4):
            print(f"window collision probability n {n} panels {panels}, {what} (all-pairs form, S {S}, K {K}, half window 60 s)", flush=True)
            med = measure("mpcx_collision_probability_window_dev",
                          lambda: lib.mpcx_collision_probability_window_dev(ctx, n, p(dpairs), S, K, None, p(dY), p(du), p(dsp), p(dP), p(dr), 0, 0,
                                                                            None, None, None, None, None, None, R.MU_EARTH, p(dhalf), panels, p(out),
                                                                            p(pst), st))
            print(f"    {1e6 * med / n:.1f} ns per row, {1e6 * med / (n * panels * 64 * 512):.4f} ns per sphere point; "
                  f"p {float(out[:, 0].min()):.3e} .. {float(out[:, 0].max()):.3e}", flush=True)
            assert int(pst.abs().sum()) == 0 and bool(torch.isfinite(out).all())
