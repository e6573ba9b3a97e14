"""profiling helper: duration of the encounter window by HIP events on its stream.
  mpcx_encounter_window_dev for n = 1024 and n = 65 536 rows, max_half 400 s, nsigma 8, levels 1 and 3, in the all-pairs form, on 6144
  objects with 40 nodes and random full 6 x 6 covariances, three lists that take the three paths of the search:
    random pairs (i < j)   far apart: clear, one node evaluation per lane;
    slow neighbours        2048 orbits and the same orbits 70 m higher (0.075 m/s): open on both sides, 1 + 2 evaluations;
    crossings              2048 orbits and one object each that crosses it at the row's time at 0.5 .. 2.6 rad (km/s): both sides
                           close, 1 + 2 levels evaluations.
  Every status is 0, asserted; the flags' census is printed.
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


H0, K, MAX_HALF = 2048, 40, 400.0
S = 3 * H0
orb = R.random_orbits(H0, seed=7)
T1 = 2 * np.pi / np.sqrt(R.MU_EARTH / 6.9e6 ** 3)
Y, units, span = R.trajectories(orb, K, (0.0, T1))
rng = np.random.default_rng(0)
# the third block: object 2 H0 + k crosses orbit k at tc[k] at the same radius, its plane turned by 0.5 .. 2.6 rad about the position
tc = rng.uniform(MAX_HALF + 100.0, T1 - MAX_HALF - 100.0, H0)
pk, vk = R.kepler_state(orb, tc)
cross = []
for k in range(H0):
    u = pk[k] / np.linalg.norm(pk[k]); vh = vk[k] / np.linalg.norm(vk[k]); ang = rng.uniform(0.5, 2.6)
    cross.append(CR.circular_through(pk[k], np.cos(ang) * vh + np.sin(ang) * np.cross(u, vh), tc[k], K, (0.0, T1)))
# the second block: the first again, every length unit larger by 1e-5 (70 m higher, 0.075 m/s faster: a slow neighbour)
Y = np.concatenate([Y, Y, np.stack([c[0] for c in cross])])
units = np.concatenate([units, units * np.array([1.0 + 1e-5, 1.0]), np.stack([c[1] for c in cross])])
span = np.concatenate([span, span, span])
P = np.concatenate([CR.random_covariances(rng, 256, K)] * (S // 256))
dY, du, dsp, dP, dr = T(Y), T(units), T(span), T(P), T(rng.uniform(1.0, 50.0, S))
for n in (1024, 65536):
    t = rng.uniform(span[0, 0] + 100.0, span[0, 1] - 100.0, n)
    i = rng.integers(0, 2 * H0 - 1, n); j = rng.integers(i + 1, 2 * H0)
    k = rng.integers(0, H0, n)
    lists = {"random pairs (far apart: clear)": np.column_stack([i, j, np.zeros(n), t]),
             "slow neighbours (70 m, 0.075 m/s: open)": np.column_stack([k, k + H0, np.zeros(n), t]),
             "crossings (km/s: both sides close)": np.column_stack([k, k + 2 * H0, np.zeros(n), tc[k]])}
    for what, pairs in lists.items():
        dpairs, dmax, out, fl, pst = T(pairs.astype(np.float64)), T(np.full(n, MAX_HALF)), E((n, _ffi.NEW)), E(n, torch.int32), E(n, torch.int32)
        for levels in (1, 3):
            print(f"encounter window n {n} levels {levels}, {what} (all-pairs form, S {S}, K {K}, max_half {MAX_HALF:.0f} s, nsigma 8)", flush=True)
            med = measure("mpcx_encounter_window_dev",
                          lambda: lib.mpcx_encounter_window_dev(ctx, n, p(dpairs), S, K, None, p(dY), p(du), p(dsp), p(dP), p(dr), 0, 0, None, None,
                                                                None, None, None, None, R.MU_EARTH, p(dmax), 8.0, levels, p(out), p(fl), p(pst), st))
            print(f"    {1e6 * med / n:.1f} ns per row; flags census (0 .. 15) {torch.bincount(fl, minlength=16).tolist()}; "
                  f"half {float(out[:, _ffi.EW_HALF].min()):.4f} .. {float(out[:, _ffi.EW_HALF].max()):.4f} s", flush=True)
            assert int(pst.abs().sum()) == 0 and bool(torch.isfinite(out).all())
