"""profiling helper: wall time of two host-pointer forms of the listed-pair family, staging included -- the calls end in a stream
synchronisation, so a host clock around them measures the whole call.
  mpcx_collision_probability   n = 1024 rows in the all-pairs form on collision_timing.py's scene (S = 4096, K = 40, random covariances)
  mpcx_avoidance_joint         n = 1024 rows on avoidance_joint_timing.py's scene (S = 4096, K = 30, J2, target 1e9 m, no hold, no ball,
                               without rows / tsens)
One library per process: name another build in MPCX_LIB and run the two alternately to compare them.  Every call is warmed up WARM
times and timed REPS times; median, minimum and maximum are printed."""
import os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conjunction_reference as R

WARM, REPS = 5, 200

from mpconstellation_amd import _ffi
from mpconstellation_amd.constellation import normalize_batch
lib = _ffi.load(); ctx = _ffi.context(0)
d, i32 = _ffi.dptr, _ffi.iptr
print(f"library {_ffi.LIB_PATH}", flush=True)


def measure(name, fn):
    for _ in range(WARM):
        assert fn() == 0, lib.mpcx_last_error(ctx)
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        rc = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
        assert rc == 0
    print(f"    {name:30s} median {statistics.median(ms):8.3f} ms  min {min(ms):8.3f}  max {max(ms):8.3f}  ({len(ms)} runs)", flush=True)


def shell(S, K, seed):
    orb = R.random_orbits(S, seed=seed)
    T1 = 2 * np.pi / np.sqrt(R.MU_EARTH / 6.9e6 ** 3)
    Y, units, span = R.trajectories(orb, K, (0.0, T1))
    state = np.zeros((S, 7)); state[:, 0] = units[:, 0]; state[:, 6] = 1.0
    return Y, units, span, normalize_batch(state)[1], T1


S, n = 4096, 1024
rng = np.random.default_rng(0)
i = rng.integers(0, S - 1, n); j = rng.integers(i + 1, S)

K = 40
Y, units, span, _, T1 = shell(S, K, seed=7)
D = np.concatenate([rng.uniform(100.0, 400.0, (S, 3)), rng.uniform(0.05, 0.3, (S, 3))], axis=1)
P = np.zeros((S, K, 6, 6)); P[:, :, np.arange(6), np.arange(6)] = (D * D)[:, None, :]
radius = rng.uniform(1.0, 50.0, S)
pairs = np.column_stack([i, j, np.zeros(n), rng.uniform(span[0, 0], span[0, 1], n)]).astype(np.float64)
out, pst = np.empty((n, _ffi.NPC)), np.empty(n, dtype=np.int32)
print(f"n {n}, S {S}: host-pointer forms, wall time", flush=True)
measure("mpcx_collision_probability", lambda: lib.mpcx_collision_probability(ctx, n, d(pairs), S, K, None, d(Y), d(units), d(span), d(P), d(radius), 0, 0,
                                                                             None, None, None, None, None, None, R.MU_EARTH, d(out), i32(pst)))
assert not pst.any() and np.isfinite(out).all()

K = 30
Y, units, span, consts, T1 = shell(S, K, seed=K)
U = 0.01 * rng.standard_normal((S, 3, K))
pairs = np.column_stack([i, j, np.zeros(n), rng.uniform(0.05 * T1, T1, n)]).astype(np.float64)
du, so, ro = np.empty((S, 3, K)), np.empty((S, _ffi.NAJ)), np.empty((n, _ffi.NAR))
ss, rs = np.empty(S, dtype=np.int32), np.empty(n, dtype=np.int32)
measure("mpcx_avoidance_joint", lambda: lib.mpcx_avoidance_joint(ctx, n, d(pairs), None, S, K, None, d(Y), d(U), d(units), d(span), d(consts), _ffi.FLAG_J2,
                                                                 1e-2, None, 0, 0, None, None, None, None, None, R.MU_EARTH, 1.0e9, None, 0,
                                                                 _ffi.AJ_DEFAULT_TOL, _ffi.AJ_DEFAULT_MAX_ITER, 0, S, d(du), d(so), d(ro), None, None,
                                                                 i32(ss), i32(rs)))
v, c = np.unique(ss, return_counts=True)
print(f"    satellite statuses {dict(zip(v.tolist(), c.tolist()))}", flush=True)
