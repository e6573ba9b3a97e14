"""profiling helper: durations of ephemeris_kernel and of the conjunction screen (transpose + screen_kernel<256, 32, SELF> + reduce) by HIP
events on their stream, S = 512 and 4096 satellites of a random LEO shell on M = 541 common instants (one orbit, 100 nodes per
trajectory), and the fp64 rate they amount to.  --share: the share of valid pair-intervals that take the Newton steps, counted
by the numpy restatement (host only, S = 512; minutes of numpy at 4096).
Operation count behind the rate (an FMA as two): 32 per valid pair-interval (two differences, four dot products, the chord, one
division) + 400 per interval that takes the Newton steps (three steps of three Hermite evaluations and three dot products, the
final evaluation); the full square is computed, so every pair counts twice."""
import ctypes as C, os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conjunction_reference as R

M, NODES = 541, 100
PEAK = 78.6e12


def inputs(S):
    orb = R.random_orbits(S, seed=S)
    T1 = 2 * np.pi / R.orbit_rate(orb).max()
    Y, units, span = R.trajectories(orb, NODES, (-1.0, T1 + 1.0))
    return Y, units, span, 0.0, T1


if "--share" in sys.argv:
    Y, units, span, T0, T1 = inputs(512)
    eph, _ = R.ephemeris(Y, units, span, M, T0, T1)
    *_, stats = R.pair_minima(eph, T0, T1)
    print(f"S 512 M {M}: {stats['newton']} of {stats['valid']} pair-intervals take the Newton steps: {stats['newton'] / stats['valid']:.4f}")
    sys.exit(0)

import torch
from mpconstellation_amd import _ffi
lib = _ffi.load(); ctx = _ffi.context(0)
dev = torch.device("cuda", 0)
p = lambda t: C.c_void_p(t.data_ptr())
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
share = float(os.environ.get("NEWTON_SHARE", "nan"))
for S in (512, 4096):
    Y, units, span, T0, T1 = inputs(S)
    T = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=dev)
    dY, du, dsp = T(Y), T(units), T(span)
    eph = torch.empty((S, 6, M), dtype=torch.float64, device=dev); status = torch.empty(S, dtype=torch.int32, device=dev)
    dmin = torch.empty(S, dtype=torch.float64, device=dev); tca = torch.empty_like(dmin); partner = torch.empty(S, dtype=torch.int32, device=dev)
    pairs = torch.zeros((1024, 4), dtype=torch.float64, device=dev); npairs = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(lib.mpcx_conjunction_workspace_bytes(S, M), dtype=torch.uint8, device=dev)

    def timed(fn, reps=4):
        ms = []
        for _ in range(reps):
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True); e0.record()
            assert fn() == 0
            e1.record(); torch.cuda.synchronize(); ms.append(e0.elapsed_time(e1))
        return ms
    t_eph = timed(lambda: lib.mpcx_ephemeris_batch_dev(ctx, S, NODES, None, p(dY), p(du), p(dsp), M, T0, T1, p(eph), p(status), st))
    t_scr = timed(lambda: lib.mpcx_conjunction_screen_dev(ctx, S, M, p(eph), T0, T1, 0, S, 5000.0, 1024, p(dmin), p(partner), p(tca), p(pairs),
                                                          p(npairs), p(ws), st))
    n_int = float(S) * (S - 1) * (M - 1)
    flops = n_int * (32.0 + (400.0 * share if share == share else 0.0))
    t = min(t_scr) * 1e-3
    print(f"S {S:5d} M {M}: ephemeris {min(t_eph):8.3f} ms (all {['%.3f' % x for x in t_eph]})  screen {min(t_scr):9.3f} ms (all {['%.3f' % x for x in t_scr]})  "
          f"{n_int / t / 1e9:8.1f} G pair-intervals/s  ~{flops / t / 1e12:6.2f} TF fp64 = {100 * flops / t / PEAK:5.1f} % of the 78.6 TF vector peak "
          f"(Newton share {share})  dmin min {float(dmin.min()):.1f} m, pairs <= 5 km: {int(npairs[0])}", flush=True)
