"""profiling helper: durations of "the close approach nearest each row's own time" (track_kernel, mpcx_conjunction_track_dev, no
max_shift, info asked for) beside the closest approach (pairs_kernel, mpcx_conjunction_pairs_dev) and every close approach
(events_kernel, mpcx_conjunction_events_dev; threshold 5 km, max_events 16) of the same list, by HIP events on their stream -- the
shapes of conjunction_events_timing.py: a random LEO shell of S = 4096 satellites on M = 541 common instants (one orbit, 100 nodes
per trajectory), n = 1024 and n = 65 536 random pairs.  The rows' times are the pairs call's (every row follows its pair's closest
approach), so the tracked rows must come back with the pairs call's bits, which is checked.  All three calls are measured in the
same visit in alternating order: 3 warm-ups of each, then 20 rounds of (pairs, events, track); median, minimum and maximum of each
and the ratios of the medians are printed.  Counted work: pair-intervals = n x (M - 1) for all three."""
import ctypes as C, os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conjunction_reference as R

S, M, NODES, WARM, REPS, THR, MAXEV = 4096, 541, 100, 3, 20, 5000.0, 16

import torch
from mpconstellation_amd import _ffi
lib = _ffi.load(); ctx = _ffi.context(0)
dev = torch.device("cuda", 0)
p = lambda t: C.c_void_p(t.data_ptr())
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
T = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=dev)
E = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)

orb = R.random_orbits(S, seed=S)
T0, T1 = 0.0, 2 * np.pi / np.sqrt(R.MU_EARTH / 6.9e6 ** 3)           # one orbit at the shell's floor
Y, units, span = R.trajectories(orb, NODES, (-1.0, T1 + 1.0))
eph, status = E((S, 6, M)), E(S, torch.int32)
dY, du, dsp = T(Y), T(units), T(span)
assert lib.mpcx_ephemeris_batch_dev(ctx, S, NODES, None, p(dY), p(du), p(dsp), M, T0, T1, p(eph), p(status), st) == 0
torch.cuda.synchronize()
assert int(status.abs().sum()) == 0


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    assert fn() == 0
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def report(name, ms, work):
    med = statistics.median(ms)
    print(f"{name:44s} median {med:9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  ({len(ms)} runs)  {work / med / 1e6:8.1f} G pair-intervals/s", flush=True)
    return med


rng = np.random.default_rng(7)
for n in (1024, 65536):
    i = rng.integers(0, S, n); j = (i + rng.integers(1, S, n)) % S
    pairs = T(np.column_stack([i, j, np.zeros(n), np.zeros(n)]).astype(np.float64))
    out, stat = E((n, 4)), E(n, torch.int32)
    events, info, count, estat = E((n, MAXEV, 4)), E((n, MAXEV, 2), torch.int32), E(n, torch.int32), E(n, torch.int32)
    tout, tinfo, tstat = E((n, 4)), E((n, 2), torch.int32), E(n, torch.int32)
    run_pairs = lambda: lib.mpcx_conjunction_pairs_dev(ctx, n, p(pairs), S, 0, M, p(eph), None, T0, T1, p(out), p(stat), st)
    run_events = lambda: lib.mpcx_conjunction_events_dev(ctx, n, p(pairs), S, 0, M, p(eph), None, T0, T1, THR, MAXEV, p(events), p(info), p(count),
                                                         p(estat), st)
    run_track = lambda: lib.mpcx_conjunction_track_dev(ctx, n, p(out), S, 0, M, p(eph), None, T0, T1, 0.0, p(tout), p(tinfo), p(tstat), st)
    for _ in range(WARM):
        timed(run_pairs); timed(run_events); timed(run_track)
    ms_pairs, ms_events, ms_track = [], [], []
    for _ in range(REPS):                                            # alternating: all three see the same minutes of the machine
        ms_pairs.append(timed(run_pairs)); ms_events.append(timed(run_events)); ms_track.append(timed(run_track))
    work = float(n) * (M - 1)
    mp = report(f"closest approach n {n} S {S} M {M}", ms_pairs, work)
    me = report(f"every approach <= 5 km, E 16, n {n}", ms_events, work)
    mt = report(f"nearest the row's time, n {n}", ms_track, work)
    same = tout.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
    print(f"    track / pairs {mt / mp:.3f}, track / events {mt / me:.3f} (pairs' own max / min {max(ms_pairs) / min(ms_pairs):.3f}); "
          f"the tracked rows have the pairs call's bits: {same}", flush=True)
    assert int(stat.abs().sum()) == 0 and int(tstat.abs().sum()) == 0 and same and int((tinfo[:, 0] < 0).sum()) == 0
