"""profiling helper: durations of "every close approach of listed pairs" (events_kernel, mpcx_conjunction_events_dev; threshold
5 km, max_events 16) beside the closest approach of the same list (pairs_kernel, mpcx_conjunction_pairs_dev, which this work
leaves as it was: the yardstick) by HIP events on their stream -- a random LEO shell of S = 4096 satellites on M = 541 common
instants (one orbit, 100 nodes per trajectory), n = 1024 and n = 65 536 random pairs.  Both calls are measured in the same visit in
alternating order: 3 warm-ups of each, then 20 rounds of (pairs, events); median, minimum and maximum of each and the ratio of
the medians are printed.  The events call is then run without a threshold and its smallest event per pair compared bit for bit
with the pairs call.  Counted work: pair-intervals = n x (M - 1) for both; the events call also stores n x E x 40 B."""
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
    run_pairs = lambda: lib.mpcx_conjunction_pairs_dev(ctx, n, p(pairs), S, 0, M, p(eph), None, T0, T1, p(out), p(stat), st)
    run_events = lambda thr=THR: lib.mpcx_conjunction_events_dev(ctx, n, p(pairs), S, 0, M, p(eph), None, T0, T1, thr, MAXEV, p(events), p(info),
                                                                 p(count), p(estat), st)
    for _ in range(WARM):
        timed(run_pairs); timed(run_events)
    ms_pairs, ms_events = [], []
    for _ in range(REPS):                                            # alternating: both see the same minutes of the machine
        ms_pairs.append(timed(run_pairs)); ms_events.append(timed(run_events))
    work = float(n) * (M - 1)
    mp = report(f"closest approach n {n} S {S} M {M}", ms_pairs, work)
    me = report(f"every approach <= 5 km, E 16, n {n}", ms_events, work)
    found = int(count.sum())
    print(f"    events / pairs {me / mp:.3f} (pairs' own max / min {max(ms_pairs) / min(ms_pairs):.3f}); {found} events <= 5 km, "
          f"outputs {n * MAXEV * 40 / 1e6:.2f} MB against {n * 36 / 1e6:.2f} MB", flush=True)
    assert int(stat.abs().sum()) == 0 and int(estat.abs().sum()) == 0
    assert run_events(0.0) == 0                                      # every event: the smallest of a pair is the pairs call's row
    torch.cuda.synchronize()
    ev, cnt, ref = events.cpu().numpy(), count.cpu().numpy(), out.cpu().numpy()
    assert (cnt >= 1).all() and (cnt <= MAXEV).all()
    d = np.where(np.arange(MAXEV)[None, :] < cnt[:, None], ev[:, :, 2], np.inf)
    best = ev[np.arange(n), np.argmin(d, axis=1)]
    same = best[:, 2:].tobytes() == ref[:, 2:].tobytes()
    print(f"    without a threshold: {int(cnt.sum())} events, {cnt.min()} .. {cnt.max()} per pair; the smallest of every pair has the pairs call's bits: {same}",
          flush=True)
    assert same
