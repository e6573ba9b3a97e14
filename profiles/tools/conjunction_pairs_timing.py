"""profiling helper: durations of the closest approach of LISTED pairs (pairs_kernel, mpcx_conjunction_pairs_dev) by HIP events
on its stream, a random LEO shell of S = 4096 satellites on M = 541 common instants (one orbit, 100 nodes per trajectory), at
n = 1024 and n = 65 536 random pairs, beside the all-pairs screen (mpcx_conjunction_screen_dev) of the same 4096 in the same
visit.  Every call is warmed up 3 times and timed 20 times; median, minimum and maximum are printed.  The screen's list of the
pairs below 5 km is then given to the list kernel and compared bit for bit.
Counted work: pair-intervals = n x (M - 1) for the list, S x (S - 1) x (M - 1) for the screen (the full square of ordered pairs)."""
import ctypes as C, os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conjunction_reference as R

S, M, NODES, WARM, REPS, THR = 4096, 541, 100, 3, 20, 5000.0

import torch
from mpconstellation_amd import _ffi
from mpconstellation_amd.conjunction import sort_pairs
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


def measure(name, fn, work):
    for _ in range(WARM):
        timed(fn)
    ms = [timed(fn) for _ in range(REPS)]
    med = statistics.median(ms)
    print(f"{name:44s} median {med:9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  ({len(ms)} runs)  {work / med / 1e6:8.1f} G pair-intervals/s", flush=True)
    return med


def list_call(pairs):
    n = pairs.shape[0]
    out, stat = E((n, 4)), E(n, torch.int32)
    return out, stat, lambda: lib.mpcx_conjunction_pairs_dev(ctx, n, p(pairs), S, 0, M, p(eph), None, T0, T1, p(out), p(stat), st)


rng = np.random.default_rng(7)
for n in (1024, 65536):
    i = rng.integers(0, S, n); j = (i + rng.integers(1, S, n)) % S
    pairs = T(np.column_stack([i, j, np.zeros(n), np.zeros(n)]).astype(np.float64))
    out, stat, run = list_call(pairs)
    measure(f"listed pairs n {n} S {S} M {M}", run, float(n) * (M - 1))
    assert int(stat.abs().sum()) == 0 and bool(torch.isfinite(out[:, 2:]).all())

dmin, tca, partner = E(S), E(S), E(S, torch.int32)
count = torch.zeros(1, dtype=torch.int64, device=dev)
ws = E(lib.mpcx_conjunction_workspace_bytes(S, M), torch.uint8)
screen = lambda maxp, lst: lib.mpcx_conjunction_screen_dev(ctx, S, M, p(eph), T0, T1, 0, S, THR, maxp, p(dmin), p(partner), p(tca), lst, p(count),
                                                           p(ws), st)
assert screen(0, None) == 0                                          # a counting call sizes the list
torch.cuda.synchronize()
maxp = max(int(count[0]), 1)
listed = torch.zeros((maxp, 4), dtype=torch.float64, device=dev)
measure(f"all-pairs screen S {S} M {M}", lambda: screen(maxp, p(listed)), float(S) * (S - 1) * (M - 1))
rows = sort_pairs(listed[:int(count[0])].cpu().numpy())
again = T(rows)
out, stat, run = list_call(again)
ms = timed(run)
same = out.cpu().numpy().tobytes() == rows.tobytes()
print(f"    the screen lists {len(rows)} pairs <= 5 km; the list kernel on that list: {ms:.3f} ms, the same bits: {same}", flush=True)
assert same and int(stat.abs().sum()) == 0
