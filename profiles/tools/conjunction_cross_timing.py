"""profiling helper: durations of the cross screen (two transposes + screen_kernel + reduce, mpcx_conjunction_cross_screen_dev)
by HIP events on its stream, a random LEO shell on M = 541 common instants (one orbit, 100 nodes per trajectory), at
(S satellites, D catalogue objects) = (512, 4096), (64, 32768), (4096, 4096); and, at (512, 4096), of the only other way to the
same answer: the all-pairs screen (mpcx_conjunction_screen_dev) of the union of 4608 objects, the two alternating on one device.
Every list is sized by a counting call (max_pairs = 0) first, so that none is cut off; then every shape is warmed up twice and
timed REPS times; median, minimum and maximum are printed.  At (512, 4096) the pairs below
5 km of the two ways are compared bit for bit (the union's rows with i < S <= j, rewritten as (i, j - S)).
Counted work: pair-intervals = rows x columns x (M - 1); the union computes the full square of 4608."""
import ctypes as C, os, statistics, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import conjunction_reference as R

M, NODES, REPS, THR = 541, 100, 7, 5000.0

import torch
from mpconstellation_amd import _ffi
from mpconstellation_amd.conjunction import sort_pairs
lib = _ffi.load(); ctx = _ffi.context(0)
dev = torch.device("cuda", 0)
p = lambda t: C.c_void_p(t.data_ptr())
st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
T = lambda a, dt=torch.float64: torch.tensor(a, dtype=dt, device=dev)
E = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=dev)


def ephemeris(N, seed):
    """N objects of the shell on the grid, made on the device: eph (N, 6, M), T0, T1"""
    orb = R.random_orbits(N, seed=seed)
    T1 = 2 * np.pi / np.sqrt(R.MU_EARTH / 6.9e6 ** 3)              # one orbit at the shell's floor: the same grid for everybody
    Y, units, span = R.trajectories(orb, NODES, (-1.0, T1 + 1.0))
    eph, status = E((N, 6, M)), E(N, torch.int32)
    dY, du, dsp = T(Y), T(units), T(span)                           # named: they must outlive the call that reads them
    assert lib.mpcx_ephemeris_batch_dev(ctx, N, NODES, None, p(dY), p(du), p(dsp), M, 0.0, T1, p(eph), p(status), st) == 0
    torch.cuda.synchronize()
    assert int(status.abs().sum()) == 0
    radius = eph[:, 0:3, :].norm(dim=1)
    assert float(radius.min()) > 6.89e6 and float(radius.max()) < 7.31e6   # the shell, not whatever the memory held
    return eph, 0.0, T1


class Outputs:
    """results of one screen; call(max_pairs, *outputs) is the screen.  The list gets the room a counting call asks for."""
    def __init__(self, rows, call):
        self.dmin, self.tca, self.partner = E(rows), E(rows), E(rows, torch.int32)
        self.n = torch.zeros(1, dtype=torch.int64, device=dev)
        assert call(0, p(self.dmin), p(self.partner), p(self.tca), None, p(self.n)) == 0
        torch.cuda.synchronize()
        self.maxp = max(int(self.n[0]), 1)
        self.pairs = torch.zeros((self.maxp, 4), dtype=torch.float64, device=dev)
        self.run = lambda: call(self.maxp, p(self.dmin), p(self.partner), p(self.tca), p(self.pairs), p(self.n))

    def listed(self):
        assert int(self.n[0]) <= self.maxp
        return sort_pairs(self.pairs[:int(self.n[0])].cpu().numpy())


def timed(fn):
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    assert fn() == 0
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def report(name, ms, work):
    med = statistics.median(ms)
    print(f"{name:42s} median {med:9.3f} ms  min {min(ms):9.3f}  max {max(ms):9.3f}  ({len(ms)} runs)  {work / med / 1e6:8.1f} G pair-intervals/s", flush=True)
    return med


for S, D in ((512, 4096), (64, 32768), (4096, 4096)):
    eph, T0, T1 = ephemeris(S, seed=S)
    cat, _, _ = ephemeris(D, seed=100000 + D)
    ws = E(lib.mpcx_conjunction_cross_workspace_bytes(S, D, M), torch.uint8)
    out = Outputs(S, lambda maxp, *o: lib.mpcx_conjunction_cross_screen_dev(ctx, S, D, M, p(eph), p(cat), T0, T1, 0, S, THR, maxp, *o, p(ws), st))
    runs = {"cross": out.run}
    if (S, D) == (512, 4096):
        union = torch.cat([eph, cat]).contiguous()
        wsu = E(lib.mpcx_conjunction_workspace_bytes(S + D, M), torch.uint8)
        outu = Outputs(S + D, lambda maxp, *o: lib.mpcx_conjunction_screen_dev(ctx, S + D, M, p(union), T0, T1, 0, S + D, THR, maxp, *o, p(wsu), st))
        runs["union"] = outu.run
    for _ in range(2):
        for fn in runs.values():
            timed(fn)
    ms = {k: [] for k in runs}
    for _ in range(REPS):
        for k, fn in runs.items():                                   # alternating
            ms[k].append(timed(fn))
    med = report(f"cross screen S {S} D {D} M {M}", ms["cross"], float(S) * D * (M - 1))
    print(f"    dmin min {float(out.dmin.min()):.1f} m, pairs <= 5 km: {int(out.n[0])}", flush=True)
    if "union" in runs:
        medu = report(f"all-pairs screen of the union, S {S + D} M {M}", ms["union"], float(S + D) * (S + D - 1) * (M - 1))
        rows = outu.listed()
        rows = rows[(rows[:, 0] < S) & (rows[:, 1] >= S)]
        rows[:, 1] -= S
        same = rows.tobytes() == out.listed().tobytes()
        print(f"    union / cross: time ratio {medu / med:.2f}  (work ratio {(S + D) ** 2 / (S * D):.2f});  union lists {int(outu.n[0])} pairs <= 5 km, "
              f"{len(rows)} of them (satellite, object); the same bits as the cross screen's list: {same}", flush=True)
        assert same
        del union, wsu, outu
    del eph, cat, ws, out
    torch.cuda.empty_cache()
