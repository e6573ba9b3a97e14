"""Wall time of avoidance_window_refine against the chain of public calls it replaces, on the same list: 4096 rows (the 65 rows of
tests/collision_window_reference.window_scene(30), repeated), 4 panels, K = 30, host arrays in and out, one device.  rounds = 0 is
avoidance_window -> U + du -> propagate_batch -> [screen_track] -> [covariance] -> collision_probability_window; the chain here makes
those calls once each on every row's own copy of its satellite (a constellation of n trajectories gathered in numpy), which is the
cheapest way to make them from Python.  The call and the chain alternate, `reps` rounds after one warm-up round; the host clock runs
around calls that end in a device synchronise.  The chain's flown figure must have the call's bits.  rounds = 2 is timed beside them.
    python profiles/tools/avoidance_window_refine_timing.py [reps]"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))

TARGET, Q_NOISE, PROP_MAX_STEP = 1e-6, 1e-8, 1e-3


def main(reps=5, n=4096, panels=4):
    import collision_window_reference as CW
    from mpconstellation_amd import conjunction as cj, propagate_batch, _ffi
    from mpconstellation_amd.satellite_scale import SatelliteScale
    K = 30
    sc = CW.window_scene(K)
    Y, units, span, P, radius, _ = sc["rows"]
    cat = sc["cat"]
    Y = Y.copy(); Y[:, 6, :] = 1.0 - 0.1 * np.arange(K) / K
    U = 0.02 * np.random.default_rng(1).standard_normal((len(Y), 3, K))
    consts = np.stack([SatelliteScale(x=np.array([L, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])).get_normalized_constants().as_vector() for L in units[:, 0]])
    times = -(-n // len(sc["pairs"]))
    pairs, half = np.tile(sc["pairs"], (times, 1))[:n], np.tile(sc["half"], times)[:n]
    grid = (4 * (K - 1) + 1, -1.0, 100.0 * (K - 1) + 1.0)
    tf = (span[:, 1] - span[:, 0]) / units[:, 1]

    def call(rounds, full):
        return cj.avoidance_window_refine(pairs, TARGET, radius, Y, U, units, span, consts, P, half, rounds=rounds, track=grid if full else None,
                                          recov=full, q=Q_NOISE if full else None, prop_max_step=PROP_MAX_STEP, panels=panels, cat=cat,
                                          return_covariances=False)

    def chain(full):
        av = cj.avoidance_window(pairs, TARGET, radius, Y, U, units, span, consts, P, half, panels=panels, cat=cat)
        ok = av.status == 0
        flies = ok & (av.alpha > 0.0)
        obj = np.where(ok, pairs[:, 0], 0.0).astype(int)
        Uv = np.where(flies[:, None, None], U[obj] + np.where(flies[:, None, None], av.du[:, 0], 0.0), U[obj])
        y, st, _ = propagate_batch(np.ascontiguousarray(Y[obj][:, :, 0]), tf[obj], consts[obj], (_ffi.CTRL_SEQUENCE, Uv, K, 1.0), K, max_step=PROP_MAX_STEP)
        flown = flies & (st == 0)
        Yv = np.where(flown[:, None, None], y, Y[obj])
        pv = pairs.copy()
        pv[:, 0] = np.where(ok, np.arange(n), np.nan)
        uv, sv = np.ascontiguousarray(units[obj]), np.ascontiguousarray(span[obj])
        if full:
            found = cj.screen_track(pv, grid[1], grid[2], Y=Yv, units=uv, span=sv, cat_Y=cat[0], cat_units=cat[1], cat_span=cat[2], cat_ns=cat[5], M=grid[0])[0]
            pv[:, 3] = np.where(flies, found[:, 3], pairs[:, 3])
            Pv = cj.covariance(Yv, uv, sv, consts[obj], np.ascontiguousarray(P[obj][:, 0]), U=Uv, q=Q_NOISE)
            Pv = np.where(flies[:, None, None, None], Pv, P[obj])
        else:
            Pv = P[obj]
        win = cj.collision_probability_window(pv, radius[obj], Yv, uv, sv, Pv, half, panels=panels, cat=cat)
        return av, flies, np.where(flies, win.start + win.entries, av.p0)

    runs = {"call, rounds 0": lambda: call(0, False), "chain of public calls": lambda: chain(False),
            "call, rounds 0, track + recov": lambda: call(0, True), "chain, track + recov": lambda: chain(True),
            "call, rounds 2": lambda: call(2, False), "call, rounds 2, track + recov": lambda: call(2, True)}
    seen = {name: [] for name in runs}
    last = {}
    for r in range(reps + 1):
        for name, f in runs.items():
            t0 = time.perf_counter()
            last[name] = f()
            if r:
                seen[name].append(time.perf_counter() - t0)
    for a, b in (("call, rounds 0", "chain of public calls"), ("call, rounds 0, track + recov", "chain, track + recov")):
        res, (av, flies, flown) = last[a], last[b]
        assert res.out.tobytes() == av.out.tobytes() and res.du.tobytes() == av.du.tobytes()
        assert np.array_equal(res.p_history[1], flown, equal_nan=True), (a, np.flatnonzero(~((res.p_history[1] == flown) | np.isnan(flown)))[:10])
    r2 = last["call, rounds 2, track + recov"]
    fl = r2.rounds_done >= 0
    print(f"n {n} rows, {panels} panels, K {K}; rows that fly {int(fl.sum())}; rounds = 2, track + recov: statuses {np.bincount(r2.status, minlength=10).tolist()}, "
          f"rounds_done {np.bincount(r2.rounds_done + 1, minlength=4).tolist()} (from -1), evaluations per flying row {np.nanmean(r2.evals[fl]):.2f}")
    for name, ts in seen.items():
        print(f"{name:32s} smallest {1e3 * min(ts):9.2f} ms   median {1e3 * float(np.median(ts)):9.2f} ms   ({len(ts)} calls)")


if __name__ == "__main__":
    main(*(int(x) for x in sys.argv[1:2]))
