"""profiling helper: the HOST time of conjunction.py's wrappers, without a device.  _ffi.call and _ffi.context are replaced by
stubs (as the recorder of tests/test_wrapper_calls_host.py does), so what is timed is the argument checks, the allocation of the
result arrays, the marshalling and the dispatch to the block functions -- everything a wrapper does around its library call.
Shapes: those of tests/test_conjunction_calls_host.py (3 satellites of 5 nodes, a list of 3 rows), where that time is all overhead.
Timed: collision_probability, screen_pairs, avoidance_window_refine on one device and on devices=[0, 0] (two blocks on the thread
pool), CALLS calls each, microseconds per call.

    python profiles/tools/conjunction_wrappers_timing.py                      one repeat of this tree, one line per wrapper
    python profiles/tools/conjunction_wrappers_timing.py --against OTHER      OTHER: a checkout of the commit to compare with; this
        tree and OTHER alternately in fresh processes, REPEATS repeats each; per wrapper both sets of figures, and the verdict: this
        tree's median must not exceed OTHER's slowest repeat by more than OTHER's own spread (its slowest minus its fastest)"""
import argparse, json, os, statistics, subprocess, sys, time

CALLS, REPEATS = 3000, 5
HERE = os.path.dirname(os.path.abspath(__file__))


def one_repeat(root):
    sys.path.insert(0, root)
    import numpy as np
    from mpconstellation_amd import _ffi, conjunction as cj
    _ffi.call = lambda name, *args, popts=None: None
    _ffi.context = lambda device=0, slot=0: None
    S, N, M, T0, T1 = 3, 5, 6, 10.0, 60.0
    ramp = lambda *shape: 1.0 + 0.01 * np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
    Y, U, units, span, consts, P, eph = ramp(S, 7, N), ramp(S, 3, N), ramp(S, 2), ramp(S, 2), ramp(S, 8), ramp(S, N, 6, 6), ramp(S, 6, M)
    pairs = np.array([[0, 1, 100.0, 20.0], [2, 0, 200.0, 30.0], [1, 0, 300.0, 40.0]])
    refine = lambda **where: cj.avoidance_window_refine(pairs, 0.001, 5.0, Y, U, units, span, consts, P, 10.0, rounds=1, track=(M, T0, T1),
                                                        recov=True, q=0.5, include_J2=True, **where)
    cases = {"collision_probability": lambda: cj.collision_probability(pairs, 5.0, Y, units, span, P),
             "screen_pairs": lambda: cj.screen_pairs(pairs, T0, T1, eph=eph),
             "avoidance_window_refine": refine,
             "avoidance_window_refine devices=[0, 0]": lambda: refine(devices=[0, 0])}
    out = {}
    for name, fn in cases.items():
        for _ in range(CALLS // 10):
            fn()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        out[name] = (time.perf_counter() - t0) / CALLS * 1e6
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(HERE, "..", ".."), help="the tree whose mpconstellation_amd is timed")
    ap.add_argument("--against", default=None, help="another tree: both alternately, REPEATS repeats each")
    ap.add_argument("--json", action="store_true", help="print the figures as one JSON line")
    a = ap.parse_args()
    if a.against is None:
        res = one_repeat(os.path.abspath(a.root))
        print(json.dumps(res) if a.json else "\n".join(f"{k:44s} {v:8.2f} us per call ({CALLS} calls)" for k, v in res.items()))
        sys.exit(0)
    runs = {"other": [], "this": []}
    for _ in range(REPEATS):                                             # alternating: both see the same minutes of the machine
        for who, root in (("other", a.against), ("this", a.root)):
            line = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--root", os.path.abspath(root), "--json"], text=True)
            runs[who].append(json.loads(line.strip().splitlines()[-1]))
    ok = True
    print(f"microseconds per call, {CALLS} calls per repeat, {REPEATS} repeats each, alternating; other = {os.path.abspath(a.against)}")
    for name in runs["this"][0]:
        other, this = sorted(r[name] for r in runs["other"]), sorted(r[name] for r in runs["this"])
        bound = other[-1] + (other[-1] - other[0])
        verdict = statistics.median(this) <= bound
        ok &= verdict
        print(f"{name}\n    other {' '.join(f'{v:7.2f}' for v in other)}   median {statistics.median(other):7.2f}\n"
              f"    this  {' '.join(f'{v:7.2f}' for v in this)}   median {statistics.median(this):7.2f}   "
              f"bound (other's slowest + its spread) {bound:7.2f}: {'within' if verdict else 'EXCEEDED'}")
    sys.exit(0 if ok else 1)
