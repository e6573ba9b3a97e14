#!/usr/bin/env python3
"""Bits of the encounter chain BEFORE its kernels took their trajectory geometry, covariance prologue, Gates row and flight set from
shared functions (csrc/trajectory_device.hpp, covariance_device.hpp, encounter_host.hpp's FlightSet): inputs and results of one small
case per group of entry points, written by the library built from the commit before that change.
tests/test_encounter_parent_bits_gpu.py holds every later build to them byte for byte.

Needs an MI355X and the OLD library: build the parent commit in a checkout of its own and name its libmpcx.so in MPCX_LIB
(mpconstellation_amd/_ffi.py loads that file instead of the tree's own):

    MPCX_LIB=/path/to/parent/mpconstellation_amd/libmpcx.so python tests/golden/make_encounter_parent_bits.py [OUT.npz]

`check` as the only argument runs whatever library is loaded on the stored inputs and compares instead of writing.

Per case the file holds `<case>.in.<name>` (the arrays BUILD[case] made; the scalars of the calls are in RUN[case] below) and
`<case>.out.<call>.<field>`: every array of every result.  A result above BIG bytes is held by its SHA-256 and shape -- as strict,
byte for byte, and it keeps the file small.

case        entry points and what they reach
ephemeris   common_clock: ragged node counts, a span that covers half the grid (NaN outside it, t == tb inside), an empty span (BADK)
screens     screen and screen_against with a threshold that lists some pairs, then screen_pairs, screen_events and screen_track
            (finite max_shift) on those lists; a pair whose closest approach is interior (the Newton steps) and one at an interval's
            end, both asserted here from the returned times
covariance  covariance (U=None, ragged counts, q for two satellites, a zero time unit: BADK) and covariance_thrust on the same four:
            an all-zero exec row, a full one with mass_var0 > 0 and a node below u_off, a NaN exec entry (NUMERIC)
figures     collision_probability, collision_probability_window (panels = 2), collision_window_sensitivity, avoidance and
            avoidance_window on collision_mc_scenes.slow_pair as a pair of one constellation and as satellite against catalogue
loops       avoidance_window_refine (rounds = 1, tracker M = 17, recov), avoidance_joint, avoidance_refine and its tracked form
            (rounds = 1, M = 17): three satellites, listed rows that share one
mc          collision_probability_mc, 64 samples, scan = 8, two chunks, samples and trajectories returned: pairs of one constellation
            on collision_mc_scenes.thrust_arc(8) with an exec row and one row whose P0 has no factor (NUMERIC); the slow pair's
            satellite against its other object as a catalogue
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, ".."))

NAME = "encounter_parent_bits.npz"
BIG = 24 * 1024
ST_BADK, ST_NUMERIC = 9, 6


# ---------------------------------------------------------------- results as arrays
def arrays_of(res, prefix=""):
    """every array (copied: some come from a pool the next call reuses) and integer of a result object, or of a dict or tuple of them"""
    if res is None:
        return {}
    if isinstance(res, np.ndarray):
        return {prefix.rstrip("."): np.array(res)}
    if isinstance(res, (bool, int, np.integer)):
        return {prefix.rstrip("."): np.array(int(res), dtype=np.int64)}
    out = {}
    if isinstance(res, (tuple, list, dict)):
        for k, r in res.items() if isinstance(res, dict) else enumerate(res):
            out.update(arrays_of(r, f"{prefix}{k}."))
        return out
    for k, v in sorted(vars(res).items()):
        if isinstance(v, (np.ndarray, bool, int, np.integer)):
            out.update(arrays_of(v, f"{prefix}{k}."))
    return out


def stored(key, a, big=BIG):
    """what the file keeps of result `a` under `key`"""
    a = np.ascontiguousarray(a)
    if a.nbytes <= big:
        return {key: a}
    return {key + ".sha256": np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8), key + ".shape": np.array(a.shape, dtype=np.int64)}


def bits(a):
    """the integer view of an array: the sign of a zero and the payload of a NaN count"""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def differs(key, a, old):
    """None where result `a` has the stored bytes of `key` in the file `old`, else what differs"""
    a = np.ascontiguousarray(a)
    if key + ".sha256" in old:
        if tuple(old[key + ".shape"]) != a.shape:
            return f"shape {a.shape}, stored {tuple(old[key + '.shape'])}"
        return None if np.array_equal(np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8), old[key + ".sha256"]) else "SHA-256 differs"
    if key not in old:
        return "not in the file"
    b = old[key]
    if a.dtype != b.dtype or a.shape != b.shape:
        return f"{a.dtype} {a.shape}, stored {b.dtype} {b.shape}"
    ne = bits(a) != bits(b)
    return None if not ne.any() else f"{int(ne.sum())} of {a.size} elements differ, the first at {tuple(int(x[0]) for x in np.nonzero(ne))}"


# ---------------------------------------------------------------- ephemeris
def build_ephemeris():
    import conjunction_reference as R
    orb = R.random_orbits(4, 7)
    n, ns = 9, np.array([2, 5, 9, 9], dtype=np.int32)
    span = np.array([[-1.0, 1601.0], [0.0, 800.0], [-1.0, 1601.0], [-1.0, 1601.0]])
    Y, units = np.zeros((4, 7, n)), np.zeros((4, 2))
    for s in range(4):
        Ys, u, _ = R.trajectories({k: v[s:s + 1] for k, v in orb.items()}, int(ns[s]), span[s])
        Y[s, :, :ns[s]], units[s] = Ys[0], u[0]
    span[2] = (500.0, 500.0)                                             # an empty span
    return dict(Y=Y, units=units, span=span, ns=ns)


def run_ephemeris(w):
    from mpconstellation_amd import common_clock
    eph, status = common_clock(w["Y"], w["units"], w["span"], 17, 0.0, 1600.0, ns=w["ns"], return_status=True)
    assert status.tolist() == [0, 0, ST_BADK, 0] and np.isnan(eph[2]).all()
    assert np.isfinite(eph[1, :, :9]).all() and np.isnan(eph[1, :, 9:]).all()         # instant 8 is t = 800 = tb
    return dict(clock=(eph, status))


# ---------------------------------------------------------------- screens
SCREEN_M = 33


def build_screens():
    import conjunction_reference as R
    w = {}
    for tag, count, seed in (("s", 5, 104), ("x", 7, 204)):
        orb = R.random_orbits(count, seed)
        T1 = 2 * np.pi / R.orbit_rate(orb).max()
        span = np.tile([-1.0, T1 + 1.0], (count, 1))
        span[count - 1, 1] = 0.55 * T1                                    # the last object leaves the grid half way: pairs still closing there
        if tag == "x":
            span[5, 0] = 0.3 * T1
        Y, units, span = R.trajectories(orb, 40, span)
        w.update({tag + "Y": Y, tag + "units": units, tag + "span": span, tag + "T1": np.array(T1)})
    return w


def _list_calls(lst, T0, T1, h, **eph):
    from mpconstellation_amd import screen_pairs, screen_events, screen_track
    moved = lst.copy()
    moved[:, 3] += 0.4 * h * np.where(np.arange(len(lst)) % 2 == 0, 1.0, -5.0)       # every second row beyond max_shift from where it was
    return dict(pairs=screen_pairs(lst, T0, T1, **eph), events=screen_events(lst, T0, T1, **eph),
                track=screen_track(moved, T0, T1, max_shift=h, **eph), track_back=screen_track(lst, T0, T1, max_shift=h, **eph))


def _assert_interior_and_end(pairs, T0, T1):
    import conjunction_reference as R
    t, _ = R.grid(SCREEN_M, T0, T1)
    on = np.isin(pairs[:, 3], t)
    assert on.any() and (~on).any(), pairs                              # an interval's end; the Newton steps


def run_screens(w):
    from mpconstellation_amd import common_clock, screen, screen_against
    out = {}
    M, T0 = SCREEN_M, 0.0
    T1 = float(w["sT1"]); h = (T1 - T0) / (M - 1)
    eph = common_clock(w["sY"], w["sunits"], w["sspan"], M, T0, T1)
    scr = screen(eph, T0, T1, threshold=3.0e6)
    assert 0 < len(scr.pairs) < 10
    _assert_interior_and_end(scr.pairs, T0, T1)
    out.update(self_eph=eph, self_screen=scr, **{"self_" + k: v for k, v in _list_calls(scr.pairs, T0, T1, h, eph=eph).items()})
    T1 = float(w["xT1"]); h = (T1 - T0) / (M - 1)
    eph = common_clock(w["xY"], w["xunits"], w["xspan"], M, T0, T1)
    sat, cat = np.ascontiguousarray(eph[:3]), np.ascontiguousarray(eph[3:])
    scr = screen_against(sat, cat, T0, T1, threshold=7.0e6)
    assert 0 < len(scr.pairs) < 12
    _assert_interior_and_end(scr.pairs, T0, T1)
    out.update(cross_eph=eph, cross_screen=scr, **{"cross_" + k: v for k, v in _list_calls(scr.pairs, T0, T1, h, eph=sat, cat_eph=cat).items()})
    return out


# ---------------------------------------------------------------- covariance
def build_covariance():
    import collision_reference as C
    from test_covariance_thrust_gpu import thrust_case, EXEC
    c = thrust_case(4, 6, True)
    units = c["units"].copy()
    units[3, 1] = 0.0                                                    # no tf: BADK
    ex = np.stack([np.zeros(5), EXEC, EXEC, EXEC])
    ex[2, 3] = np.nan                                                    # NUMERIC
    U = c["U"].copy()
    nn = int(c["ns"][1])
    U[1, :, nn - 1] = np.array([0.3, -0.4, 0.0]) * EXEC[4]              # a node below u_off on the satellite with the full row
    return dict(Y=c["Y"], units=units, span=c["span"], ns=c["ns"], consts=c["consts"], U=U, ex=ex, mv=np.array([0.0, 1e-4, 0.0, 0.0]),
                q=np.array([1e-6, 0.0, 1e-7, 0.0]), P0=np.array(C.P0_TEST))


def run_covariance(w):
    from mpconstellation_amd import covariance, covariance_thrust
    plain = covariance(w["Y"], w["units"], w["span"], w["consts"], w["P0"], U=None, ns=w["ns"], q=w["q"], return_status=True)
    thrust = covariance_thrust(w["Y"], w["units"], w["span"], w["consts"], w["P0"], w["U"], w["ex"], mass_var0=w["mv"], ns=w["ns"], q=w["q"],
                               return_status=True, return_mass=True)
    assert plain[1].tolist() == [0, 0, 0, ST_BADK] and thrust[2].tolist() == [0, 0, ST_NUMERIC, ST_BADK]
    return dict(plain=plain, thrust=thrust)


# ---------------------------------------------------------------- figures
def build_figures():
    import collision_mc_scenes as SC
    from mpconstellation_amd import covariance
    sc = SC.slow_pair()
    P, st = covariance(sc["Y"], sc["units"], sc["span"], sc["consts"], sc["P0"], return_status=True)
    assert (st == 0).all()
    return dict(Y=sc["Y"], units=sc["units"], span=sc["span"], consts=sc["consts"], radius=sc["radius"], P=np.array(P), pairs=sc["pairs"])


def run_figures(w):
    from mpconstellation_amd import conjunction as cj
    Y, units, span, consts, radius, P = (w[k] for k in ("Y", "units", "span", "consts", "radius", "P"))
    U = np.zeros((2, 3, Y.shape[2]))
    half, panels = 2000.0, 2
    out = {}
    for form in ("pair", "cat"):
        if form == "pair":
            side, plan, pairs, cat6, cat3 = (Y, units, span, P), (Y, U, units, span, consts), w["pairs"], None, None
            rad = radius
        else:
            side, plan = (Y[:1], units[:1], span[:1], P[:1]), (Y[:1], U[:1], units[:1], span[:1], consts[:1])
            pairs, rad = np.array([[0.0, 0.0, 50.0, 3000.0]]), radius[:1]
            cat6, cat3 = (Y[1:], units[1:], span[1:], P[1:], radius[1:]), (Y[1:], units[1:], span[1:])
        res = dict(pc=cj.collision_probability(pairs, rad, *side, cat=cat6),
                   window=cj.collision_probability_window(pairs, rad, *side, half, panels=panels, cat=cat6),
                   sens=cj.collision_window_sensitivity(pairs, rad, *plan, side[3], half, panels=panels, cat=cat6),
                   avoid=cj.avoidance(pairs, 200.0, *plan, cat=cat3, return_sensitivities=True),
                   avoid_window=cj.avoidance_window(pairs, 1e-3, rad, *plan, side[3], half, panels=panels, cat=cat6, return_sensitivities=True))
        if form == "pair":
            res["avoid_both"] = cj.avoidance(pairs, 4.0, *plan, P=P, who="both")
        for k, r in res.items():
            assert (r.status == 0).all(), (form, k, r.status)
            out[f"{form}_{k}"] = r
    return out


# ---------------------------------------------------------------- loops
LOOP_K = 13


def build_loops():
    from test_avoidance_gpu import scene as fast_scene
    from test_avoidance_window_gpu import scene as slow_scene
    w = {}
    sc = slow_scene(LOOP_K, 3, (6, 7))                                   # two slow rows of satellite 2
    Y, units, span, P, radius, _ = sc["rows"]
    objs = sc["pairs"][:, 1].astype(int)
    cY, cunits, cspan, cP, cradius, cns = (np.ascontiguousarray(x[objs]) for x in sc["cat"])
    pairs = sc["pairs"].copy()
    pairs[:, 1] = np.arange(len(pairs))
    assert pairs[0, 0] == pairs[1, 0]
    w.update(wY=Y, wunits=units, wspan=span, wP=P, wradius=radius, wU=sc["U"], wconsts=sc["consts"], wpairs=pairs, whalf=sc["half"],
             wcY=cY, wcunits=cunits, wcspan=cspan, wcP=cP, wcradius=cradius, wcns=cns)
    sc = fast_scene(3, LOOP_K, 3, False)                                 # rows 0 and 1 are satellite 0's
    (Y, units, span, _), (cY, cunits, cspan, cns, _) = sc["rows"], sc["cat"]
    assert sc["pairs"][0, 0] == sc["pairs"][1, 0]
    w.update(fY=Y, funits=units, fspan=span, fU=sc["U"], fconsts=sc["consts"], fpairs=sc["pairs"], fcY=cY, fcunits=cunits, fcspan=cspan, fcns=cns)
    return w


def run_loops(w):
    from mpconstellation_amd import conjunction as cj
    K = LOOP_K
    cat6 = tuple(w[k] for k in ("wcY", "wcunits", "wcspan", "wcP", "wcradius", "wcns"))
    window = cj.avoidance_window_refine(w["wpairs"], 1e-6, w["wradius"], w["wY"], w["wU"], w["wunits"], w["wspan"], w["wconsts"], w["wP"], w["whalf"],
                                        rounds=1, track=(17, -1.0, 100.0 * (K - 1) + 1.0), recov=True, q=1e-8, prop_max_step=1e-3, panels=1,
                                        cat=cat6, tol=1e-6, max_eval=40, return_sensitivities=True)
    plan = tuple(w[k] for k in ("fY", "fU", "funits", "fspan", "fconsts"))
    cat = tuple(w[k] for k in ("fcY", "fcunits", "fcspan", "fcns"))
    target = 1.0e7                                                      # (rows of few nodes interpolate badly: test_avoidance_joint_gpu.targets)
    joint = cj.avoidance_joint(w["fpairs"], target, *plan, cat=cat, return_rows=True, return_terminal=True)
    grid = dict(M=17, T0=-1.0, T1=2999.0, rounds=1, prop_max_step=1e-3, return_rows=True, return_terminal=True, return_rhs=True)
    refine = cj.avoidance_refine(w["fpairs"], target, *plan, cat=cat, **grid)
    tracked = cj.avoidance_refine(w["fpairs"], target, *plan, cat=cat, track=True, max_shift=400.0, **grid)
    return dict(window=window, joint=joint, refine=refine, tracked=tracked)


# ---------------------------------------------------------------- Monte Carlo
def build_mc():
    import collision_mc_scenes as SC
    a = SC.thrust_arc(8)
    three = lambda x: np.ascontiguousarray(np.repeat(x, 3, axis=0))
    P0 = np.stack([a["P0"], a["P0"], -a["P0"]])                          # object 2: no factor
    t = 0.5 * a["span"][0, 1]
    sc = SC.slow_pair()
    return dict(aY=three(a["Y"]), aU=three(a["U"]), aunits=three(a["units"]), aspan=three(a["span"]), aconsts=three(a["consts"]), aP0=P0,
                apairs=np.array([[0.0, 1.0, 0.0, t], [0.0, 2.0, 0.0, t]]), aex=np.array(SC.EXEC),
                sY=sc["Y"], sunits=sc["units"], sspan=sc["span"], sconsts=sc["consts"], sP0=sc["P0"], sradius=sc["radius"])


def run_mc(w):
    from mpconstellation_amd import collision_probability_mc
    kw = dict(seed=12345 + (7 << 40), scan=8, return_samples=True, return_trajectories=True)
    arc = collision_probability_mc(w["apairs"], 5.0, w["aY"], w["aU"], w["aunits"], w["aspan"], w["aconsts"], w["aP0"], 10.0, 64, execution=w["aex"],
                                   mass_var0=1e-6, max_flights=2 * 2 * 32, **kw)
    assert arc.status.tolist() == [0, ST_NUMERIC], arc.status
    cat = tuple(w[k][1:] for k in ("sY", "sunits", "sspan", "sconsts", "sP0", "sradius"))
    slow = collision_probability_mc(np.array([[0.0, 0.0, 50.0, 3000.0]]), w["sradius"][:1], w["sY"][:1], None, w["sunits"][:1], w["sspan"][:1],
                                    w["sconsts"][:1], w["sP0"][:1], 2000.0, 64, cat=cat, max_flights=32, **kw)
    assert slow.status.tolist() == [0], slow.status
    return dict(arc=arc, slow=slow)


BUILD = dict(ephemeris=build_ephemeris, screens=build_screens, covariance=build_covariance, figures=build_figures, loops=build_loops, mc=build_mc)
RUN = dict(ephemeris=run_ephemeris, screens=run_screens, covariance=run_covariance, figures=run_figures, loops=run_loops, mc=run_mc)
CASES = list(RUN)


def inputs_of(old, case):
    pre = f"{case}.in."
    return {k[len(pre):]: old[k] for k in old.files if k.startswith(pre)}


def results(case, w):
    """{`<call>.<field>`: array} of the loaded library on the case's inputs"""
    return arrays_of(RUN[case](w))


def main():
    check = sys.argv[1:] == ["check"]
    path = os.path.join(HERE, NAME) if check or not sys.argv[1:] else sys.argv[1]
    old = np.load(path) if check else None
    out, bad = {}, 0
    for case in CASES:
        try:
            w = inputs_of(old, case) if check else BUILD[case]()
            res = results(case, w)
        except (AssertionError, ValueError, TypeError, KeyError, AttributeError):   # (of the case's own making; an error of the library's ends the run)
            import traceback
            traceback.print_exc()
            bad += 1
            continue
        print(f"{case:10s}: {len(w)} inputs of {sum(a.nbytes for a in w.values())} bytes, {len(res)} results of {sum(a.nbytes for a in res.values())} bytes")
        if check:
            for k, a in res.items():
                what = differs(f"{case}.out.{k}", a, old)
                if what:
                    bad += 1
                    print(f"    {k}: {what}")
            want = {k for k in old.files if k.startswith(f"{case}.out.")}
            have = {f"{case}.out.{k}" for k in res}
            missing = {k for k in want if k.replace(".sha256", "").replace(".shape", "") not in have}
            bad += len(missing)
            for k in sorted(missing):
                print(f"    {k}: stored, not returned")
        else:
            out.update({f"{case}.in.{k}": np.asarray(a) for k, a in w.items()})
            for k, a in res.items():
                out.update(stored(f"{case}.out.{k}", a))
    if check:
        print("identical" if not bad else f"{bad} arrays differ")
        return 1 if bad else 0
    if bad:
        print(f"{bad} cases failed: nothing written")
        return 1
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
