"""The window manoeuvre flown and corrected on the device (csrc/avoidance_window_refine.hip: mpcx_avoidance_window_refine): with
rounds = 0 the whole fly / track / covariance / figure chain against the public calls it is made of, bit for bit, row by row on the
list's own indices; the host tests' slow pair on the arc the device flies against the restatement
(avoidance_window_refine_reference.py) and inside the host tests' conditions; the bits across forms, blocks, contexts and a stale
workspace; the statuses of one call; the C ABI; ConstellationMPC.  Scenes come from test_avoidance_window_gpu.py and the host tests.
The measured figures are in profiles/avoidance_window_refine.txt."""
import functools

import numpy as np
import pytest

import avoidance_reference as AR
import avoidance_window_reference as AW
import avoidance_window_refine_reference as RF
import collision_reference as C
from dev_solve import dev, filled, same_bits, _p, _stream
from test_avoidance_window_gpu import scene, case_rows, scale_constants, CASES

pytestmark = pytest.mark.gpu

TARGET, TOL, MAX_EVAL = 1e-6, 1e-6, 40
PROP_MAX_STEP = 1e-3
Q_NOISE = 1e-8


def grid_of(K):
    """the tracker's grid on test_avoidance_window_gpu.scene: the satellites' span, four intervals per node interval"""
    return (4 * (K - 1) + 1, -1.0, 100.0 * (K - 1) + 1.0)


def side_of(sc, union):
    """(rows, U, consts, pairs, cat) of a form of the scene"""
    if union:
        return sc["urows"], sc["uU"], sc["uconsts"], sc["upairs"], None
    return sc["rows"], sc["U"], sc["consts"], sc["pairs"], sc["cat"]


def refine(sc, union=False, who="i", rounds=0, track=None, recov=False, panels=1, pairs=None, half=None, target=TARGET, **kw):
    from mpconstellation_amd import conjunction as cj
    (Y, units, span, P, radius, ns), U, consts, pr, cat = side_of(sc, union)
    kw.setdefault("tol", TOL); kw.setdefault("max_eval", MAX_EVAL)
    return cj.avoidance_window_refine(pr if pairs is None else pairs, target, radius, Y, U, units, span, consts, P, sc["half"] if half is None else half,
                                      rounds=rounds, track=track, recov=recov, q=Q_NOISE if recov else None, prop_max_step=PROP_MAX_STEP, panels=panels,
                                      ns=ns, cat=cat, who=who, **kw)


def first_order(sc, union=False, who="i", panels=1, pairs=None, half=None, target=TARGET, **kw):
    from mpconstellation_amd import conjunction as cj
    (Y, units, span, P, radius, ns), U, consts, pr, cat = side_of(sc, union)
    kw.setdefault("tol", TOL); kw.setdefault("max_eval", MAX_EVAL)
    return cj.avoidance_window(pr if pairs is None else pairs, target, radius, Y, U, units, span, consts, P, sc["half"] if half is None else half,
                               panels=panels, ns=ns, cat=cat, who=who, **kw)


def bits(r):
    return (r.out.tobytes(), r.du.tobytes(), r.status.tobytes(), r.rounds_done.tobytes(), r.Y_flown.tobytes(), r.p_history.tobytes(),
            r.t_history.tobytes(), r.p_predicted.tobytes())


def same(a, b):
    """the same numbers, NaN where NaN: what two NaNs of different origin can be held to"""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ---------------------------------------------------------------- rounds = 0: the chain through public calls
def chain_row(sc, union, who, av, r, track, recov, panels, max_shift=None):
    """avoidance_window -> apply -> propagate_batch -> [screen_track] -> [covariance] -> collision_probability_window for row r of the
    list, on the list's own indices -> dict(status, t, p, Y (NS, 7, K), P (NS, K, 6, 6))"""
    from mpconstellation_amd import conjunction as cj, propagate_batch, _ffi
    (Y, units, span, P, radius, ns), U, consts, pairs, cat = side_of(sc, union)
    K = Y.shape[2]
    pr = pairs[r]
    NS = 2 if union else 1
    moves = [who != "j", union and who != "i"]
    ok = av.status[r] == 0
    slots = [int(pr[sl]) if ok else 0 for sl in range(NS)]
    o = dict(status=int(av.status[r]), t=pr[3], p=av.p0[r], Y=Y[slots].copy(), P=P[slots].copy())
    if not (ok and av.alpha[r] > 0.0):
        return o
    objs = [slots[sl] for sl in range(NS) if moves[sl]]
    U2 = av.apply(U, r)
    tf = (span[:, 1] - span[:, 0]) / units[:, 1]
    counts = None if ns is None else np.ascontiguousarray(ns[objs])
    y, pst, _ = propagate_batch(np.ascontiguousarray(Y[objs][:, :, 0]), tf[objs], consts[objs], (_ffi.CTRL_SEQUENCE, np.ascontiguousarray(U2[objs]), K, 1.0),
                                K if ns is None else counts, max_step=PROP_MAX_STEP, Kus=counts)
    Yf, Pf = Y.copy(), P.copy()
    for s, yy, st in zip(objs, y, pst):
        if st == 0:
            Yf[s] = 0.0
            Yf[s][:, :yy.shape[1]] = yy
        elif o["status"] == 0:
            o["status"] = int(st)
    row = pr.copy()
    if track is not None:
        M, T0, T1 = track
        cats = {} if cat is None else dict(cat_Y=cat[0], cat_units=cat[1], cat_span=cat[2], cat_ns=cat[5])
        found = cj.screen_track(pr[None], T0, T1, max_shift, Y=Yf, units=units, span=span, ns=ns, M=M, **cats)[0]
        row[2], row[3] = found[0, 2], found[0, 3]
        if not np.isfinite(found[0, 3]):
            row[3] = np.nan
            if o["status"] == 0:
                o["status"] = AW.ST_BADK
    if recov:
        Pm, cst = cj.covariance(Yf[objs], units[objs], span[objs], consts[objs], np.ascontiguousarray(P[objs][:, 0]), U=np.ascontiguousarray(U2[objs]),
                                ns=counts, q=Q_NOISE, return_status=True)
        for s, pp, st in zip(objs, Pm, cst):
            Pf[s] = pp
            if st != 0 and o["status"] == 0:
                o["status"] = int(st)
    win = cj.collision_probability_window(row[None], radius, Yf, units, span, Pf, sc["half"][r:r + 1], panels=panels, ns=ns, cat=cat)
    if win.status[0] != 0 and o["status"] == 0:
        o["status"] = int(win.status[0])
    o.update(t=row[3], p=win.start[0] + win.entries[0] if win.status[0] == 0 else np.nan, Y=Yf[slots], P=Pf[slots])
    return o


def chain_check(sc, union, who, tracked, recov, rows, what, max_shift=None):
    K = sc["rows"][0].shape[2]
    track = grid_of(K) if tracked else None
    av = first_order(sc, union, who, return_sensitivities=True)
    res = refine(sc, union, who, 0, track, recov, return_sensitivities=True, max_shift=max_shift)
    n = len(av.pairs)
    flies = (av.status == 0) & (av.alpha > 0.0)
    assert same_bits(res.out, av.out) and same_bits(res.du, av.du) and same_bits(res.sens, av.sens), what
    assert res.rounds_done.tolist() == np.where(flies, 0, -1).tolist() and same(res.p_history[0], av.p0) and same_bits(res.t_history[0], av.pairs[:, 3])
    assert same(res.p_predicted[0], np.where(flies, av.p1, np.nan)) and res.p_history.shape == (2, n) and res.p_predicted.shape == (1, n)
    assert (res.P_flown is None) == (not recov)
    seen = []
    for r in rows:
        c = chain_row(sc, union, who, av, r, track, recov, 1, max_shift)
        seen.append(c["status"])
        assert res.status[r] == c["status"], (what, r, res.status[r], c["status"])
        assert same(res.t_history[1, r], c["t"]) and same(res.p_history[1, r], c["p"]), (what, r, res.t_history[:, r], c["t"], res.p_history[:, r], c["p"])
        assert same(res.Y_flown[r], c["Y"]), (what, r)
        if recov:
            assert same(res.P_flown[r], c["P"]), (what, r)
        if c["status"] == AW.ST_BADK and av.status[r] == 0:              # the chain's tracker found no event: NaN on both sides
            assert np.isnan(res.p_history[1, r]) and np.isnan(res.t_history[1, r]) and np.isnan(c["p"])
    fixed = ~flies
    assert same(res.p_history[1, fixed], av.p0[fixed]) and same_bits(res.t_history[1, fixed], av.pairs[fixed, 3])
    return res, av, flies, seen


@pytest.mark.parametrize("recov", [False, True])
@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("K,S,n", CASES)
def test_rounds_zero_is_the_chain_of_public_calls(K, S, n, tracked, recov):
    """rounds = 0 in both forms with who = i, j and both: out, du, sens are avoidance_window's bits; for every checked row Y_flown,
    P_flown, t_history[1], p_history[1] and the status are those of the public calls on the list's own indices (at n = 65: the first
    six rows, one more of each class and row 64 past the block of 64).  The scene's thrust table is random and its trajectories are
    Kepler arcs, so the flights are not the plan's own; test_chain_on_a_consistent_plan flies a plan that is."""
    sc = scene(K, S, case_rows(K, S, n))
    rows = list(range(n)) if n < 65 else [0, 1, 2, 3, 4, 5, 36, 37, 38, 39, 64]
    for union, who in ((False, "i"), (True, "i"), (True, "j"), (True, "both")):
        what = f"K {K} S {S} n {n} {'all pairs' if union else 'catalogue'} who {who} tracked {tracked} recov {recov}"
        res, av, flies, seen = chain_check(sc, union, who, tracked, recov, rows, what)
        print(f"{what}: fly {int(flies.sum())} of {n}, statuses of the checked rows {seen}, flown p {res.p_history[1, rows][:6]}")


def test_chain_on_a_consistent_plan():
    """the scene at K = 30 with zero thrust and a constant mass -- the given Kepler arcs ARE the flight of the plan -- so that the
    manoeuvred flights stay at their encounters: the flown figures of the chain are then real probabilities, the same bits"""
    base = scene(30)
    (Y, units, span, P, radius, ns) = base["rows"]
    Y = Y.copy(); Y[:, 6, :] = 1.0
    sc = dict(base, rows=(Y, units, span, P, radius, ns), U=np.zeros_like(base["U"]))
    rows = [j for j in range(65) if j % 4 >= 2 and j != 3][:8] + [0, 64]
    res, av, flies, seen = chain_check(sc, False, "i", True, True, rows, "consistent plan")
    live = [r for r in rows if flies[r] and res.status[r] == 0]
    print(f"consistent plan: fly {int(flies.sum())}, checked statuses {seen}, p0 {av.p0[live]}, flown {res.p_history[1, live]}, target {TARGET}")
    assert len(live) >= 4 and (res.p_history[1, live] > 0.0).all() and (res.p_history[1, live] < av.p0[live]).all()
    # a tracker that may look no further than 10 ms from the given time loses the events the manoeuvres have moved: NaN and
    # MPCX_ST_BADK on both sides, du kept
    res, av, flies, seen = chain_check(sc, False, "i", True, True, rows, "consistent plan, max_shift 0.01 s", max_shift=1e-2)
    lost = [r for r in rows if flies[r] and res.status[r] == AW.ST_BADK]
    print(f"max_shift 0.01 s: checked statuses {seen}")
    assert len(lost) >= 4 and np.isnan(res.p_history[1, lost]).all() and np.isnan(res.t_history[1, lost]).all() and np.isfinite(res.du[lost]).all()


# ---------------------------------------------------------------- the planted slow pair on the arc the device flies
# largest differences between the device's call and the restatement (the CPU oracle's flight and discretisation) on the arc, measured
# on the device when this file was written (profiles/avoidance_window_refine.txt); the tests allow three times as much.  p: |ln(device
# / restated)| of p_history; t: |difference| of t_history in s; du: largest |difference| over the largest |du|.
DEVICE_MEASURED = dict(cat_p=1.064e-10, cat_t=7.117e-10, cat_du=1.163e-11, union_p=2.342e-10, union_t=1.193e-9, union_du=1.981e-11)
ARC_ROUNDS = 2


def allowed(key):
    m = DEVICE_MEASURED[key]
    assert m is not None, f"{key}: no measured figure recorded yet (see the printed differences)"
    return 3.0 * m


@functools.lru_cache(maxsize=None)
def arc_case(union):
    """test_avoidance_window_host.pair_on_arc on the arc as the device flies it (arc_on_device), 2 panels; union: the arc and the
    planted object as one constellation of rows 41 long (the arc has 30 in use), who = both.  -> dict of the call's arguments"""
    from test_avoidance_gpu import arc_on_device
    from test_avoidance_window_host import pair_on_arc, HALF
    a = AR.arc_setup()
    K = AR.SCENE["K"]
    x = arc_on_device(a["U"])
    t, rows, cat, pairs = pair_on_arc(x, a, 20.37)
    U, consts = a["U"][None], a["consts"][None]
    grid = (4 * (K - 1) + 1, float(a["span"][0]), float(a["span"][1]))
    if union:
        (Y, units, span, P, radius, _), (cY, cunits, cspan, cP, cradius, _) = rows, cat
        Kc = cY.shape[2]
        pad = lambda z, ax: np.concatenate([z, np.zeros(z.shape[:ax] + (Kc - K,) + z.shape[ax + 1:])], axis=ax)
        rows = (np.concatenate([pad(Y, 2), cY]), np.concatenate([units, cunits]), np.concatenate([span, cspan]), np.concatenate([pad(P, 1), cP]),
                np.concatenate([radius, cradius]), np.array([K, Kc], dtype=np.int32))
        U, consts = np.concatenate([pad(U, 2), np.zeros((1, 3, Kc))]), np.concatenate([consts, scale_constants(cunits[:, 0])])
        pairs, cat = np.array([[0.0, 1.0, 120.0, t]]), None
    return dict(t=t, rows=rows, cat=cat, pairs=pairs, U=U, consts=consts, half=HALF, grid=grid, who="both" if union else "i")


@functools.lru_cache(maxsize=None)
def arc_on_the_device(union, rounds):
    from mpconstellation_amd import conjunction as cj
    c = arc_case(union)
    Y, units, span, P, radius, ns = c["rows"]
    win0 = cj.collision_probability_window(c["pairs"], radius, Y, units, span, P, c["half"], panels=2, ns=ns, cat=c["cat"])
    target = 1e-2 * (win0.start[0] + win0.entries[0])
    return target, cj.avoidance_window_refine(c["pairs"], target, radius, Y, c["U"], units, span, c["consts"], P, c["half"], rounds=rounds, track=c["grid"],
                                              panels=2, ns=ns, cat=c["cat"], who=c["who"], prop_max_step=AR.SCENE["prop_max_step"],
                                              max_step=AR.SCENE["disc_max_step"])


@pytest.mark.parametrize("union", [False, True])
def test_arc_against_the_restatement(union):
    """p_history, t_history and du against the restatement within 3 x the measured differences; the host test's conditions on the
    device's own histories (the first flight at least 0.05 off in ln P, the last at most 1e-2 of that, at most 4 evaluations in the
    solve of pass 2: EVALS of rounds = 2 less EVALS of rounds = 1); collision_probability_window on Y_flown at t_history[-1] returns
    p_history[-1] to the bit"""
    from mpconstellation_amd import conjunction as cj
    c = arc_case(union)
    key = "union" if union else "cat"
    target, res = arc_on_the_device(union, ARC_ROUNDS)
    _, one = arc_on_the_device(union, 1)
    ref = RF.refine(c["pairs"], c["rows"], c["U"], c["consts"], target, c["half"], 2, ARC_ROUNDS, cols=c["cat"], who=c["who"], track=c["grid"],
                    max_step=AR.SCENE["disc_max_step"], prop_max_step=AR.SCENE["prop_max_step"])
    gaps = np.abs(np.log(res.p_history[1:, 0] / target))
    diff = {f"{key}_p": np.abs(np.log(res.p_history / ref["p_history"])).max(), f"{key}_t": np.abs(res.t_history - ref["t_history"]).max(),
            f"{key}_du": np.abs(res.du - ref["du"]).max() / np.abs(ref["du"]).max()}
    evals2 = res.evals[0] - one.evals[0]
    print(f"{key}: status {res.status.tolist()}, rounds_done {res.rounds_done.tolist()}, target {target:.4e}, p_history {res.p_history[:, 0]}, "
          f"|ln(Q_flown / target)| {gaps}, event at {res.t_history[:, 0] - c['t']} s, evaluations {res.evals[0]:.0f} (pass 2: {evals2:.0f}), "
          f"restated gaps {np.abs(np.log(ref['p_history'][1:, 0] / target))}\n"
          f"measured differences {({k: float(f'{v:.3e}') for k, v in diff.items()})}, recorded {DEVICE_MEASURED}")
    assert res.status.tolist() == [0] and ref["status"].tolist() == [0] and res.rounds_done.tolist() == [ARC_ROUNDS] == ref["rounds_done"].tolist()
    assert gaps[0] >= 0.05 and gaps[-1] <= 1e-2 * gaps[0] and 0 <= evals2 <= 4
    assert same_bits(one.p_history, res.p_history[:3]) and same_bits(one.t_history, res.t_history[:3])       # the passes do not depend on how many follow
    assert (np.abs(np.log(res.p_predicted[:, 0] / target)) <= cj._ffi.AW_DEFAULT_TOL).all() and res.p1[0] == res.p_predicted[-1, 0]
    # the answer as flown, through the public call
    Y, units, span, P, radius, ns = c["rows"]
    obj = [0, 1] if union else [0]
    last = np.array([[0.0, 1.0 if union else 0.0, 0.0, res.t_history[-1, 0]]])
    win = cj.collision_probability_window(last, radius[obj], res.Y_flown[0], units[obj], span[obj], P[obj], c["half"], panels=2,
                                          ns=None if ns is None else ns[obj], cat=c["cat"])
    assert win.status.tolist() == [0] and win.start[0] + win.entries[0] == res.p_history[-1, 0]
    for k, d in diff.items():
        assert d <= allowed(k), (k, d)


def test_arc_with_covariances_propagated_again():
    """recov on the arc, the window held on the given time: P_flown is covariance's chain about (Y_flown, U + du), the window call
    on (Y_flown, P_flown) at t_history[-1] returns p_history[-1] to the bit, and the loop closes although pass 0 aimed with the given
    covariances and every later pass sees the chained ones (2.5 km at the encounter against the given 400 m: the first flight is
    off by 2.2 in ln P).  Tracked, the same call returns a figure for every pass but does not close on this scene: a manoeuvre of
    that size moves the event by hundreds of seconds from pass to pass (a time carried from pass to pass)."""
    from mpconstellation_amd import conjunction as cj
    c = arc_case(False)
    Y, units, span, P, radius, ns = c["rows"]
    target, _ = arc_on_the_device(False, ARC_ROUNDS)
    run = lambda track: cj.avoidance_window_refine(c["pairs"], target, radius, Y, c["U"], units, span, c["consts"], P, c["half"], rounds=ARC_ROUNDS,
                                                   track=track, recov=True, q=Q_NOISE, panels=2, cat=c["cat"],
                                                   prop_max_step=AR.SCENE["prop_max_step"], max_step=AR.SCENE["disc_max_step"])
    for track in (None, c["grid"]):
        res = run(track)
        gaps = np.abs(np.log(res.p_history[1:, 0] / target))
        print(f"recov, {'tracked' if track else 'time held'}: status {res.status.tolist()}, |ln(Q_flown / target)| {gaps}, event at "
              f"{res.t_history[:, 0] - c['t']} s, evaluations {res.evals[0]:.0f}")
        assert res.status.tolist() == [0] and np.isfinite(res.p_history).all()
        if track is None:
            assert gaps[0] >= 0.05 and gaps[-1] <= 1e-2 * gaps[0]
        Pc = cj.covariance(res.Y_flown[0], units, span, c["consts"], P[:, 0], U=res.apply(c["U"], 0), q=Q_NOISE, max_step=AR.SCENE["disc_max_step"])
        assert same_bits(res.P_flown[0], Pc)
        win = cj.collision_probability_window(np.array([[0.0, 0.0, 0.0, res.t_history[-1, 0]]]), radius, res.Y_flown[0], units, span, res.P_flown[0],
                                              c["half"], panels=2, cat=c["cat"])
        assert win.status.tolist() == [0] and win.start[0] + win.entries[0] == res.p_history[-1, 0]


# ---------------------------------------------------------------- the bits
def refine_dev(sc, rounds, track, recov, fill, optional):
    """mpcx_avoidance_window_refine_dev on the catalogue form, every device buffer a torch tensor: the workspace and every result
    pre-filled with `fill`; optional: ask for sens and P_out -> dict of numpy arrays"""
    import torch
    from mpconstellation_amd import _ffi
    from mpconstellation_amd.conjunction import DEFAULT_MAX_STEP
    lib, ctx = _ffi.load(), _ffi.context(0)
    Y, units, span, P, radius, _ = sc["rows"]
    cY, cunits, cspan, cP, cradius, cns = sc["cat"]
    S, _, K = Y.shape
    n, D = len(sc["pairs"]), len(cY)
    M, T0, T1 = track if track is not None else (0, 0.0, 0.0)
    wsb = int(lib.mpcx_avoidance_window_refine_workspace_bytes(n, S, K, D, M, 1))
    assert wsb > 0 and wsb % 8 == 0
    ws = filled(wsb // 8, fill)
    ins = [dev(a) for a in (sc["pairs"], Y, sc["U"], units, span, sc["consts"], P, radius, cns, cY, cunits, cspan, cP, cradius, sc["half"], np.full(S, Q_NOISE))]
    shapes = dict(out=(n, 9), du=(n, 1, 3, K), sens=(n, 1, 3, K), Y_flown=(n, 1, 7, K), P_flown=(n, 1, K, 6, 6), p_history=(rounds + 2, n),
                  t_history=(rounds + 2, n), p_predicted=(rounds + 1, n))
    o = {k: filled(int(np.prod(sh)), fill).reshape(sh) for k, sh in shapes.items()}
    for k in ("status", "rounds_done"):
        o[k] = torch.full((n,), -7, dtype=torch.int32, device=ws.device)
    opt = lambda k: _p(o[k] if optional else None)
    rc = lib.mpcx_avoidance_window_refine_dev(ctx, n, _p(ins[0]), S, K, None, _p(ins[1]), _p(ins[2]), _p(ins[3]), _p(ins[4]), _p(ins[5]), 0, DEFAULT_MAX_STEP,
                                              _p(ins[6]), _p(ins[7]), D, cY.shape[2], _p(ins[8]), _p(ins[9]), _p(ins[10]), _p(ins[11]), _p(ins[12]),
                                              _p(ins[13]), C.MU_EARTH, _p(ins[14]), 1, 0, TARGET, TOL, MAX_EVAL, PROP_MAX_STEP, rounds, M, T0, T1, 0.0,
                                              1 if recov else 0, _p(ins[15]), _p(o["out"]), _p(o["du"]), opt("sens"), _p(o["status"]),
                                              _p(o["rounds_done"]), _p(o["Y_flown"]), opt("P_flown"), _p(o["p_history"]), _p(o["t_history"]),
                                              _p(o["p_predicted"]), _p(ws), _stream(torch))
    _ffi.check(rc, ctx, "avoidance_window_refine_dev")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@functools.lru_cache(maxsize=None)
def consistent_scene():
    """scene(30) with zero thrust and a constant mass (test_chain_on_a_consistent_plan): flights that stay at their encounters, so
    that the solves of the later passes run"""
    base = scene(30)
    (Y, units, span, P, radius, ns) = base["rows"]
    Y = Y.copy(); Y[:, 6, :] = 1.0
    uY = base["urows"][0].copy(); uY[:5, 6, :] = 1.0
    return dict(base, rows=(Y, units, span, P, radius, ns), U=np.zeros_like(base["U"]), urows=(uY,) + base["urows"][1:], uU=np.zeros_like(base["uU"]))


def test_same_bits():
    """the list reversed; a row alone; two rows that move one satellite, each equal to its single-row call; devices=[0, 0]; with and
    without the optional outputs; a second context; the _dev form over a workspace and results full of NaN and of 1e300"""
    from mpconstellation_amd import conjunction as cj, _ffi
    sc = consistent_scene()
    K = 30
    kw = dict(rounds=1, track=grid_of(K), recov=True)
    a = refine(sc, return_sensitivities=True, **kw)
    solved = (a.rounds_done == 1) & (a.evals > 0)
    print(f"statuses {np.bincount(a.status, minlength=10).tolist()}, rounds_done {np.bincount(a.rounds_done + 1).tolist()}, evaluations up to {np.nanmax(a.evals):.0f}, "
          f"rows solved in pass 1: {int(solved.sum())}")
    assert solved.sum() >= 4 and (a.status[a.rounds_done == 1] == 0).all()
    b = refine(sc, return_covariances=False, **kw)
    assert b.sens is None and b.P_flown is None and bits(a) == bits(b)
    c = refine(sc, devices=[0, 0], return_sensitivities=True, **kw)
    assert bits(a) == bits(c) and same_bits(a.sens, c.sens) and same_bits(a.P_flown, c.P_flown)
    rev = refine(sc, pairs=sc["pairs"][::-1].copy(), half=sc["half"][::-1].copy(), return_sensitivities=True, **kw)
    for name in ("out", "du", "status", "rounds_done", "Y_flown", "P_flown", "sens"):
        assert same_bits(getattr(rev, name)[::-1], getattr(a, name)), name
    for name in ("p_history", "t_history", "p_predicted"):
        assert same_bits(getattr(rev, name)[:, ::-1], getattr(a, name)), name
    # two rows that move one satellite do not see each other: each is its single-row call
    sat = int(sc["pairs"][np.flatnonzero(solved)[0], 0])
    mine = [r for r in np.flatnonzero(solved) if int(sc["pairs"][r, 0]) == sat]
    both = [r for r in range(65) if int(sc["pairs"][r, 0]) == sat and a.rounds_done[r] >= 0][:2] if len(mine) < 2 else mine[:2]
    assert len(both) == 2
    for r in both + [64]:
        one = refine(sc, pairs=sc["pairs"][r:r + 1], half=sc["half"][r:r + 1], return_sensitivities=True, **kw)
        for name in ("out", "du", "status", "rounds_done", "Y_flown", "P_flown", "sens"):
            assert same_bits(getattr(one, name), getattr(a, name)[r:r + 1]), (r, name)
        for name in ("p_history", "t_history", "p_predicted"):
            assert same_bits(getattr(one, name), getattr(a, name)[:, r:r + 1]), (r, name)
    for fill, optional in (("nan-", True), ("big", False)):
        d = refine_dev(sc, 1, kw["track"], True, fill, optional)
        for k in ("out", "du", "status", "rounds_done", "Y_flown", "p_history", "t_history", "p_predicted") + (("sens", "P_flown") if optional else ()):
            assert same_bits(d[k], getattr(a, k)), (fill, k)
    # the second context of device 0, by the block call the wrapper makes
    Y, units, span, P, radius, ns = sc["rows"]
    n = 65
    out = dict(out=np.empty((n, _ffi.NAW)), du=np.empty((n, 1, 3, K)), status=np.zeros(n, dtype=np.int32), rounds_done=np.zeros(n, dtype=np.int32),
               Y_flown=np.empty((n, 1, 7, K)), P_flown=np.empty((n, 1, K, 6, 6)), p_history=np.empty((3, n)), t_history=np.empty((3, n)),
               p_predicted=np.empty((2, n)))
    cols = cj._check_side(*sc["cat"][:5], sc["cat"][5], "cat_")
    cj._avoidance_window_refine_call(sc["pairs"], sc["half"], device=0, slot=1, out=out, rows=sc["rows"] + (sc["U"], sc["consts"]), cols=cols,
                                     mu=C.MU_EARTH, panels=1, who=0, flags=0, max_step=cj.DEFAULT_MAX_STEP, atmosphere=None, target_p=TARGET, tol=TOL,
                                     max_eval=MAX_EVAL, prop_max_step=PROP_MAX_STEP, rounds=1, grid=kw["track"] + (0.0,), recov=1, q=np.full(5, Q_NOISE))
    for k, v in out.items():
        assert same_bits(v, getattr(a, k)), k


def test_union_forms_solve_and_hold_their_bits():
    """the all-pairs form of the consistent scene with who = j and both through one solve: a slot that does not move keeps the given
    trajectory and a zero du, the rows that solve predict the target within tol, and a block of the list has the bits of the whole"""
    sc = consistent_scene()
    for who in ("j", "both"):
        a = refine(sc, True, who, rounds=1, track=grid_of(30), recov=True)
        done = a.rounds_done == 1
        print(f"who {who}: statuses {np.bincount(a.status, minlength=10).tolist()}, accepted in pass 1: {int(done.sum())}")
        assert done.sum() >= 4 and (np.abs(np.log(a.p_predicted[1, done] / TARGET)) <= TOL).all()
        fly = a.rounds_done >= 0
        if who == "j":
            rows_i = sc["upairs"][fly, 0].astype(int)
            assert same_bits(a.Y_flown[fly, 0], sc["urows"][0][rows_i]) and not a.du[fly, 0].any() and a.du[done, 1].any(axis=(1, 2)).all()
        part = refine(sc, True, who, rounds=1, track=grid_of(30), recov=True, pairs=sc["upairs"][10:30], half=sc["half"][10:30])
        assert same_bits(part.out, a.out[10:30]) and same_bits(part.du, a.du[10:30]) and same_bits(part.p_history, a.p_history[:, 10:30])


# ---------------------------------------------------------------- statuses
def test_statuses_in_one_call():
    """On the arc, in one call with max_eval = 2 and a target 1e-3 below Q0 in ln: the planted pair, whose pass 0 needs two evaluations
    and whose pass 1 -- the tracked window has moved -- needs three (the restatement's counts, printed): du has pass 0's bits, the
    status is reported, rounds_done = 0 and the two flights are the same; a row with a bad index: NaN and never flown; a row of the same
    pair taken 2000 s early, far below the target: zero with constant histories; the good row again: the bits of the first"""
    from mpconstellation_amd import conjunction as cj
    c = arc_case(False)
    Y, units, span, P, radius, ns = c["rows"]
    win0 = cj.collision_probability_window(c["pairs"], radius, Y, units, span, P, c["half"], panels=1, cat=c["cat"])
    target = (win0.start[0] + win0.entries[0]) * np.exp(-1e-3)
    tol = 3e-7
    pairs = np.repeat(c["pairs"], 4, axis=0)
    pairs[1, 0] = 1.0                                                    # no such satellite
    pairs[2, 3] -= 2000.0
    args = (pairs, target, radius, Y, c["U"], units, span, c["consts"], P, c["half"])
    kw = dict(panels=1, cat=c["cat"], tol=tol, max_eval=2, max_step=AR.SCENE["disc_max_step"])
    av = cj.avoidance_window(*args, **kw)
    res = cj.avoidance_window_refine(*args, rounds=1, track=c["grid"], prop_max_step=AR.SCENE["prop_max_step"], **kw)
    ref = RF.refine(pairs[:1], c["rows"], c["U"], c["consts"], target, c["half"], 1, 1, cols=c["cat"], track=c["grid"], tol=tol, max_eval=[2, 40],
                    max_step=AR.SCENE["disc_max_step"], prop_max_step=AR.SCENE["prop_max_step"])
    print(f"statuses {res.status.tolist()} (pass 0: {av.status.tolist()}), rounds_done {res.rounds_done.tolist()}, evaluations {res.evals.tolist()}, "
          f"restated evaluations per pass {ref['evals'][:, 0].tolist()}, p_history {res.p_history.T.tolist()}")
    assert av.status.tolist() == [0, AW.ST_BADK, 0, 0] and av.alpha[0] > 0.0 and av.alpha[2] == 0.0
    assert res.status[0] in (AW.ST_INFEASIBLE, AW.ST_MAXITER) and res.status[1:].tolist() == [AW.ST_BADK, 0, res.status[0]]
    assert res.rounds_done.tolist() == [0, -1, -1, 0]
    assert same_bits(res.du, av.du) and same_bits(res.out[:, :8], av.out[:, :8]) and res.evals[0] == av.evals[0] + 2
    assert res.p_history[1, 0] == res.p_history[2, 0] and res.t_history[1, 0] == res.t_history[2, 0] != pairs[0, 3]
    assert np.isnan(res.out[1]).all() and np.isnan(res.du[1]).all() and np.isnan(res.p_history[:, 1]).all() and np.isnan(res.p_predicted[:, 1]).all()
    assert same_bits(res.Y_flown[1, 0], Y[0])
    assert not res.du[2].any() and (res.p_history[:, 2] == av.p0[2]).all() and (res.t_history[:, 2] == pairs[2, 3]).all() and av.p0[2] <= target
    assert np.isnan(res.p_predicted[:, 2]).all() and same_bits(res.Y_flown[2, 0], Y[0])
    for name in ("out", "du", "Y_flown"):
        assert same_bits(getattr(res, name)[3], getattr(res, name)[0]), name
    assert same_bits(res.p_history[:, 3], res.p_history[:, 0]) and np.isnan(res.p_predicted[1, 0]) and res.p_predicted[0, 0] == av.p1[0]


# ---------------------------------------------------------------- the C ABI
def test_c_abi_refuses_bad_arguments():
    from mpconstellation_amd import _ffi
    lib, ctx = _ffi.load(), _ffi.context(0)
    S, K, n = 2, 5, 3
    Y, U, units, span, consts = np.ones((S, 7, K)), np.zeros((S, 3, K)), np.ones((S, 2)), np.array([[0.0, 1.0]] * S), np.ones((S, 8))
    P, radius, pairs, half = np.zeros((S, K, 6, 6)), np.ones(S), np.zeros((n, 4)), np.ones(n)
    out, du, st, rd = np.zeros((n, _ffi.NAW)), np.zeros((n, 2, 3, K)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    Yo, hp, ht, hq = np.zeros((n, 2, 7, K)), np.zeros((3, n)), np.zeros((3, n)), np.zeros((2, n))
    d, i = _ffi.dptr, _ffi.iptr

    def call(n=n, who=0, target=1e-4, tol=1e-6, max_eval=10, prop=1e-3, rounds=1, M=0, T0=0.0, T1=1.0, shift=0.0, recov=0, panels=2, out=d(out), du=d(du),
             st=i(st), rd=i(rd), Yo=d(Yo), hp=d(hp), ht=d(ht), hq=d(hq)):
        return lib.mpcx_avoidance_window_refine(ctx, n, d(pairs), S, K, None, d(Y), d(U), d(units), d(span), d(consts), 0, 1e-2, d(P), d(radius), 0, 0, None,
                                                None, None, None, None, None, C.MU_EARTH, d(half), panels, who, target, tol, max_eval, prop, rounds, M, T0, T1,
                                                shift, recov, None, out, du, None, st, rd, Yo, None, hp, ht, hq)
    for bad in (dict(n=0), dict(who=3), dict(target=0.0), dict(target=1.0), dict(tol=0.0), dict(max_eval=0), dict(panels=0), dict(prop=0.0), dict(prop=-1.0),
                dict(rounds=-1), dict(M=1), dict(M=-2), dict(M=5, T0=1.0, T1=1.0), dict(M=5, T0=2.0, T1=1.0), dict(M=5, shift=np.nan), dict(recov=2),
                dict(recov=-1), dict(out=None), dict(du=None), dict(st=None), dict(rd=None), dict(Yo=None), dict(hp=None), dict(ht=None), dict(hq=None)):
        out[:] = 7.0
        assert call(**bad) == -2, bad
        assert b"avoidance_window_refine" in lib.mpcx_last_error(ctx) and (out == 7.0).all(), bad
    wb = lib.mpcx_avoidance_window_refine_workspace_bytes
    assert wb(0, 2, 5, 0, 0, 1) == 0 and wb(3, 0, 5, 0, 0, 1) == 0 and wb(3, 2, 1, 0, 0, 1) == 0 and wb(3, 2, 5, -1, 0, 1) == 0
    assert wb(3, 2, 5, 0, 1, 1) == 0 and wb(3, 2, 5, 0, -1, 1) == 0 and wb(3, 2, 5, 0, 0, 0) == 0 and wb(3, 2, 5, 0, 0, _ffi.PW_MAX_PANELS + 1) == 0
    assert wb(3, 2, 5, 0, 9, 1) > wb(3, 2, 5, 0, 0, 1) > lib.mpcx_avoidance_window_workspace_bytes(3, 2, 5, 1) > 0
    # M = 0 ignores the grid; all-zero covariances fail in pass 0 and nothing flies
    assert call(T0=1.0, T1=0.0, shift=np.nan) == 0 and (st == C.ST_NUMERIC).all() and np.isnan(out).all() and (rd == -1).all() and np.isnan(hp).all()
    assert same_bits(Yo, np.ones((n, 2, 7, K)))


# ---------------------------------------------------------------- ConstellationMPC
def test_constellation_mpc_avoidance_window_refine():
    """test_avoidance_window_gpu.py's planted three-satellite plan: the method returns the screen, the window probabilities and the
    refine result of the module-level call on the plan, bit for bit, and installs nothing"""
    from mpconstellation_amd import Satellite, ConstellationMPC, conjunction as cj
    from mpconstellation_amd.constellation import constellation_states
    st = constellation_states(3)
    mpc = ConstellationMPC([Satellite(s[:3].copy(), s[3:6].copy(), float(s[6])) for s in st], base_res=30, tf_horizon=2, tf_interval=1, r_des=1.5)
    mpc.update()
    (w,) = mpc._screen_windows("plan", samples_per_node=4)
    X = mpc._plan[0]
    m = w["M"] // 3
    tb = w["T0"] + m * ((w["T1"] - w["T0"]) / (w["M"] - 1))
    side = (X, w["units"], w["span"], np.zeros((3, X.shape[2], 6, 6)), np.zeros(3), w["ns"])
    _, pa, va, _, _ = C.state_and_cov_at(side, 0, tb, C.MU_EARTH)
    _, pb, vb, _, _ = C.state_and_cov_at(side, 1, tb, C.MU_EARTH)
    e = np.cross(vb - va, [0.0, 0.0, 1.0]); e /= np.linalg.norm(e)
    X[0, 0:3, :] += ((pb - pa + 500.0 * e) / w["units"][0, 0])[:, None]
    P0 = np.diag([100.0 ** 2] * 3 + [0.1 ** 2] * 3)
    before = (mpc._plan[0].copy(), mpc._plan[1].copy())
    scr, win, res = mpc.avoidance_window_refine(1000.0, P0, 5.0, 60.0, 1e-9, rounds=1, panels=2, q=1e-8, who="both")
    print("planted pair:", scr.pairs, "window p", win.p, "status", res.status, "rounds_done", res.rounds_done, "p_history", res.p_history.T, "t", res.t_history.T)
    assert scr.pairs[:, :2].tolist() == [[0, 1]] and win.status.tolist() == [0] and res.p0[0] == win.start[0] + win.entries[0]
    assert same_bits(mpc._plan[0], before[0]) and same_bits(mpc._plan[1], before[1])
    assert res.du.shape == (1, 2, 3, X.shape[2]) and res.Y_flown.shape == (1, 2, 7, X.shape[2]) and res.P_flown.shape == (1, 2, X.shape[2], 6, 6)
    P = cj.covariance(X, w["units"], w["span"], mpc.consts, P0, U=mpc._plan[1], ns=w["ns"], q=1e-8)
    res2 = cj.avoidance_window_refine(scr, 1e-9, 5.0, X, mpc._plan[1], w["units"], w["span"], mpc.consts, P, 60.0, rounds=1, track=(w["M"], w["T0"], w["T1"]),
                                      recov=True, q=1e-8, panels=2, ns=w["ns"], who="both")
    assert bits(res) == bits(res2) and same_bits(res.P_flown, res2.P_flown)
