"""numpy restatement of "the close approach nearest a listed row's own time" (include/mpcx.h: mpcx_conjunction_track) on top of
conjunction_events_reference: the events of the row's pair without a threshold, and of those the one that minimises (|t - t_row|,
interval); and the iterated avoidance's restatement (avoidance_refine_reference.refine) with that as its re-screen
(mpcx_avoidance_refine_tracked).  Also the two-event scene both are shown on.  Test infrastructure: the product never imports it."""
import functools

import numpy as np

import avoidance_reference as AR
import avoidance_refine_reference as R
import conjunction_events_reference as E
import conjunction_reference as CJ

ST_BADK = 9


def _index(x, N):
    return int(x) if x >= 0.0 and x < N and x == np.floor(x) else -1


def track_rows(pairs, ref, S, D=0, max_shift=None):
    """pairs (n, 4) rows (i, j, ., t_row); ref {(i, j): PairEvents} as all_pairs (D = 0; keys i < j) or against (D > 0; keys
    (satellite, object)) give it; a pair ref does not hold has no valid interval.  -> dict(out (n, 4), info (n, 2) int32,
    status (n,) int32, margin (n,): the second smallest |dt| of the row's admitted events minus the smallest (inf with fewer than
    two), boundary (n,): the smallest | |dt| - max_shift | over the row's events (inf without a limit or without events) --
    how far the row is from a decision that rounding could turn)"""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 4)
    n = len(pairs)
    limit = max_shift if max_shift is not None and max_shift > 0.0 else None
    out = pairs.copy()
    out[:, 2:] = np.nan
    info = np.tile(np.array([-1, 0], dtype=np.int32), (n, 1))
    status = np.zeros(n, dtype=np.int32)
    margin, boundary = np.full(n, np.inf), np.full(n, np.inf)
    for r, (xi, xj, _, tr) in enumerate(pairs):
        i, j = _index(xi, S), _index(xj, D if D > 0 else S)
        if i < 0 or j < 0 or (D == 0 and i == j) or not np.isfinite(tr):
            status[r] = ST_BADK
            continue
        p = ref.get((i, j) if D > 0 else (min(i, j), max(i, j)))
        out[r, 2] = np.inf
        if p is None or p.count == 0:
            continue
        dt = np.abs(p.t - tr)
        if limit is not None:
            boundary[r] = np.abs(dt - limit).min()
        ok = np.flatnonzero(dt <= limit) if limit is not None else np.arange(p.count)
        if len(ok) == 0:
            continue
        order = ok[np.lexsort((p.interval[ok], dt[ok]))]             # by |dt|, then by interval
        k = order[0]
        if len(order) > 1:
            margin[r] = dt[order[1]] - dt[k]
        out[r, 2], out[r, 3] = p.d[k], p.t[k]
        info[r] = (p.interval[k], int(p.edge[k]))
    return dict(out=out, info=info, status=status, margin=margin, boundary=boundary)


def track(pairs, eph, T0, T1, cat_eph=None, max_shift=None):
    """track_rows on the restated events of eph (S, 6, M) [and cat_eph (D, 6, M)] on linspace(T0, T1, M)"""
    if cat_eph is None:
        return track_rows(pairs, E.all_pairs(eph, T0, T1), eph.shape[0], 0, max_shift)
    return track_rows(pairs, E.against(eph, cat_eph, T0, T1), eph.shape[0], cat_eph.shape[0], max_shift)


def rescreen_tracked(pairs, rows, cat, M, T0, T1, max_shift=None):
    """avoidance_refine_reference.rescreen's arguments -> mpcx_conjunction_track_traj's out (n, 4) for the list as GIVEN (column 3
    is the time each row follows)"""
    Y, units, span, ns = rows
    eph, _ = CJ.ephemeris(Y, units, span, M, T0, T1, ns)
    ceph = None
    if cat is not None:
        ceph, _ = CJ.ephemeris(cat[0], cat[1], cat[2], M, T0, T1, cat[3])
    return track(pairs, eph, T0, T1, ceph, max_shift)["out"]


def refine_tracked(*args, max_shift=None, **kw):
    """avoidance_refine_reference.refine (same arguments) with its module-level re-screen replaced by the tracked one for the
    duration of the call: refine hands its re-screen the GIVEN list in every pass, so every row follows its given time"""
    saved = R.rescreen
    R.rescreen = functools.partial(rescreen_tracked, max_shift=max_shift)
    try:
        return R.refine(*args, **kw)
    finally:
        R.rescreen = saved


# ---------------------------------------------------------------- the two-event scene
TARGET = 1000.0
ROUNDS = 3


def coasting_arc(fly=None):
    """avoidance_reference's arc with SCENE["u_scale"] = 0 -- a coasting satellite, K = 30, tf = 0.8 period -- without touching that
    module's cached scene: arc_setup's dict with U = 0 x its thrust table, and x the arc under it (fly(U) -> x (7, K); None: the CPU
    oracle's propagation)"""
    sc = dict(AR.arc_setup())
    sc["U"] = 0.0 * np.random.default_rng(AR.SCENE["seed"]).standard_normal((3, AR.SCENE["K"]))
    sc["x"] = AR.propagate_arc(sc["U"], sc) if fly is None else fly(sc["U"])
    return sc


def two_events(sc):
    """The coasting arc sc against ONE object on a circular orbit that crosses it twice inside the span: planted 200 m away at 0.15
    of the span, the second crossing half a revolution later.  Grid M = 4 (K - 1) + 1 = 117.  -> dict(sc, rows, cat, grid, ref
    (the restated PairEvents of pair (0, 0) on the given arc), pairs (its events as list rows), U, consts)"""
    K = AR.SCENE["K"]
    T0, T1 = float(sc["span"][0]), float(sc["span"][1])
    y, u, s = AR.planted_object(sc, T0 + 0.15 * (T1 - T0), miss=200.0, angle=1.1, n=30)
    cat = (y[None], u[None], s[None], None, None)
    rows = (sc["x"][None], sc["units"][None], sc["span"][None], None)
    M = 4 * (K - 1) + 1
    eph, _ = CJ.ephemeris(*rows[:3], M, T0, T1)
    ceph, _ = CJ.ephemeris(cat[0], cat[1], cat[2], M, T0, T1)
    ref = E.against(eph, ceph, T0, T1)[(0, 0)]
    pairs = np.column_stack([np.zeros(ref.count), np.zeros(ref.count), ref.d, ref.t])
    return dict(sc=sc, rows=rows, cat=cat, grid=(M, T0, T1), ref=ref, pairs=pairs, U=sc["U"][None], consts=sc["consts"][None])


@functools.lru_cache(maxsize=None)
def two_event_scene():
    """two_events on the arc as the CPU oracle flies it.  Treat as read-only."""
    return two_events(coasting_arc())


@functools.lru_cache(maxsize=None)
def two_event_loop(tracked, hold, rounds=ROUNDS):
    """the restated loop on the two-event scene, target 1000 m, no ball -> refine's dict.  Treat as read-only."""
    s = two_event_scene()
    run = refine_tracked if tracked else R.refine
    return run(s["pairs"], None, s["rows"], s["U"], s["consts"], TARGET, s["grid"], rounds, cat=s["cat"], hold_terminal=hold)
