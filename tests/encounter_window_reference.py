"""numpy restatement of the encounter window (include/mpcx.h: mpcx_encounter_window) -- the rule of csrc/encounter_window.hip line by
line, one array entry per scan time where the device has one lane, on the node of collision_window_reference (relative_state,
node_setup: the restatement of cw_node).  Beside the device's outputs it reports every row's MARGIN, the smallest |g| over every time
it evaluated: a row whose margin is above the rounding of g is decided -- no other correct fp64 evaluation can test a time the other
way -- and only such rows are held to the device bit-tight.  Test infrastructure: the product never imports it."""
import numpy as np

import collision_window_reference as W

MU_EARTH = W.MU_EARTH
ST_OK, ST_NUMERIC, ST_BADK = W.ST_OK, W.ST_NUMERIC, W.ST_BADK
NEW = 6
EW_HALF, EW_TA, EW_TB, EW_REACH_BEFORE, EW_REACH_AFTER, EW_G0 = range(NEW)
CLEAR, OPEN_BEFORE, OPEN_AFTER, BAD_SCAN = 1, 2, 4, 8
MAX_LEVELS = 4
LANES = 64


def g_of(d, Li, Rp, nsigma):
    """g = |L^-1 d| - Rp |L^-1|_F - nsigma from the mean d (3, T) and Li = (i00, i10, i11, i20, i21, i22), each (T,)"""
    i00, i10, i11, i20, i21, i22 = Li
    with np.errstate(all="ignore"):
        z0 = i00 * d[0]
        z1 = i10 * d[0] + i11 * d[1]
        z2 = i20 * d[0] + i21 * d[1] + i22 * d[2]
        zn = np.sqrt(z0 * z0 + z1 * z1 + z2 * z2)
        fn = np.sqrt(i00 * i00 + i10 * i10 + i11 * i11 + i20 * i20 + i21 * i21 + i22 * i22)
        return (zn - Rp * fn) - nsigma


def window_search(g, H, levels):
    """The rule on a function of the OFFSET alone: g(sign, offsets (T,)) -> (code (T,), g (T,)), code ST_OK, ST_BADK (outside a span:
    not live) or ST_NUMERIC (live, sets BAD_SCAN); g(0, [0]) is the row's own time.  -> (status, [reach_before, reach_after], g0, flags,
    margin).  The time t, the spans and the outputs' cuts are the caller's (encounter_window below)."""
    code, g0 = g(0.0, np.zeros(1))
    code, g0 = int(code[0]), float(g0[0])
    if code != ST_OK:
        return code, None, np.nan, 0, np.nan
    if not np.isfinite(g0):
        return ST_NUMERIC, None, np.nan, 0, np.nan
    margin, flags = abs(g0), 0
    if g0 > 0.0:                                                         # clear: nothing is searched
        cell = H
        for _ in range(levels):
            cell = cell / 64.0
        return ST_OK, [cell, cell], g0, CLEAR, margin
    reach = [0.0, 0.0]
    lane = np.arange(LANES)
    for sd, sg in enumerate((-1.0, 1.0)):
        lb, ub = 0.0, H
        for lv in range(levels):
            wd = (ub - lb) / 64.0
            off = lb + (lane + 1.0) * wd                                 # (the device: one fused multiply-add)
            code, gv = g(sg, off)
            with np.errstate(invalid="ignore"):
                live = np.where(code == ST_OK, gv <= 0.0, code != ST_BADK)
            if (code == ST_NUMERIC).any():
                flags |= BAD_SCAN
            seen = code == ST_OK
            if seen.any():
                margin = min(margin, float(np.nanmin(np.abs(gv[seen]))))
            dead = np.flatnonzero(~live)
            if len(dead) == 0:
                if lv == 0:
                    flags |= OPEN_AFTER if sd else OPEN_BEFORE
                break
            ls = int(dead[0])
            lb, ub = lb + ls * wd, lb + (ls + 1.0) * wd
        reach[sd] = ub
    return ST_OK, reach, g0, flags, margin


def _pair_g(rows, cols, oa, ob, sa, sb, t, mu, Rp, nsigma):
    """g of the pair (oa, ob) as window_search takes it: cw_node at t + sign offset -- ST_BADK outside either span, ST_NUMERIC for a
    pivot that is not positive and finite or a relative speed that is not finite"""
    def g(sg, off):
        tau = t + sg * off
        inside = (tau >= sa[0]) & (tau <= sa[1]) & (tau >= sb[0]) & (tau <= sb[1])
        code = np.where(inside, ST_OK, ST_BADK)
        gv = np.full(len(tau), np.nan)
        if inside.any():
            with np.errstate(all="ignore"):
                d, w, A, B, D = W.relative_state(rows, cols, oa, ob, tau[inside], mu)
                wn = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
                ok, Li, _, _, _ = W.node_setup(A, B, D)
                good = ok & np.isfinite(wn)
                gi = g_of(d, Li, Rp, nsigma)
            idx = np.flatnonzero(inside)
            code[idx[~good]] = ST_NUMERIC
            gv[idx[good]] = gi[good]
        return code, gv
    return g


def encounter_window(pairs, rows, max_half, nsigma=8.0, levels=3, cols=None, mu=MU_EARTH):
    """pairs (n, 4); rows, cols = (Y, units, span, P, radius, ns) (cols None: the columns are the rows); max_half a scalar or (n,) ->
    out (n, 6), flags (n,), status (n,), margin (n,) (NaN for a failed row)"""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 4)
    cols = rows if cols is None else cols
    mh = np.broadcast_to(np.asarray(max_half, dtype=np.float64), (len(pairs),))
    out = np.full((len(pairs), NEW), np.nan)
    flags = np.zeros(len(pairs), dtype=np.int32)
    status = np.zeros(len(pairs), dtype=np.int32)
    margin = np.full(len(pairs), np.nan)
    for n, (i, j, _, t) in enumerate(pairs):
        H = float(mh[n])
        st, oa, sa = W._object_check(rows, i, t)
        if st == ST_OK:
            st, ob, sb = W._object_check(cols, j, t)
        if st == ST_OK and not (H > 0.0 and np.isfinite(H)):
            st = ST_BADK
        if st == ST_OK:
            R = float(rows[4][oa]) + float(cols[4][ob])
            if not np.isfinite(R):
                st = ST_NUMERIC
        if st == ST_OK:
            Rp = max(R, 0.0)
            st, reach, g0, fl, mg = window_search(_pair_g(rows, cols, oa, ob, sa, sb, t, mu, Rp, nsigma), H, levels)
        if st == ST_OK:
            lo, hi = max(sa[0], sb[0]), min(sa[1], sb[1])
            out[n] = (max(reach[0], reach[1]), max(t - reach[0], lo), min(t + reach[1], hi), reach[0], reach[1], g0)
            flags[n], margin[n] = fl, mg
        status[n] = st
    return out, flags, status, margin
