"""numpy restatement of the window manoeuvre flown and corrected (include/mpcx.h: mpcx_avoidance_window_refine), built on
avoidance_window_reference: pass 0 is its avoidance_window; every later pass flies each row's own copy of the objects that move with
the CPU oracle's propagation, finds the row's time again with conjunction_track_reference, linearises with the oracle's
discretisation, chains the covariances with collision_reference, takes the window figure with avoidance_window_reference's rule and
solves for the total change from the given thrust by the header's search.  Rows are independent, so the loop runs row by row on a
constellation of the row's own one or two objects.  Test infrastructure: the product never imports it."""
import numpy as np

import avoidance_window_reference as AW
import collision_reference as C
import collision_window_reference as CW
import conjunction_track_reference as T

ST_OK, ST_SINGULAR, ST_MAXITER, ST_NUMERIC, ST_INFEASIBLE, ST_BADK = 0, AW.ST_SINGULAR, AW.ST_MAXITER, AW.ST_NUMERIC, AW.ST_INFEASIBLE, AW.ST_BADK


def fly(y0, U, tf, consts, nn, flags=0, max_step=1e-3):
    """the oracle's propagation from y0 (7,) under the thrust table U (3, nn) played over the whole of tf, sampled at the nn nodes"""
    import oracle_lib as O
    ctrl = O.make_ctrl(O.CTRL_SEQUENCE, useq=np.ascontiguousarray(U), end_tau=1.0)
    x, rc, _ = O.propagate(np.ascontiguousarray(y0), float(tf), consts, ctrl, int(nn), flags, max_step)
    return x, rc


def linearise(Y, U, tf, consts, ns=None, flags=0, max_step=1e-2):
    """the oracle's discretisation of every object about (Y, U) on its own nodes -> (A (S, K-1, 7, 7), B_kn, B_kp (S, K-1, 7, 3)), status
    (S,); records past an object's nodes are zero"""
    import oracle_lib as O
    S, _, K = Y.shape
    A, Bn, Bp, st = np.zeros((S, K - 1, 7, 7)), np.zeros((S, K - 1, 7, 3)), np.zeros((S, K - 1, 7, 3)), np.zeros(S, dtype=np.int32)
    for s in range(S):
        nn = K if ns is None else int(ns[s])
        d = O.discretize(np.ascontiguousarray(Y[s][:, :nn]), np.ascontiguousarray(U[s][:, :nn]), float(tf[s]), consts[s], flags, max_step)
        st[s] = d["status"]
        if st[s] == 0:
            A[s, :nn - 1], Bn[s, :nn - 1], Bp[s, :nn - 1] = d["A"], d["Bn"], d["Bp"]
    return (A, Bn, Bp), st


def shifted_window(e, rows, cols, movers, panels, mu=CW.MU_EARTH):
    """Q_t(alpha) of a row: movers = [(object, sgn, X_e (nn, 7), X_prev (nn, 7))] -> a function alpha -> START + ENTRIES of the window
    rule at the means moved by sgn (alpha X_e - X_prev), with the unmoved frames and covariances (avoidance_window_reference.
    shifted_window with two responses)"""
    def mean_shift(tau, which):
        dd, dw = np.zeros((3, len(tau))), np.zeros((3, len(tau)))
        for o, sgn, xe, xp in movers:
            dx = xe if which == 0 else xp
            k, bp, bv = AW.bases(rows, o, tau)
            x0, x1 = dx[k].T, dx[k + 1].T
            dd = dd + sgn * (bp[0] * x0[0:3] + bp[1] * x0[3:6] + bp[2] * x1[0:3] + bp[3] * x1[3:6])
            dw = dw + sgn * (bv[0] * x0[0:3] + bv[1] * x0[3:6] + bv[2] * x1[0:3] + bv[3] * x1[3:6])
        return dd, dw

    ta, tb, R = e["ta"], e["tb"], e["R"]
    hp = (tb - ta) / panels
    nodes = []
    for p in list(range(panels)) + [None]:
        tau = np.array([ta]) if p is None else (ta + p * hp) + (0.5 * hp) * (1.0 + CW.GL_X)
        nodes.append(CW.relative_state(rows, cols, e["oa"], e["ob"], tau, mu) + mean_shift(tau, 0) + mean_shift(tau, 1))

    def Q(alpha):
        entries = 0.0
        for d, w, A, B, D, de, we, dp, wp in nodes[:-1]:
            _, rate = AW.rate_and_gradient(R, d + (alpha * de - dp), w + (alpha * we - wp), A, B, D, wf=w, grad=False)
            entries = entries + CW.butterfly_sum(((0.5 * hp) * CW.GL_W) * rate)
        d, w, A, _, _, de, we, dp, wp = nodes[-1]
        _, start = AW.ball_and_gradient(R, (d + (alpha * de - dp))[:, 0], w[:, 0], A[:, :, 0], grad=False)
        return start + entries
    return Q


def step_length(Q, Qt, c0, Gam, target_p, tol, max_eval):
    """The header's search of a pass t >= 1 -> (status, alpha, Q(alpha), evaluations)"""
    f0 = np.log(Qt / target_p)
    with np.errstate(all="ignore"):
        alpha = (c0 + Qt * f0) / Gam
    if not alpha > 0.0 or not np.isfinite(alpha):
        return ST_NUMERIC, np.nan, np.nan, 0
    lo = flo = hi = fhi = 0.0
    evals, way = 0, 0
    while True:                                                          # bracketing
        if evals == max_eval:
            return ST_INFEASIBLE, np.nan, np.nan, evals
        Q1 = Q(alpha); evals += 1
        if not Q1 >= 0.0 or not np.isfinite(Q1) or not np.isfinite(alpha) or not alpha > 0.0:
            return ST_NUMERIC, np.nan, np.nan, evals
        with np.errstate(divide="ignore"):
            f = np.log(Q1 / target_p)
        if abs(f) <= tol:
            return ST_OK, alpha, Q1, evals
        if f > 0.0:
            lo, flo = alpha, f
            if way < 0:
                break
            way = 1
            alpha = 2.0 * alpha
        else:
            hi, fhi = alpha, f
            if way > 0:
                break
            way = -1
            alpha = 0.5 * alpha
    side = 0
    while True:                                                          # closing: avoidance_window_reference.step_length's
        if evals == max_eval:
            return ST_MAXITER, np.nan, np.nan, evals
        with np.errstate(all="ignore"):
            alpha = lo + (hi - lo) * (flo / (flo - fhi))
        if not (alpha > lo and alpha < hi):
            alpha = 0.5 * (lo + hi)
        Q1 = Q(alpha); evals += 1
        if not Q1 >= 0.0 or not np.isfinite(Q1):
            return ST_NUMERIC, np.nan, np.nan, evals
        with np.errstate(divide="ignore"):
            f = np.log(Q1 / target_p)
        if abs(f) <= tol:
            return ST_OK, alpha, Q1, evals
        if f > 0.0:
            lo, flo = alpha, f
            if side == 1:
                fhi = 0.5 * fhi
            side = 1
        else:
            hi, fhi = alpha, f
            if side == -1:
                flo = 0.5 * flo
            side = -1


def refine(pairs, rows, U, consts, target_p, half_window, panels, rounds, cols=None, who="i", track=None, max_shift=None, recov=False, q=None,
           tol=1e-6, max_eval=40, flags=0, max_step=1e-2, prop_max_step=1e-3, mu=CW.MU_EARTH, stage0=None):
    """The whole call for rows, cols = (Y, units, span, P, radius, ns) as avoidance_window_reference takes them.  max_eval: one
    number, or one per solve (passes 0 .. rounds) -- how a test makes a later solve fail.  stage0: the linearisation of the given plan
    (None: the oracle's).  -> dict(out, du, status, rounds_done, Y_flown (n, NS, 7, K), P_flown, p_history, t_history (rounds + 2, n),
    p_predicted, evals (rounds + 1, n): the evaluations of every pass's solve)"""
    Y, units, span, P, radius, ns = rows
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 4)
    S, _, K = Y.shape
    n = len(pairs)
    NS = 1 if cols is not None else 2
    whoi = AW.WHO[who] if isinstance(who, str) else who
    moves = (whoi != 1, NS == 2 and whoi != 0)
    half = np.broadcast_to(np.asarray(half_window, dtype=np.float64), (n,))
    evs = [max_eval] * (rounds + 1) if np.ndim(max_eval) == 0 else list(max_eval)
    tf = (span[:, 1] - span[:, 0]) / units[:, 1]
    # ---- pass 0
    if stage0 is None:
        stage0, dst = linearise(np.nan_to_num(Y, nan=1.0), U, tf, consts, ns, flags, max_step)
    else:
        dst = None
    grads = AW.row_gradients(pairs, rows, half, panels, cols, mu)
    sens, Es, st = AW.window_sensitivity(grads, rows, stage0, who, cols, disc_status=dst)
    out, du, status, _ = AW.avoidance_window(grads, sens, Es, st, rows, stage0, target_p, tol, evs[0], panels, who, cols, mu)
    o = dict(out=out, du=du, status=status, rounds_done=np.full(n, -1, dtype=np.int32), Y_flown=np.zeros((n, NS, 7, K)),
             P_flown=np.zeros((n, NS, K, 6, 6)) if recov else None, p_history=np.full((rounds + 2, n), np.nan),
             t_history=np.tile(pairs[:, 3], (rounds + 2, 1)), p_predicted=np.full((rounds + 1, n), np.nan), evals=np.zeros((rounds + 1, n)),
             sens=sens.copy())
    o["p_history"][:] = out[:, AW.P0]
    o["evals"][0] = out[:, AW.EVALS]
    for r in range(n):
        good = status[r] == ST_OK
        obj = [int(pairs[r, sl]) if good else 0 for sl in range(NS)]
        o["Y_flown"][r] = Y[obj]
        if recov:
            o["P_flown"][r] = P[obj]
        if not (good and out[r, AW.ALPHA] > 0.0):
            continue
        o["rounds_done"][r] = 0
        o["p_predicted"][0, r] = out[r, AW.P1]
        # ---- the row's own constellation
        nsv = None if ns is None else np.asarray(ns)[obj]
        given = pairs[r].copy()
        given[0] = 0.0
        if NS == 2:
            given[1] = 1.0
        track_row = given.copy()
        if NS == 2 and pairs[r, 0] == pairs[r, 1]:
            track_row[:2] = np.nan
        frozen = False
        for t in range(1, rounds + 2):
            Ut = U[obj] + du[r]
            Yt, Pt = Y[obj].copy(), P[obj].copy()
            for sl in range(NS):
                if not moves[sl]:
                    continue
                nn = K if nsv is None else int(nsv[sl])
                x, rc = fly(Y[obj[sl]][:, 0], Ut[sl][:, :nn], tf[obj[sl]], consts[obj[sl]], nn, flags, prop_max_step)
                if rc != 0:
                    if not frozen:
                        frozen, status[r] = True, rc
                    continue
                Yt[sl] = 0.0
                Yt[sl][:, :nn] = x
            row_t = given.copy()
            if track is not None:
                M, T0, T1 = track
                cat4 = None if cols is None else (cols[0], cols[1], cols[2], cols[5])
                found = T.rescreen_tracked(track_row[None], (Yt, units[obj], span[obj], nsv), cat4, M, T0, T1, max_shift)[0]
                row_t[2], row_t[3] = found[2], found[3]
                if not np.isfinite(found[3]):
                    row_t[3] = np.nan
                    if not frozen:
                        frozen, status[r] = True, ST_BADK
            o["t_history"][t, r] = row_t[3]
            solve = t <= rounds
            stage = dstat = None
            if solve or recov:
                stage, dstat = linearise(np.nan_to_num(Yt, nan=1.0), Ut, tf[obj], consts[obj], nsv, flags, max_step)
            if recov:
                Pc, cst = C.covariance_chain(stage[0], units[obj], span[obj], P[obj][:, 0], None if q is None else np.broadcast_to(q, (S,))[obj], nsv, dstat)
                for sl in range(NS):
                    if moves[sl]:
                        Pt[sl] = Pc[sl]
                        if cst[sl] != 0 and not frozen:
                            frozen, status[r] = True, int(cst[sl])
            vrows = (Yt, units[obj], span[obj], Pt, radius[obj], nsv)
            o["Y_flown"][r] = Yt
            if recov:
                o["P_flown"][r] = Pt
            g = AW.row_gradients(row_t[None], vrows, half[r:r + 1], panels, cols, mu)
            e = g[0]
            if e["st"] != ST_OK:
                o["p_history"][t, r] = np.nan
                if not frozen:
                    frozen, status[r] = True, e["st"]
                continue
            Qt = (e["start"] + e["entries"]) if e["R"] > 0.0 else 0.0
            o["p_history"][t, r] = Qt
            if not solve or frozen:
                continue
            st_t = ST_OK
            sens_t, _, wst = AW.window_sensitivity(g, vrows, stage, who, cols, disc_status=dstat)
            o["sens"][r] = sens_t[0]
            if wst[0] != ST_OK:
                st_t = int(wst[0])
            elif not (Qt > 0.0 and np.isfinite(Qt)):
                st_t = ST_NUMERIC
            evals = 0
            if st_t == ST_OK and abs(np.log(Qt / target_p)) <= tol:
                out[r, AW.P1] = Qt
                o["rounds_done"][r] = t
                o["p_predicted"][t, r] = Qt
                continue
            if st_t == ST_OK:
                objs = (0, 1) if NS == 2 else (0, e["ob"])
                e1, Gam, dv, um = AW.direction(vrows, sens_t[0], objs, moves, K)
                s = 0.0
                for sl in range(NS):
                    for m in range(K):
                        for c in range(3):
                            s = s + sens_t[0, sl, c, m] * du[r, sl, c, m]
                c0 = -s
                if not Gam > 0.0 or not np.isfinite(Gam):
                    st_t = ST_SINGULAR
            if st_t == ST_OK:
                A, Bn, Bp = stage
                movers = []
                for sl in range(NS):
                    if moves[sl]:
                        nn = K if nsv is None else int(nsv[sl])
                        movers.append((sl, 1.0 if sl else -1.0, AW.response(A[sl], Bn[sl], Bp[sl], e1[sl], nn),
                                       AW.response(A[sl], Bn[sl], Bp[sl], du[r, sl], nn)))
                Q = shifted_window(e, vrows, vrows if cols is None else cols, movers, panels, mu)
                st_t, alpha, Q1, evals = step_length(Q, Qt, c0, Gam, target_p, tol, evs[t])
            out[r, AW.EVALS] += evals
            o["evals"][t, r] = evals
            if st_t != ST_OK:
                frozen, status[r] = True, st_t
                continue
            du[r] = alpha * e1
            out[r, AW.P1], out[r, AW.ALPHA], out[r, AW.DQ_LINEAR] = Q1, alpha, c0 - alpha * Gam
            out[r, AW.DV_I], out[r, AW.DV_J], out[r, AW.UMAX_I], out[r, AW.UMAX_J] = alpha * dv[0], alpha * dv[1], alpha * um[0], alpha * um[1]
            o["rounds_done"][r] = t
            o["p_predicted"][t, r] = Q1
    return o
