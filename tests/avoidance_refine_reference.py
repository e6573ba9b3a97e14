"""numpy restatement of the iterated avoidance (include/mpcx.h: mpcx_avoidance_refine), built on avoidance_joint_reference: the joint
problem with a reference thrust, a terminal right-hand side and a warm start, and the loop around it -- fly the changed thrust with
the CPU oracle's propagation, look at the listed pairs again with conjunction_reference's screen, linearise with the oracle's
discretisation, solve again.  Uniform node counts only (ns = None).  Test infrastructure: the product never imports it."""
import numpy as np

import avoidance_joint_reference as J
import collision_reference as C
import conjunction_reference as CJ

ST_OK = 0


def solve_qp(D, uref, T, a, b, scale, umax=np.inf, trhs=None, z0=None, tol=J.DEFAULT_TOL, max_iter=J.DEFAULT_MAX_ITER):
    """avoidance_joint_reference.solve_qp with the three inputs of the refinement: minimise 1/2 sum_m D_m |du_m|^2 subject to
    sum_m T_m du_m = trhs (None: 0), sum_m a_p,m . du_m >= b_p (b is the row's right-hand side as solved: the caller has added
    sum_m a_p,m . (U_m - uref_m)), |uref_m + du_m| <= umax, from z0 = (y (6,), lambda * scale (r,)) (None: 0).
    -> solve_qp's dict plus z = (y, lambda * scale), the warm start of the next solve."""
    n, r = D.shape[0], a.shape[0]
    ne = 0 if T is None else 6
    Afull = np.concatenate(([T] if ne else []) + [a / scale]) if (ne or r) else np.zeros((0, 3, n))
    bh = b / scale
    nz = ne + r
    rt = np.zeros(ne) if trhs is None or not ne else np.asarray(trhs, dtype=np.float64)
    z = np.zeros(nz)
    if z0 is not None:
        z = np.concatenate([z0[0][:ne], z0[1]]).astype(np.float64)
    cs = np.array([((Afull[ne + p] * Afull[ne + p]).sum(axis=0) / D).sum() for p in range(r)])
    nan = dict(status=J.ST_MAXITER, du=np.full((3, n), np.nan), y=np.full(6, np.nan), lam=np.full(r, np.nan), iters=0, residual=np.nan,
               active=np.zeros(r, bool), onball=np.zeros(n, bool), z=None)
    if np.isfinite(umax):
        an = np.sqrt((a * a).sum(axis=1))
        for p in range(r):
            if (umax * an[p] - (a[p] * uref).sum(axis=0)).sum() < b[p]:
                return dict(nan, status=J.ST_INFEASIBLE)

    def evaluate(z):
        v = np.einsum("i,icm->cm", z, Afull)
        pp, Jm, out = J.project(uref + v / D, umax)
        du = pp - uref
        res = np.einsum("icm,cm->i", Afull, du)
        s = res[ne:] - bh
        F = np.concatenate([res[:ne] - rt, np.minimum(cs * z[ne:], s)])
        return du, Jm, out, s, F, (np.abs(F).max() if nz else 0.0)

    du, Jm, out, s, F, mF = evaluate(z)
    it = 0
    while True:
        if not np.isfinite(mF):
            return dict(nan, iters=it)
        act = np.concatenate([np.ones(ne, bool), cs * z[ne:] > s])
        if mF <= tol and not z[~act].any() and (z[ne:] >= 0.0).all():
            break
        if it == max_iter:
            return dict(nan, iters=it)
        H = np.einsum("iam,mab,jbm->ij", Afull, Jm / D[:, None, None], Afull)
        G = np.where(np.outer(act, act), H, 0.0) + np.diag((~act).astype(float))
        zi = np.where(act, 0.0, z)
        rhs = np.where(act, -F + H @ zi, -z)
        Lc = np.zeros((nz, nz))
        for j in range(nz):
            d = G[j, j] - Lc[j, :j] @ Lc[j, :j]
            if not d > J.PIVOT_REL * G[j, j]:
                return dict(nan, status=J.ST_SINGULAR, iters=it)
            Lc[j, j] = np.sqrt(d)
            Lc[j + 1:, j] = (G[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
        dz = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))
        t, ok = 1.0, False
        for _ in range(J.LINE_SEARCH):
            zn = z + t * dz
            cand = evaluate(zn)
            if cand[5] < mF or cand[5] <= tol:
                ok = True
                break
            t *= 0.5
        it += 1
        if not ok:
            return dict(nan, iters=it)
        z = zn
        du, Jm, out, s, F, mF = cand
    y = np.zeros(6)
    y[:ne] = z[:ne]
    return dict(status=ST_OK, du=du, y=y, lam=z[ne:] / scale, iters=it, residual=mF, active=z[ne:] > 0.0, onball=out, z=(y, z[ne:].copy()))


def rescreen(pairs, rows, cat, M, T0, T1):
    """mpcx_conjunction_pairs_traj restated from conjunction_reference: the listed pairs' closest approach on linspace(T0, T1, M)
    -> out (n, 4) rows (i, j, distance, time), (+inf, NaN) for a pair without a valid interval.  With a catalogue the pair (i, j) is
    the pair (i, S + j) of the union, as the header states."""
    Y, units, span, ns = rows
    S = Y.shape[0]
    eph, _ = CJ.ephemeris(Y, units, span, M, T0, T1, ns)
    if cat is not None:
        ceph, _ = CJ.ephemeris(cat[0], cat[1], cat[2], M, T0, T1, cat[3])
        eph = np.concatenate([eph, ceph])
    lo, hi, q, tq, _ = CJ.pair_minima(eph, T0, T1)
    out = np.array(pairs, dtype=np.float64)
    for r, (fi, fj) in enumerate(out[:, :2]):
        i, j = int(fi), int(fj) + (S if cat is not None else 0)
        at = np.flatnonzero((lo == min(i, j)) & (hi == max(i, j)))[0]
        out[r, 2] = np.sqrt(q[at]) if q[at] < np.inf else np.inf
        out[r, 3] = tq[at]
    return out


def linearise(Y, U, tf, consts, flags=0, max_step=1e-2):
    """the oracle's discretisation of every satellite about (Y, U) -> (A (S, K-1, 7, 7), B_kn, B_kp (S, K-1, 7, 3))"""
    import oracle_lib as O
    ds = [O.discretize(Y[s], U[s], float(tf[s]), consts[s], flags, max_step) for s in range(len(Y))]
    assert all(d["status"] == 0 for d in ds)
    return tuple(np.stack([d[k] for d in ds]) for k in ("A", "Bn", "Bp"))


def fly(y0, U, tf, consts, K, flags=0, max_step=1e-3):
    """the oracle's propagation from y0 (7,) under the thrust table U (3, K) played over the whole of tf, sampled at the K nodes"""
    import oracle_lib as O
    ctrl = O.make_ctrl(O.CTRL_SEQUENCE, useq=U, end_tau=1.0)
    x, rc, _ = O.propagate(y0, float(tf), consts, ctrl, K, flags, max_step)
    return x, rc


def refine(pairs, mover, rows, U, consts, target, grid, rounds, cat=None, P=None, u_max=None, hold_terminal=True, tol=J.DEFAULT_TOL,
           max_iter=J.DEFAULT_MAX_ITER, flags=0, max_step=1e-2, prop_max_step=1e-3, mu=C.MU_EARTH):
    """The whole call for rows = (Y (S, 7, K), units, span, None).  max_iter: one number, or one per solve (passes 0 .. rounds) -- how a
    test makes a later solve fail.  -> dict(du, sat_out, row_out, sat_status, row_status, rows, tsens, Y_flown, pairs_flown, d0_history,
    tca_history, terminal_history, rounds_done, rhs_rows, rhs_term, cost_history (rounds + 1, S): the effort of every pass's solve,
    NaN where there was none)"""
    Y, units, span, ns = rows
    assert ns is None
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 4)
    S, _, K = Y.shape
    n = len(pairs)
    M, T0, T1 = grid
    tf = (span[:, 1] - span[:, 0]) / units[:, 1]
    iters = [max_iter] * (rounds + 1) if np.ndim(max_iter) == 0 else list(max_iter)
    o = dict(du=np.zeros((S, 3, K)), sat_out=np.zeros((S, J.NAJ)), row_out=np.full((n, J.NAR), np.nan), sat_status=np.zeros(S, dtype=np.int32),
             row_status=np.zeros(n, dtype=np.int32), rows=None, tsens=np.zeros((S, 6, 3, K)), Y_flown=Y.copy(), pairs_flown=pairs.copy(),
             d0_history=np.zeros((rounds + 2, n)), tca_history=np.zeros((rounds + 2, n)), terminal_history=np.zeros((rounds + 2, S)),
             rounds_done=np.full(S, -1, dtype=np.int32), rhs_rows=np.full(n, np.nan), rhs_term=np.zeros((S, 6)),
             cost_history=np.full((rounds + 1, S), np.nan))
    z = [None] * S
    flies = np.zeros(S, bool)
    skip = np.zeros(S, bool)
    Yt, Ut, pt = Y, U, pairs
    for t in range(rounds + 2):
        if t >= 1:
            Ut = np.where(flies[:, None, None], U + np.where(flies[:, None, None], o["du"], 0.0), U)
            Yt = Y.copy()
            for s in np.flatnonzero(flies):
                x, rc = fly(Y[s][:, 0], Ut[s], tf[s], consts[s], K, flags, prop_max_step)
                if rc != 0:
                    if not skip[s]:
                        skip[s] = True; o["sat_status"][s] = rc
                    continue
                Yt[s] = x
                o["terminal_history"][t, s] = np.abs(x[:6, -1] - Y[s][:6, -1]).max()
            pt = rescreen(pairs, (Yt, units, span, None), cat, M, T0, T1)
            o["Y_flown"], o["pairs_flown"] = Yt, pt
        stage = linearise(Yt, Ut, tf, consts, flags, max_step)
        A, Bn, Bp = stage
        enc = J.encounter_rows(pt, mover, (Yt, units, span, None), stage, target, P, cat, mu)
        o["d0_history"][t], o["tca_history"][t] = enc["d0"], pt[:, 3]
        if t == rounds + 1:
            break
        if t == 0:
            o["row_status"] = enc["status"].copy()
            o["row_out"][:, J.AR_D0] = enc["d0"]
        o["rows"] = enc["a"]
        for s in range(S):
            mine = np.flatnonzero(enc["owner"] == s)
            if (t == 0 and len(mine) == 0) or (t >= 1 and skip[s]):
                continue
            bad = [int(enc["status"][p]) for p in mine if enc["status"][p] != 0]
            st = bad[0] if bad else (J.ST_BADK if len(mine) > J.MAX_ROWS else ST_OK)
            res = None
            if st == ST_OK:
                D, w, c = J.effort_weights(Yt, units, span, None, s)
                Ts, trhs = None, None
                if hold_terminal:
                    Ts = J.terminal_sens(A[s], Bn[s], Bp[s], K, K)
                    o["tsens"][s] = Ts
                    if t >= 1:
                        trhs = np.einsum("icm,cm->i", Ts, o["du"][s]) - (Yt[s][:6, -1] - Y[s][:6, -1])
                um = np.inf if u_max is None else float(u_max[s])
                a = enc["a"][mine]
                b = enc["b"][mine] + np.einsum("pcm,cm->p", a, Ut[s] - U[s])
                res = solve_qp(D, U[s], Ts, a, b, target, um, trhs, z[s], tol, iters[t])
                st = res["status"]
                o["rhs_rows"][mine] = b
                o["rhs_term"][s] = 0.0 if trhs is None else trhs
            if st != ST_OK:
                o["sat_status"][s] = st
                if t == 0:
                    o["du"][s] = np.nan; o["sat_out"][s] = np.nan
                else:
                    skip[s] = True
                continue
            du = res["du"]
            z[s] = res["z"]
            o["du"][s] = du
            o["sat_status"][s] = ST_OK
            o["rounds_done"][s] = t
            da, ut = c * du, U[s] + du
            o["sat_out"][s] = (0.5 * (D * (du * du).sum(axis=0)).sum(), (w * np.sqrt((da * da).sum(axis=0))).sum(), np.sqrt((ut * ut).sum(axis=0)).max(),
                               len(mine), res["active"].sum(), res["onball"].sum(), res["iters"], res["residual"])
            o["cost_history"][t, s] = o["sat_out"][s, J.AJ_COST]
            dd = du - (Ut[s] - U[s])                                   # the change from the thrust the pass linearised about
            for i, p in enumerate(mine):
                g, W, mn = enc["g"][p], enc["W"][p], enc["mn"][p]
                x = np.array([mn, 0.0]) + np.array([(g[0] * dd).sum(), (g[1] * dd).sum()])
                o["row_out"][p] = (enc["d0"][p], enc["d0"][p] + (enc["a"][p] * dd).sum(), np.sqrt(x @ W @ x), res["lam"][i], -(g[2] * dd).sum() / enc["wn"][p])
                o["row_status"][p] = enc["status"][p]
        if t == 0:
            flies = (o["sat_status"] == ST_OK) & (o["sat_out"][:, J.AJ_ROWS] > 0)
            skip = ~flies
    return o
