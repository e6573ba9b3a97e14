"""numpy restatement of the joint avoidance step (include/mpcx.h: mpcx_avoidance_joint), built on avoidance_reference: the encounter
rows a_p and their right-hand sides, the terminal sensitivities T_m, and the strictly convex problem per manoeuvring satellite, solved
by the header's semismooth Newton / primal-dual active-set iteration.  Test infrastructure: the product never imports it."""
import numpy as np

import avoidance_reference as AR
import collision_reference as C

ST_OK, ST_SINGULAR, ST_MAXITER, ST_NUMERIC, ST_INFEASIBLE, ST_BADK = 0, 4, 5, 6, 8, 9
MAX_ROWS = 8
NAJ = 8
AJ_COST, AJ_DV, AJ_UMAX, AJ_ROWS, AJ_ACTIVE, AJ_ONBALL, AJ_ITERS, AJ_RESIDUAL = range(NAJ)
NAR = 5
AR_D0, AR_MARGIN, AR_DIST, AR_LAMBDA, AR_DT = range(NAR)
PIVOT_REL = 1e-12                  # a Cholesky pivot at or below this share of its own diagonal entry: not positive definite
LINE_SEARCH = 30                   # halvings of a Newton step
DEFAULT_TOL, DEFAULT_MAX_ITER = 1e-10, 50


def sweep_rows(A, Bn, Bp, k, seed_hi, seed_lo, K):
    """avoidance_reference.sweep for any number of rows: seed_hi, seed_lo (R, 7) -> g (R, 3, K)"""
    lam = {k + 1: seed_hi}
    for m in range(k, -1, -1):
        lam[m] = AR.ordered(lam[m + 1], A[m])
        if m == k:
            lam[m] = lam[m] + seed_lo
    g = np.zeros((seed_hi.shape[0], 3, K))
    for m in range(0, k + 2):
        if m <= k and m >= 1:
            g[:, :, m] = AR.ordered(lam[m + 1], Bn[m]) + AR.ordered(lam[m], Bp[m - 1])
        elif m <= k:
            g[:, :, m] = AR.ordered(lam[m + 1], Bn[m])
        else:
            g[:, :, m] = AR.ordered(lam[m], Bp[m - 1])
    return g


def terminal_sens(A, Bn, Bp, nn, K):
    """T (6, 3, K): the derivative of the last node's normalised position and velocity with respect to every thrust node -- the
    adjoint recursion seeded with [I_6 | 0] at node nn - 1 and swept over the whole horizon"""
    hi = np.hstack([np.eye(6), np.zeros((6, 1))])
    return sweep_rows(A, Bn, Bp, nn - 2, hi, np.zeros((6, 7)), K)


def effort_weights(Y, units, span, ns, o):
    """D_m = w_m c_m^2 (nn,), w_m, c_m of satellite o"""
    K = Y.shape[2]
    nn = K if ns is None else int(ns[o])
    L, Tu = units[o]
    hn = (span[o, 1] - span[o, 0]) / (nn - 1)
    w = AR.node_weights(hn, nn, K)[:nn]
    c = (L / (Tu * Tu)) / Y[o, 6, :nn]
    return w * c * c, w, c


def project(p, umax):
    """p (3, n) onto the ball of radius umax, the Jacobians J (n, 3, 3), and which columns were outside"""
    n = p.shape[1]
    pn = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])
    out = pn > umax
    J = np.broadcast_to(np.eye(3), (n, 3, 3)).copy()
    pp = p.copy()
    if out.any():
        s = umax / pn[out]
        pp[:, out] = p[:, out] * s
        ph = p[:, out] / pn[out]
        J[out] = s[:, None, None] * (np.eye(3)[None] - np.einsum("am,bm->mab", ph, ph))
    return pp, J, out


def solve_qp(D, ubar, T, a, b, scale, umax=np.inf, tol=DEFAULT_TOL, max_iter=DEFAULT_MAX_ITER):
    """minimise 1/2 sum_m D_m |du_m|^2 subject to sum_m T_m du_m = 0 (T (6, 3, n) or None), sum_m a_p,m . du_m >= b_p (a (r, 3, n)),
    |ubar_m + du_m| <= umax.  The encounter rows are taken in units of `scale` (the target) and a row's multiplier is weighed by the
    row's own authority c_p = sum_m |a_p,m / scale|^2 / D_m: F = [T du; min(c lam, (a du - b) / scale)].
    -> dict(status, du (3, n), y (6,), lam (r,) in the rows' own units, iters, residual, active (r,) bool, onball (n,) bool)"""
    n = D.shape[0]
    r = a.shape[0]
    ne = 0 if T is None else 6
    Afull = np.concatenate(([T] if ne else []) + [a / scale]) if (ne or r) else np.zeros((0, 3, n))
    bh = b / scale
    nz = ne + r
    z = np.zeros(nz)
    cs = np.array([((Afull[ne + p] * Afull[ne + p]).sum(axis=0) / D).sum() for p in range(r)])
    nan = dict(status=ST_MAXITER, du=np.full((3, n), np.nan), y=np.full(6, np.nan), lam=np.full(r, np.nan), iters=0, residual=np.nan,
               active=np.zeros(r, bool), onball=np.zeros(n, bool))
    if np.isfinite(umax):
        an = np.sqrt((a * a).sum(axis=1))
        for p in range(r):
            if (umax * an[p] - (a[p] * ubar).sum(axis=0)).sum() < b[p]:
                return dict(nan, status=ST_INFEASIBLE)

    def evaluate(z):
        v = np.einsum("i,icm->cm", z, Afull)
        pp, J, out = project(ubar + v / D, umax)
        du = pp - ubar
        res = np.einsum("icm,cm->i", Afull, du)
        s = res[ne:] - bh
        F = np.concatenate([res[:ne], np.minimum(cs * z[ne:], s)])
        return du, J, out, s, F, (np.abs(F).max() if nz else 0.0)

    du, J, out, s, F, mF = evaluate(z)
    it = 0
    while True:
        if not np.isfinite(mF):
            return dict(nan, iters=it)
        act = np.concatenate([np.ones(ne, bool), cs * z[ne:] > s])
        if mF <= tol and not z[~act].any() and (z[ne:] >= 0.0).all():          # (an inactive row's multiplier is exactly 0)
            break
        if it == max_iter:
            return dict(nan, iters=it)
        H = np.einsum("iam,mab,jbm->ij", Afull, J / D[:, None, None], Afull)
        G = np.where(np.outer(act, act), H, 0.0) + np.diag((~act).astype(float))
        zi = np.where(act, 0.0, z)
        rhs = np.where(act, -F + H @ zi, -z)
        Lc = np.zeros((nz, nz))
        for j in range(nz):                                  # Cholesky with the pivot rule
            d = G[j, j] - Lc[j, :j] @ Lc[j, :j]
            if not d > PIVOT_REL * G[j, j]:
                return dict(nan, status=ST_SINGULAR, iters=it)
            Lc[j, j] = np.sqrt(d)
            Lc[j + 1:, j] = (G[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
        dz = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rhs))
        t, ok = 1.0, False
        for _ in range(LINE_SEARCH):
            zn = z + t * dz                                  # (t = 1 takes an inactive row's multiplier to 0 exactly)
            cand = evaluate(zn)
            if cand[5] < mF or cand[5] <= tol:
                ok = True
                break
            t *= 0.5
        it += 1
        if not ok:
            return dict(nan, iters=it)
        z = zn
        du, J, out, s, F, mF = cand
    return dict(status=ST_OK, du=du, y=z[:ne] if ne else np.zeros(6), lam=z[ne:] / scale, iters=it, residual=mF, active=z[ne:] > 0.0, onball=out)


def encounter_rows(pairs, mover, rows, stage, target, P=None, cat=None, mu=C.MU_EARTH, disc_status=None):
    """For every listed pair the row of the joint problem.  pairs (n, 4); mover (n,) 0 = object i moves, 1 = object j (None: all 0);
    rows = (Y, units, span, ns); stage = (A, B_kn, B_kp); cat = (Y, units, span, ns, P or None) or None.
    -> dict(a (n, 3, K), g (n, 3, 3, K), d0, b, q (n, 2), W (n, 2, 2), mn, wn, owner (n,) int (-1: no such satellite), status (n,))"""
    pairs = np.asarray(pairs, dtype=np.float64).reshape(-1, 4)
    Y, units, span, ns = rows
    A, Bn, Bp = stage
    S, _, K = Y.shape
    n = len(pairs)
    mover = np.zeros(n, dtype=np.int32) if mover is None else np.asarray(mover, dtype=np.int32)
    zP = lambda y: np.zeros((y.shape[0], y.shape[2], 6, 6))
    side_r = (Y, units, span, zP(Y) if P is None else P, np.zeros(S), ns)
    side_c = side_r if cat is None else (cat[0], cat[1], cat[2], zP(cat[0]) if cat[4] is None else cat[4], np.zeros(len(cat[0])), cat[3])
    o = dict(a=np.full((n, 3, K), np.nan), g=np.full((n, 3, 3, K), np.nan), d0=np.full(n, np.nan), b=np.full(n, np.nan), q=np.full((n, 2), np.nan),
             W=np.full((n, 2, 2), np.nan), mn=np.full(n, np.nan), wn=np.full(n, np.nan), owner=np.full(n, -1), status=np.zeros(n, dtype=np.int32))
    for r, (fi, fj, _, t) in enumerate(pairs):
        fm = fj if mover[r] else fi
        if fm >= 0.0 and fm < S:
            o["owner"][r] = int(fm)
        st, pa, va, Ca, _ = C.state_and_cov_at(side_r, fi, t, mu)
        if st == ST_OK:
            st, pb, vb, Cb, _ = C.state_and_cov_at(side_c, fj, t, mu)
        if st == ST_OK:
            s = int(fm)
            with np.errstate(all="ignore"):
                tf = (span[s, 1] - span[s, 0]) / np.float64(units[s, 1])
            if not tf > 0.0 or not np.isfinite(tf):
                st = ST_BADK
            elif disc_status is not None and disc_status[s] != 0:
                st = int(disc_status[s])
        fr = AR.frame(pb - pa, vb - va) if st == ST_OK else None
        if st == ST_OK and fr is None:
            st = ST_NUMERIC
        W = np.eye(2)
        if st == ST_OK:
            ew, e1, e2, mn, wn = fr
            if P is not None:
                E2 = np.stack([e1, e2], axis=1)
                C2 = E2.T @ (Ca + Cb) @ E2
                c11, c12, c22 = C2[0, 0], 0.5 * (C2[0, 1] + C2[1, 0]), C2[1, 1]
                with np.errstate(all="ignore"):
                    l1 = 0.5 * (c11 + c22 + np.sqrt((c11 - c22) ** 2 + 4.0 * c12 * c12))
                    l2 = (c11 * c22 - c12 * c12) / l1
                if not l2 > 0.0 or not np.isfinite(l2) or not np.isfinite(l1):
                    st = ST_NUMERIC
                else:
                    W = np.array([[c22, -c12], [-c12, c11]]) / (c11 * c22 - c12 * c12)
        if st == ST_OK:
            L, Tu = units[s]
            k, basis, hn, nn = AR.node_of(Y, units, span, ns, s, t)
            htau = ((span[s, 1] - span[s, 0]) / Tu) / (nn - 1)
            hi, lo = AR.seeds((1.0 if mover[r] else -1.0) * np.stack([e1, e2, ew]), L, htau, basis)
            g = AR.sweep(A[s], Bn[s], Bp[s], k, hi, lo, K)
            sq = np.sqrt(W[0, 0])
            q = np.array([W[0, 0] / sq, W[0, 1] / sq])
            o["g"][r] = g
            o["a"][r] = g[0] if P is None else q[0] * g[0] + q[1] * g[1]
            o["d0"][r] = mn * sq
            o["b"][r] = target - mn * sq
            o["q"][r], o["W"][r], o["mn"][r], o["wn"][r] = q, W, mn, wn
        o["status"][r] = st
    return o


def avoidance_joint(pairs, mover, rows, U, stage, target, P=None, cat=None, u_max=None, hold_terminal=True, tol=DEFAULT_TOL,
                    max_iter=DEFAULT_MAX_ITER, mu=C.MU_EARTH, a_rows=None, T=None):
    """The whole call -> dict(du (S, 3, K), sat_out (S, NAJ), row_out (n, NAR), rows (n, 3, K), tsens (S, 6, 3, K), sat_status (S,),
    row_status (n,), y (S, 6)).  a_rows (n, 3, K), T (S, 6, 3, K): use these (the device's own) instead of the restated ones."""
    Y, units, span, ns = rows
    A, Bn, Bp = stage
    S, _, K = Y.shape
    enc = encounter_rows(pairs, mover, rows, stage, target, P, cat, mu)
    n = len(enc["status"])
    a_all = enc["a"] if a_rows is None else a_rows
    out = dict(du=np.zeros((S, 3, K)), sat_out=np.zeros((S, NAJ)), row_out=np.full((n, NAR), np.nan), rows=a_all, tsens=np.zeros((S, 6, 3, K)),
               sat_status=np.zeros(S, dtype=np.int32), row_status=enc["status"], y=np.zeros((S, 6)))
    out["row_out"][:, AR_D0] = enc["d0"]
    for s in range(S):
        mine = np.flatnonzero(enc["owner"] == s)
        if len(mine) == 0:
            continue
        bad = [int(enc["status"][p]) for p in mine if enc["status"][p] != 0]
        st = bad[0] if bad else (ST_BADK if len(mine) > MAX_ROWS else ST_OK)
        res = None
        if st == ST_OK:
            nn = K if ns is None else int(ns[s])
            D, w, c = effort_weights(Y, units, span, ns, s)
            Ts = None
            if hold_terminal:
                Ts = terminal_sens(A[s], Bn[s], Bp[s], nn, K) if T is None else T[s]
                out["tsens"][s] = Ts
                Ts = Ts[:, :, :nn]
            um = np.inf if u_max is None else float(u_max[s])
            res = solve_qp(D, U[s][:, :nn], Ts, a_all[mine][:, :, :nn], enc["b"][mine], target, um, tol, max_iter)
            st = res["status"]
        out["sat_status"][s] = st
        if st != ST_OK:
            out["du"][s] = np.nan; out["sat_out"][s] = np.nan
            continue
        du = res["du"]
        out["du"][s, :, :nn] = du
        out["y"][s] = res["y"]
        da = c * du
        ut = U[s][:, :nn] + du
        out["sat_out"][s] = (0.5 * (D * (du * du).sum(axis=0)).sum(), (w * np.sqrt((da * da).sum(axis=0))).sum(), np.sqrt((ut * ut).sum(axis=0)).max(),
                             len(mine), res["active"].sum(), res["onball"].sum(), res["iters"], res["residual"])
        for i, p in enumerate(mine):
            g, W, mn = enc["g"][p][:, :, :nn], enc["W"][p], enc["mn"][p]
            dm = np.array([(g[0] * du).sum(), (g[1] * du).sum()])
            x = np.array([mn, 0.0]) + dm
            out["row_out"][p] = (enc["d0"][p], enc["d0"][p] + (a_all[p][:, :nn] * du).sum(), np.sqrt(x @ W @ x), res["lam"][i],
                                 -(g[2] * du).sum() / enc["wn"][p])
    return out


def random_problem(K, r, hold, ball, seed):
    """A synthetic problem for the QP alone: D, ubar, T or None, a, b, umax; feasible by construction when the ball is off (b is what a
    random du that holds the terminal rows reaches, minus a slack), never trivial (row 0 asks for 0.9 of what that du reaches there, a
    positive amount: du = 0 violates it, so at least one row is active at the solution), ball: umax = 0.8 x the largest
    |ubar + du| of the solution without a ball."""
    rng = np.random.default_rng(seed)
    D = rng.uniform(0.5, 2.0, K)
    ubar = 0.02 * rng.standard_normal((3, K))
    T = rng.standard_normal((6, 3, K)) * np.linspace(1.0, 0.1, K) if hold else None
    a = rng.standard_normal((r, 3, K)) * 30.0
    for p in range(r):
        a[p, :, int(rng.integers(2, K + 1)):] = 0.0
    x = 0.01 * rng.standard_normal(3 * K)
    if hold:
        Tm = T.reshape(6, -1)
        x = x - Tm.T @ np.linalg.solve(Tm @ Tm.T, Tm @ x)
    reach = a.reshape(r, -1) @ x
    if reach[0] < 0.0:                                       # (-x holds the terminal rows as well)
        x, reach = -x, -reach
    slack = rng.uniform(0.0, 0.3, r)
    slack[0] = 0.1 * reach[0]
    b = reach - slack
    umax = np.inf
    if ball:
        free = solve_qp(D, ubar, T, a, b, 1.0)
        assert free["status"] == ST_OK
        ut = ubar + free["du"]
        umax = 0.8 * np.sqrt((ut * ut).sum(axis=0)).max()
    return D, ubar, T, a, b, umax
